"""A/B of the two data planes of a robust aggregator / secure aggregation on a multi-rank engine
(``EngineConfig.gather_plane``): the host gather (every rank's buffer over gloo, the rule launched from
Python: the path before the xgmi plane existed) against the one-shot xGMI gather-select kernel, issued
eagerly and through captured graphs.

W ranks share ``cuda:0`` (a 1-GPU box has no xGMI links), so the ranks time-slice one GPU's CUs: the
numbers bound the HOST cost the xgmi plane removes (the gloo gather, the Python launches, the host round
trip that keeps rounds out of a graph); they are not the xGMI link time of a real node.

Per (world, rule, dtype): three engines on the same shards and seeds -- host plane, xgmi plane eager,
xgmi plane with ``graph_rounds`` -- run ``--rounds`` rounds each, interleaved ``--reps`` times; a timing
is the wall time of ``run(rounds)`` (which ends in a device synchronise) between two barriers, the
slowest rank's, per round.  The three engines must end with the same bits.

    python tools/gather_plane_ab.py [--worlds 2 4] [--rounds 200] [--reps 3] [--out profiles/gather_plane_ab.log]
"""
import argparse
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.multiprocessing as mp  # noqa: E402

DIMS = [14, 50, 200, 2]
RULES = {"median": dict(aggregator="median"), "secagg": dict(secagg=True, secagg_seed=1)}
WARM = 32


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, a, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), FEDMI_PEER_TIMEOUT_S="20")
    try:
        import gc

        import numpy as np
        import torch
        from fedmi.data.synthetic import make_income_like
        from fedmi.fl.engine import EngineConfig, HipRoundEngine
        from fedmi.models.mlp import init_flat
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="xgmi", device="cuda:0", rccl=False)
        X, y = make_income_like(a.rows, seed=40 + rank)
        flat = init_flat(DIMS, 3 + rank)
        total = WARM + a.reps * a.rounds
        rows = []
        for rule, kw in RULES.items():
            for dtype in ("fp32", "bf16"):
                engines = {}
                for name, plane, g in (("host", "host", 0), ("xgmi eager", "xgmi", 0), ("xgmi graph", "xgmi", a.graph_rounds)):
                    cfg = EngineConfig(hidden=tuple(DIMS[1:-1]), max_rounds=total, early_stop=False, dtype=dtype,
                                       graph_rounds=g, gather_plane=plane, **kw)
                    e = HipRoundEngine(X, y, 2, cfg, comm, flat, n_total=world * a.rows,
                                       client_sizes=[a.rows] * world)
                    want = "xgmi-select" if plane == "xgmi" else "host-gather"
                    if e.aggregation != want:
                        raise RuntimeError(f"{name}: aggregation {e.aggregation!r}, expected {want!r}")
                    e.run(WARM)   # code objects, the first graph capture, the ranks' start skew
                    engines[name] = e
                times = {name: [] for name in engines}
                for _ in range(a.reps):
                    for name, e in engines.items():
                        torch.cuda.synchronize()
                        comm.Barrier()
                        t0 = time.perf_counter()
                        e.run(a.rounds)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        times[name].append(max(comm.allgather(dt)) / a.rounds * 1e6)
                w = {name: e.global_flat() for name, e in engines.items()}
                same = all(np.array_equal(w["host"], v, equal_nan=True) for v in w.values())
                captures = int(engines["xgmi graph"].engine.graph_captures)
                rows.append((rule, dtype, times, same, captures))
                engines.clear()
                del e
                gc.collect()
        torch.cuda.synchronize()
        comm.Barrier()
        q.put((rank, rows, None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


def _run_world(world, a):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, a, q)) for r in range(world)]
    for p in procs:
        p.start()
    out, failed = [], None
    try:
        for _ in range(world):
            out.append(q.get(timeout=a.timeout))
    except Exception as e:  # noqa: BLE001 -- a rank hung or died: nothing more is started
        failed = f"world {world}: no result from a rank ({e!r})"
    for p in procs:
        p.join(timeout=5 if failed else 60)
        if p.is_alive():
            p.terminate()
            p.join(timeout=10)
            failed = failed or f"world {world}: a rank did not exit"
    for rank, _, err in out:
        if err is not None:
            failed = failed or f"world {world} rank {rank}:\n{err}"
    if failed:
        raise SystemExit(failed)
    return sorted(out, key=lambda t: t[0])[0][1]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--rows", type=int, default=1000, help="rows per rank's shard")
    ap.add_argument("--rounds", type=int, default=200, help="rounds per timing")
    ap.add_argument("--reps", type=int, default=3, help="timings per engine, interleaved")
    ap.add_argument("--graph-rounds", type=int, default=16)
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds to wait for a world's ranks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_plane_ab.log"))
    a = ap.parse_args(argv)
    lines = [f"gather_plane A/B: MLP {'-'.join(map(str, DIMS))}, {a.rows}-row shards, ranks sharing cuda:0 (they "
             f"time-slice its CUs), {a.rounds} rounds per timing, {a.reps} interleaved timings, us per round "
             f"(wall, slowest rank); graph_rounds = {a.graph_rounds}",
             f"{'world':>5} {'rule':>7} {'dtype':>5}  {'host-gather':>24}  {'xgmi-select eager':>24}  "
             f"{'xgmi-select graph':>24}  {'host/eager':>10} {'host/graph':>10}  same bits  captures"]
    med = lambda v: sorted(v)[len(v) // 2]
    fmt = lambda v: "/".join(f"{x:.1f}" for x in v)
    for world in a.worlds:
        for rule, dtype, times, same, captures in _run_world(world, a):
            h, e, g = (med(times[k]) for k in ("host", "xgmi eager", "xgmi graph"))
            lines.append(f"{world:>5} {rule:>7} {dtype:>5}  {fmt(times['host']):>24}  {fmt(times['xgmi eager']):>24}  "
                         f"{fmt(times['xgmi graph']):>24}  {h / e:>10.2f} {h / g:>10.2f}  {str(same):>9}  {captures:>8}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""Robust and secure aggregation on the xGMI peer plane (``gather_plane="xgmi"``): the one-shot
gather-select kernel (fedmi/ops/csrc/peer_allreduce.hip peer_select_kernel, peer_select.h) alone against
the host models, and multi-rank engines against ``ClientGroup`` bit for bit.

All ranks share ``cuda:0`` (a 1-GPU box has no xGMI links): every rank still maps the others'
allocations through HIP IPC and the publish / wait / pull protocol runs unchanged.  One spawn per
world; every case of that world runs inside the same workers; a missing result ends the spawn and no
later one starts.  The peer timeout is a few seconds, so a protocol bug ends as a reported
PEER_ERR_TIMEOUT failure word, not as a hang.

Bounds: none -- every comparison is equality of bits (any NaN matching any NaN, payloads are not part
of the rules): the kernel applies the very functions of fl_robust.hip / fl_secagg.hip, whose fp32 host
models (fedmi/fl/aggregate.py, fedmi/fl/secagg.py) are bit exact.
"""
import functools
import hashlib
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.aggregate import robust_aggregate_torch
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine
from fedmi.fl.secagg import secagg_mask, secagg_open, secagg_quantize
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KIND = {"median": 1, "trimmed_mean": 2}
TINY, INCOME, SMALL = [5, 4, 2], [14, 50, 200, 2], [17, 24, 3]
TAILS = 7
BITS = 20
PEER_TIMEOUT_S = 8.0
ROUNDS = 6
GROUP_EPS = 1e-4
ENGINE_CASES = {
    "median_fp32": dict(aggregator="median"),
    "median_bf16": dict(aggregator="median", dtype="bf16"),
    "trimmed_2of3": dict(aggregator="trimmed_mean", participation=0.67),
    "median_server": dict(aggregator="median", server_opt="sgd"),
    "secagg_dp": dict(secagg=True, secagg_seed=5, dp_clip=0.5, dp_noise=0.5, dp_seed=7),
}
ES = dict(aggregator="median", early_stop=True, patience=1, tolerance=0.5, max_rounds=16)


# ---- helpers shared by the workers and the parent ----
def _bits_equal(a, b):
    """None when equal bit for bit (any NaN matching any NaN), else a short description."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return f"shapes {a.shape} != {b.shape}"
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.int32) != b.view(np.int32)))
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        return f"{int(bad.sum())} of {a.size} differ, first at {i}: {a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r}"
    return None


def _state(live, r):
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"], rec["next_round"], rec["stop_round"] = int(live), r, r + 1, -1
    return torch.as_tensor(rec.view(np.uint8).copy()).to(DEV)


def _rtab(masks):
    t = np.zeros((len(masks), 4), np.uint32)
    for r, m in enumerate(masks):
        bits = sum(1 << int(k) for k in np.flatnonzero(m))
        t[r, 0] = np.float32(1.0).view(np.uint32)
        t[r, 1] = np.float32(m.sum()).view(np.uint32)
        t[r, 2], t[r, 3] = bits & 0xFFFFFFFF, bits >> 32
    return torch.as_tensor(t.reshape(-1).view(np.int32)).to(DEV)


def _fold(a):
    """fp32 left fold of the rows in rank order."""
    acc = torch.as_tensor(a[0]).clone()
    for row in a[1:]:
        acc += torch.as_tensor(row)
    return acc.numpy()


def _image_positions(dims):
    """Image position of every dense parameter, and the mask of real (non-padding) image floats."""
    P, pimg = param_count(dims), image_layout(dims)[2]
    img = dense_to_image(np.arange(1, P + 1, dtype=np.float32), dims)
    pos = np.flatnonzero(img != 0)
    pos = pos[np.argsort(img[pos])]
    assert pos.size == P and img.size == pimg
    real = np.zeros(pimg, bool)
    real[pos] = True
    return pos, real


def _crafted(dims, W, seed):
    """[W, Pimg + TAILS] seeded normals with, on known dense coordinates: values equal across ranks,
    -0 / +0 ties, a NaN rank, a +inf and a -inf rank; nonzero garbage (and a NaN) in rank 1's padding."""
    pos, real = _image_positions(dims)
    pimg = real.size
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((W, pimg + TAILS)).astype(np.float32)
    a[:, :pimg][:, ~real] = 0.0
    a[:, pos[2:6]] = a[0, pos[2:6]]
    a[:, pos[6:10]] = 0.0
    a[::2, pos[6:10]] = -0.0
    a[W // 2, pos[10:12]] = np.nan
    a[1, pos[12:14]] = np.inf
    a[W - 1, pos[14:16]] = -np.inf
    pad = np.flatnonzero(~real)
    a[1, pad] = 3.5
    a[1, pad[0]] = np.nan
    return a, pos, real


def _mask_cases(W):
    """All ranks sampled; rank 1 unsampled."""
    one = np.ones(W, bool)
    one[1] = False
    return [np.ones(W, bool), one]


# ---- 1. the kernel alone (runs inside the workers) ----
def _kernel_cases(comm, dims, errs, digests):
    from fedmi.parallel.peer import make_peer_allreduce
    W, rank = comm.size, comm.rank
    a, pos, real = _crafted(dims, W, 1000 + W)
    pimg, n = real.size, real.size + TAILS
    h = make_peer_allreduce(comm, n, comm.device, timeout_s=PEER_TIMEOUT_S)
    if h is None:
        errs.append(f"{dims}: the peer plane did not come up")
        return
    masks = _mask_cases(W)
    rtab = _rtab(masks)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    calls = [0]

    def call(rows, launch, tag):
        """This rank's row into its send buffer, the select call, the output; then a barrier: every
        rank has read this parity before anyone rewrites it."""
        par = calls[0] & 1
        calls[0] += 1
        h.write(par, 0, np.ascontiguousarray(rows[rank], np.float32).tobytes())
        out.fill_(7.0)
        launch(par)
        torch.cuda.synchronize()
        got = out.cpu().numpy().copy()
        comm.Barrier()
        digests.append((tag, hashlib.sha256(got.tobytes()).hexdigest()))
        return got

    def check(tag, got, want):
        d = _bits_equal(got, want)
        if d is not None:
            errs.append(f"W={W} {dims} {tag}: {d}")

    tails, whole = _fold(a[:, pimg:]), _fold(a)
    for kind, beta in (("median", 0.0), ("trimmed_mean", 0.25)):
        for r, mask in enumerate(masks):
            st = _state(1, r)
            tag = f"{kind} mask={np.flatnonzero(mask).tolist()}"
            got = call(a, lambda par: h.robust(par, dims, KIND[kind], beta, out.data_ptr(), st.data_ptr(),
                                               rtab.data_ptr(), len(masks), s), tag)
            model = robust_aggregate_torch(torch.as_tensor(a[:, :pimg]), mask, kind, beta).numpy()
            check(tag + ": image", got[:pimg][real], model[real])
            check(tag + ": padding", got[:pimg][~real], np.zeros(int((~real).sum()), np.float32))
            check(tag + ": tails", got[pimg:], tails)
        st = _state(0, 0)
        got = call(a, lambda par: h.robust(par, dims, KIND[kind], beta, out.data_ptr(), st.data_ptr(),
                                           rtab.data_ptr(), len(masks), s), f"{kind} not live")
        check(f"{kind} not live", got, whole)
    # secure aggregation: the words of secagg_mask under two seeds open to the same image
    c = (0.25 * a[:, :pimg][:, pos]).astype(np.float32)   # dense contributions, the planted NaN / inf included
    for r, mask in enumerate(masks):
        sampled = np.flatnonzero(mask).tolist()
        opened = []
        for seed in (11, 12):
            rows = a.copy()   # an unsampled rank's buffer stays clear floats; tails and padding as crafted
            ys = {}
            for i in sampled:
                q, _ = secagg_quantize(c[i], BITS, len(sampled))
                ys[i] = secagg_mask(q, i, sampled, r, seed)
                rows[i, pos] = ys[i].view(np.float32)
            st = _state(1, r)
            tag = f"secagg seed={seed} mask={sampled}"
            got = call(rows, lambda par: h.secagg_open(par, dims, BITS, out.data_ptr(), st.data_ptr(), rtab.data_ptr(),
                                                       len(masks), s), tag)
            want = secagg_open(np.stack([ys[i] for i in sampled]), BITS)
            check(tag + ": image", got[pos], want)
            check(tag + ": padding", got[:pimg][~real], np.zeros(int((~real).sum()), np.float32))
            check(tag + ": tails", got[pimg:], tails)
            opened.append(got)
        check(f"secagg mask={sampled}: the two seeds", opened[0], opened[1])
    st = _state(0, 0)
    got = call(a, lambda par: h.secagg_open(par, dims, BITS, out.data_ptr(), st.data_ptr(), rtab.data_ptr(),
                                            len(masks), s), "secagg not live")
    check("secagg not live", got, whole)
    if h.error() != 0:
        errs.append(f"W={W} {dims}: failure word {h.error():#x}")
    comm.Barrier()
    h.close()


# ---- 2. engines (run inside the workers) ----
def _data():
    return make_multiclass(240, 17, 3, DATA_SEED)


def _cfg(**kw):
    base = dict(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, eps=GROUP_EPS, trim_ratio=0.2)
    return EngineConfig(**{**base, **kw})


def _engine(comm, plane, **kw):
    from fedmi.data.sharding import shard_indices
    X, y = _data()
    W, rank = comm.size, comm.rank
    idx = [shard_indices(len(X), r, W, mode="iid", seed=2, labels=y, alpha=0.5) for r in range(W)]
    cfg = _cfg(gather_plane=plane, **kw)
    flat = init_flat(SMALL, 2 * 1000003 + (rank if cfg.server_opt == "none" else 0))
    return HipRoundEngine(X[idx[rank]], y[idx[rank]], 3, cfg, comm, flat, n_total=sum(len(i) for i in idx))


def _result(e):
    h = e.history()
    return {"aggregation": e.aggregation, "plane": e.layout["gather_plane"], "w": e.global_flat(), "global": h["global"],
            "loss": h["loss"], "per_rank": h["per_rank"], "rounds_run": h["rounds_run"], "stop_round": h["stop_round"],
            "clamped": h.get("secagg_clamped")}


def _engine_cases(comm, res):
    import gc
    for name, kw in ENGINE_CASES.items():
        e = _engine(comm, "xgmi", **kw)
        e.run(ROUNDS)
        res["engine:" + name] = _result(e)
        del e
        gc.collect()
    # early stop inside the run: 8 issued rounds against exactly stop_round rounds
    e = _engine(comm, "xgmi", **ES)
    e.run(8)
    res["es:long"] = _result(e)
    stop = int(res["es:long"]["stop_round"])
    del e
    gc.collect()
    e = _engine(comm, "xgmi", **ES)
    e.run(stop if stop > 0 else 2)
    res["es:exact"] = _result(e)
    del e
    gc.collect()
    # graph-replayed rounds against the eager ones of engine:median_fp32
    e = _engine(comm, "xgmi", aggregator="median", graph_rounds=4)
    primed = e.prime_graph(4)
    e.run(ROUNDS - primed)
    res["graph"] = dict(_result(e), primed=primed, captures=int(e.engine.graph_captures))
    del e
    gc.collect()
    e = _engine(comm, "host", aggregator="median")
    try:
        e.prime_graph(4)
        res["host_prime_graph"] = "no error"
    except RuntimeError as err:
        res["host_prime_graph"] = str(err)
    res["host_aggregation"] = e.aggregation
    del e
    gc.collect()


def _fallback_cases(comm, res):
    import gc
    e = _engine(comm, "xgmi", aggregator="median")
    e.run(ROUNDS)
    res["fb:xgmi"] = _result(e)
    del e
    gc.collect()
    os.environ["FEDMI_TEST_PEER_FAIL"] = "1"   # the set-up fails on rank 1: every rank falls back together
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            e = _engine(comm, "xgmi", aggregator="median")
    finally:
        del os.environ["FEDMI_TEST_PEER_FAIL"]
    res["fb:warnings"] = [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)]
    e.run(ROUNDS)
    res["fb:host"] = _result(e)
    del e
    gc.collect()


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), FEDMI_PEER_TIMEOUT_S=str(PEER_TIMEOUT_S))
    try:
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="xgmi", device="cuda:0", rccl=False)
        res = {"errs": [], "digests": []}
        for dims in (TINY, INCOME):
            _kernel_cases(comm, dims, res["errs"], res["digests"])
        if world == 3:
            _engine_cases(comm, res)
        if world == 2:
            _fallback_cases(comm, res)
        torch.cuda.synchronize()
        comm.Barrier()
        q.put((rank, res, None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


# ---- the parent: one spawn per world ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_SPAWN_FAILED = []


@functools.lru_cache(maxsize=None)
def _spawn(world):
    """Results of every rank of one spawn of `world` workers, or the reason it failed."""
    if _SPAWN_FAILED:
        return None, "an earlier spawn of this module failed; nothing more is started: " + _SPAWN_FAILED[0]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out, failed = [], None
    try:
        for _ in range(world):
            out.append(q.get(timeout=150))
    except Exception as e:  # noqa: BLE001 -- a child hung or died: reported below, nothing more runs
        failed = f"world {world}: no result from a rank ({e!r})"
    for p in procs:
        p.join(timeout=5 if failed else 30)
        if p.is_alive():
            p.terminate()
            p.join(timeout=10)
            failed = failed or f"world {world}: a rank did not exit"
    out.sort(key=lambda t: t[0])
    for rank, _, err in out:
        if err is not None and failed is None:
            failed = f"world {world} rank {rank}:\n{err}"
    if failed is None and not all(p.exitcode == 0 for p in procs):
        failed = f"world {world}: exit codes {[p.exitcode for p in procs]}"
    if failed is not None:
        _SPAWN_FAILED.append(failed)
        return None, failed
    return [res for _, res, _ in out], None


def _ranks(world):
    res, failed = _spawn(world)
    assert failed is None, failed
    return res


@pytest.mark.parametrize("world", [2, 3, 8])
def test_kernel_against_the_host_models(world):
    res = _ranks(world)
    for rank, r in enumerate(res):
        assert r["errs"] == [], f"rank {rank}: " + "\n".join(r["errs"][:8])
        # 2 shapes x (2 rules x (2 masks + not live) + 2 masks x 2 seeds + not live)
        assert len(r["digests"]) == 2 * (2 * 3 + 2 * 2 + 1)
    for r in res[1:]:
        assert r["digests"] == res[0]["digests"]       # every rank's output identical


def _group(k, **kw):
    X, y = _data()
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, _cfg(**kw), backend="hip", shard_mode="iid", seed=2)
    g.run(ROUNDS)
    return g


@pytest.mark.parametrize("case", sorted(ENGINE_CASES))
def test_engine_world3_equals_the_group_bitwise(case):
    res = _ranks(3)
    # (only now, with every child done and clean, the reference group runs on the GPU)
    g = _group(3, **ENGINE_CASES[case])
    h = g.history()
    for rank, r in enumerate(res):
        e = r["engine:" + case]
        assert e["aggregation"] == "xgmi-select" and e["plane"] == "xgmi", (rank, e["aggregation"], e["plane"])
        np.testing.assert_array_equal(e["w"], g.global_flat(), err_msg=f"rank {rank}")
        for key in ("global", "loss", "per_rank"):
            np.testing.assert_array_equal(e[key], h[key], err_msg=f"rank {rank} {key}")
        assert e["rounds_run"] == h["rounds_run"] == ROUNDS
        if case == "secagg_dp":
            np.testing.assert_array_equal(e["clamped"], g.clients[rank].history()["secagg_clamped"])


def test_rounds_past_an_early_stop_change_nothing():
    for rank, r in enumerate(_ranks(3)):
        a, b = r["es:long"], r["es:exact"]
        assert a["aggregation"] == "xgmi-select"
        assert 0 < a["stop_round"] < 8 and a["stop_round"] == b["stop_round"], (rank, a["stop_round"], b["stop_round"])
        assert a["rounds_run"] == b["rounds_run"] == a["stop_round"], (rank, a["rounds_run"], b["rounds_run"])
        np.testing.assert_array_equal(a["w"], b["w"])
        np.testing.assert_array_equal(a["global"], b["global"])


def test_graph_replayed_rounds_equal_eager_rounds():
    for rank, r in enumerate(_ranks(3)):
        g, e = r["graph"], r["engine:median_fp32"]
        assert g["aggregation"] == "xgmi-select" and g["captures"] >= 1 and g["primed"] == 4, (rank, g)
        assert g["rounds_run"] == ROUNDS
        for key in ("w", "global", "loss", "per_rank"):
            np.testing.assert_array_equal(g[key], e[key], err_msg=f"rank {rank} {key}")
        assert "aggregated from Python" in r["host_prime_graph"] and r["host_aggregation"] == "host-gather"


def test_fallback_to_the_host_gather():
    for rank, r in enumerate(_ranks(2)):
        x, f = r["fb:xgmi"], r["fb:host"]
        assert x["aggregation"] == "xgmi-select" and x["plane"] == "xgmi"
        assert f["aggregation"] == "host-gather" and f["plane"] == "host"
        assert len(r["fb:warnings"]) == 1 and "host gather" in r["fb:warnings"][0], r["fb:warnings"]
        for key in ("w", "global", "loss", "per_rank"):
            np.testing.assert_array_equal(x[key], f[key], err_msg=f"rank {rank} {key}")
        assert x["rounds_run"] == f["rounds_run"] == ROUNDS

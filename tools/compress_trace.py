"""Cost of the compression kernel (fl_compress.hip) and what compression does to convergence.

Timing: HipRoundEngine.trace (eager launches behind a gate kernel, a hipEvent marker after every
launch) of one client on the income CSV's 8000 training rows, 14-50-200-2, R = 32, fp32 and bf16:
the classic round (fused_eval=False), the same round with fl_dp clipping only (dp_noise = 0; the
nearest existing kernel of the same structure) and with each compressor.  Every case runs twice,
alternating, so a drift of the box shows as a difference between the passes.

Convergence (--convergence): rounds-to-target on the CSV with k = 8 clients in one process
(ClientGroup), dense / top-k 10 % / top-k 1 % / sign / qsgd s = 127 / qsgd s = 1 / rand-k 10 % /
rand-k 1 % (compress_seed = 1), with and without error feedback.  Reported, not asserted.

--cases old | new | all picks the deterministic cases (classic, dp-clip, top-k, sign: the ones an older
extension loaded through FEDMI_NATIVE_SO knows), the stochastic ones, or both; every line carries the
extension it ran on ("native_so").

One JSON line per case on stdout and in --out (default profiles/compress_trace.jsonl; --append adds to it).

    python tools/compress_trace.py [--rounds 200] [--cases all] [--convergence] [--out FILE] [--append]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("classic", {}), ("dp-clip", dict(dp_clip=1e-3, dp_noise=0.0, dp_seed=1)),
         ("topk-10%", dict(compress="topk", compress_ratio=0.1)), ("topk-1%", dict(compress="topk", compress_ratio=0.01)),
         ("sign", dict(compress="sign"))]
NEW_CASES = [("qsgd-127", dict(compress="qsgd", compress_levels=127, compress_seed=1)),
             ("qsgd-1", dict(compress="qsgd", compress_levels=1, compress_seed=1)),
             ("randk-10%", dict(compress="randk", compress_ratio=0.1, compress_seed=1)),
             ("randk-1%", dict(compress="randk", compress_ratio=0.01, compress_seed=1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--convergence", action="store_true", help="also the rounds-to-target table (k = 8 clients)")
    ap.add_argument("--backend", default="hip", help="--convergence: hip | torch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress_trace.jsonl"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--cases", choices=["old", "new", "all"], default="all",
                    help="old: classic, dp-clip, top-k, sign; new: qsgd, rand-k")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--no-trace", action="store_true", help="--convergence only")
    a = ap.parse_args()
    timed = {"old": CASES, "new": NEW_CASES, "all": CASES + NEW_CASES}[a.cases]
    conv = {"old": CASES[2:], "new": NEW_CASES, "all": CASES[2:] + NEW_CASES}[a.cases]
    so = os.environ.get("FEDMI_NATIVE_SO") or "tree"
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig, HipRoundEngine
    from fedmi.fl.simulate import rounds_to_target
    from fedmi.models.mlp import init_flat
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    flat = init_flat([X.shape[1], 50, 200, 2], 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a" if a.append else "w")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for dtype in ("fp32", "bf16") if not a.no_trace else ():
        for rep in range(a.passes):
            for name, kw in timed:
                cfg = EngineConfig(max_rounds=a.rounds + 16, early_stop=False, graph_rounds=0, dtype=dtype,
                                   rows_per_block=32, fused_eval=False, lagged_eval=False, **kw)
                e = HipRoundEngine(X, y, 2, cfg, None, flat)
                tr = e.trace(a.rounds, close=True, warm=8)
                emit({"what": "trace", "rows": int(len(X)), "dtype": dtype, "case": name, "pass": rep, "R": int(e.R),
                      "compress_layout": e.layout["compress"], "native_so": so,
                      **{k: (round(v, 2) if isinstance(v, float) else v) for k, v in tr.items()}})
    if a.convergence:
        table = ([("dense", {})] if a.cases != "new" else []) + [
            (f"{name} ef={int(ef)}", dict(error_feedback=ef, **kw)) for name, kw in conv for ef in (True, False)]
        for name, kw in table:
            cfg = EngineConfig(max_rounds=300, **kw)
            res = rounds_to_target(X, y, 8, cfg, backend=a.backend)
            from fedmi.fl.compress import compress_k, uplink_bytes
            P = len(flat)
            emit({"what": "rounds_to_target", "clients": 8, "backend": a.backend, "case": name,
                  "uplink_bytes": uplink_bytes(cfg.compress, compress_k(cfg, P), P, cfg.compress_levels), **res})
    out.close()


if __name__ == "__main__":
    main()

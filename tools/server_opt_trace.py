"""Cost of the server-optimizer kernel (fl_server.hip): HipRoundEngine.trace of one client on the
income CSV's 8000 training rows, 14-50-200-2, fp32 and bf16 -- the classic round without a server
optimizer (fused_eval=False, lagged_eval=False) against the same round with each server optimizer.
Prints one JSON line per case: mean us per round by kernel kind, the whole round, launch counts.

    python tools/server_opt_trace.py [--rounds 200] [--classic-only]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--classic-only", action="store_true", help="only the round without a server optimizer")
    a = ap.parse_args()
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig, HipRoundEngine
    from fedmi.models.mlp import init_flat
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    flat = init_flat([X.shape[1], 50, 200, 2], 1)
    opts = ["none"] if a.classic_only else ["none", "sgd", "adagrad", "adam", "yogi"]
    for dtype in ("fp32", "bf16"):
        for opt in opts:
            kw = {} if opt == "none" else dict(server_opt=opt, server_lr=1.0 if opt == "sgd" else 1e-2)
            cfg = EngineConfig(max_rounds=a.rounds + 16, early_stop=False, graph_rounds=0, dtype=dtype,
                               fused_eval=False, lagged_eval=False, **kw)
            e = HipRoundEngine(X, y, 2, cfg, None, flat)
            tr = e.trace(a.rounds, close=True, warm=8)
            row = {"rows": int(len(X)), "dtype": dtype, "server_opt": opt, "R": int(e.R),
                   **{k: (round(v, 2) if isinstance(v, float) else v) for k, v in tr.items()}}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

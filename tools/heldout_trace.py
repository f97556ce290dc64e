"""Cost of the held-out scoring launches (fl_heldout.hip): HipRoundEngine.trace of one client on the income
CSV's 8000 training rows, 14-50-200-2, fp32 and bf16, classic rounds (fused_eval=False, so the round has
an `eval` interval to compare with) -- without a held-out set, with the 2000-row test split and with
8000 held-out rows (the training rows again).  The `heldout` interval is the row launch plus the fold
launch; the row kernel does the fp32 eval kernel's work on as many rows, so the expectation is about the
fp32 `eval` interval at equal rows plus one small launch.  Prints one JSON line per case: mean us per
round by kernel kind, the whole round, launch counts.

    python tools/heldout_trace.py [--rounds 200]
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
    a = ap.parse_args()
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig, HipRoundEngine
    from fedmi.models.mlp import init_flat
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    flat = init_flat([X.shape[1], 50, 200, 2], 1)
    sets = {0: None, int(len(ds.X_test)): (ds.X_test, ds.y_test), int(len(X)): (X, y)}
    for dtype in ("fp32", "bf16"):
        for n_val, held in sets.items():
            cfg = EngineConfig(max_rounds=a.rounds + 16, early_stop=False, graph_rounds=0, dtype=dtype,
                               fused_eval=False, lagged_eval=False)
            e = HipRoundEngine(X, y, 2, cfg, None, flat)
            if held is not None:
                e.set_heldout(held[0], held[1], keep_best=True)
            tr = e.trace(a.rounds, close=True, warm=8)
            row = {"rows": int(len(X)), "dtype": dtype, "n_val": n_val, "R": int(e.R),
                   **{k: (round(v, 2) if isinstance(v, float) else v) for k, v in tr.items()}}
            if held is not None:
                row["heldout_over_eval"] = round(tr["heldout"] / tr["eval"], 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()

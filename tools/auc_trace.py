"""Cost of the held-out AUC launches (fl_auc.hip) beside the held-out pair (fl_heldout.hip):
HipRoundEngine.trace of one client on the income CSV's 8000 training rows, 14-50-200-2, fp32, classic
rounds, with a held-out set of 2000 rows (the CSV's test split) and of 32768 rows (the rank kernel's cap: the
training rows repeated with a little seeded noise), each with AUC off and on.  The passes alternate
between the two engines of a size, so both see the same machine; every pass is eager launches behind a
gate with an event marker after each.  `heldout` is the row launch plus the fold launch, `heldout_auc`
the key launch plus the rank launch, split under `heldout_auc_keys` / `heldout_auc_rank`.  Prints one
JSON line per (size, auc): mean us per round over the passes by launch kind, and each pass's figures.

    python tools/auc_trace.py [--rounds 200] [--passes 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("train", "adam", "eval", "heldout", "heldout_auc", "heldout_auc_keys", "heldout_auc_rank", "round")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import AUC_MAX_ROWS, EngineConfig, HipRoundEngine
    from fedmi.models.mlp import init_flat
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    flat = init_flat([X.shape[1], 50, 200, 2], 1)
    rng = np.random.default_rng(0)
    idx = np.arange(AUC_MAX_ROWS) % len(X)
    big = (X[idx] + 1e-3 * rng.standard_normal((AUC_MAX_ROWS, X.shape[1]))).astype(np.float32)
    sets = {int(len(ds.X_test)): (ds.X_test, ds.y_test), AUC_MAX_ROWS: (big, y[idx])}
    warm = 8
    for n_val, held in sets.items():
        engines = {}
        for auc in (False, True):
            cfg = EngineConfig(max_rounds=a.passes * (a.rounds + warm) + 16, early_stop=False, graph_rounds=0,
                               dtype="fp32", fused_eval=False, lagged_eval=False)
            engines[auc] = HipRoundEngine(X, y, 2, cfg, None, flat)
            engines[auc].set_heldout(held[0], held[1], auc=auc)
        per_pass = {False: [], True: []}
        for _ in range(a.passes):
            for auc in (False, True):
                tr = engines[auc].trace(a.rounds, close=True, warm=warm)
                per_pass[auc].append({k: round(float(tr[k]), 2) for k in KINDS if k in tr})
        for auc in (False, True):
            mean = {k: round(float(np.mean([p[k] for p in per_pass[auc]])), 2) for k in per_pass[auc][0]}
            print(json.dumps({"what": "trace", "rows": int(len(X)), "dtype": "fp32", "n_val": n_val, "auc": auc,
                              "rounds": a.rounds, **mean, "passes": per_pass[auc]}), flush=True)


if __name__ == "__main__":
    main()

"""SCAFFOLD on BASELINE config 4: 8 clients, Dirichlet label-skew shards (alpha 0.3), 5 local Adam steps per
round, 50 rounds; held-out accuracy of the global model for FedAvg, FedProx (mu 0.01 / 0.1) and SCAFFOLD (alone and
with mu 0.01).  Every case starts all clients from one common model (``server_opt="sgd"``, lr 1, momentum 0 -- the
identity server step up to one rounding), so the four differ in the drift remedy alone.

The 8 clients run in one process (fedmi/fl/simulate.py): ``--backend hip`` on one GPU, ``--backend torch`` the eager
specification on CPU.  The table is the point, not a win: with Adam as the local optimizer nobody has measured
whether the correction helps on this data.

    python tools/scaffold_config4.py --backend hip --out profiles/scaffold_config4_hip.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("fedavg", {}), ("fedprox mu 0.01", dict(prox_mu=0.01)), ("fedprox mu 0.1", dict(prox_mu=0.1)),
         ("scaffold", dict(scaffold=True)), ("scaffold + mu 0.01", dict(scaffold=True, prox_mu=0.01))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="hip", choices=["hip", "torch"])
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.metrics import metrics_from_confusion
    from fedmi.fl.simulate import ClientGroup
    if a.backend == "torch":
        torch.set_num_threads(1)
    ds = load_tabular()
    res = []
    for name, kw in CASES:
        for seed in a.seeds:
            cfg = EngineConfig(max_rounds=a.rounds, local_steps=5, early_stop=False, graph_rounds=0, server_opt="sgd",
                               server_lr=1.0, server_momentum=0.0, **kw)
            g = ClientGroup(ds.X_train, ds.y_train, a.clients, cfg, backend=a.backend, shard_mode="label_skew",
                            alpha=a.alpha, seed=seed)
            t0 = time.perf_counter()
            g.run(a.rounds)
            dt = time.perf_counter() - t0
            cm = g.clients[0].confusion(ds.X_test, ds.y_test, flat=g.global_flat())
            h = g.history()
            row = {"backend": a.backend, "clients": a.clients, "alpha": a.alpha, "case": name, "seed": seed,
                   "rounds": int(h["rounds_run"]), "train_global_last": [float(x) for x in h["global"][-1]],
                   "loss_last": float(h["loss"][-1]), "heldout_accuracy": float(metrics_from_confusion(cm)["accuracy"]),
                   "scaffold_norm_last": float(h["scaffold_norm"][-1]) if "scaffold_norm" in h else None, "wall_s": dt}
            res.append(row)
            print(json.dumps(row), flush=True)
        acc = [r["heldout_accuracy"] for r in res if r["case"] == name]
        print(json.dumps({"case": name, "heldout_accuracy_mean": float(np.mean(acc)), "min": min(acc), "max": max(acc)}),
              flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Server optimizers on BASELINE config 4: 8 clients, Dirichlet label-skew shards (alpha 0.3), 5 local
Adam steps per round, 50 rounds; held-out accuracy of the global model for plain FedAvg, FedAvgM
(sgd, momentum 0.9) and FedAdam / FedYogi (tau 1e-3, b1 0.9, b2 0.99) at the given server
learning rates, without and with client-level DP (``--dp-clip S --dp-noise Z``).

The 8 clients run in one process (fedmi/fl/simulate.py): ``--backend hip`` on one GPU, ``--backend
torch`` the eager oracle on CPU.  With a server optimizer every client starts from one common model
(plain FedAvg keeps the reference's per-client inits).

    python tools/server_opt_config4.py --backend hip --out profiles/server_opt_config4_hip.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="hip", choices=["hip", "torch"])
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--sgd-lr", type=float, nargs="+", default=[1.0, 0.1])
    ap.add_argument("--adaptive-lr", type=float, nargs="+", default=[1e-2, 10 ** -1.5])
    ap.add_argument("--dp-clip", type=float, default=0.0)
    ap.add_argument("--dp-noise", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.metrics import metrics_from_confusion
    from fedmi.fl.simulate import ClientGroup
    if a.backend == "torch":
        torch.set_num_threads(1)
    ds = load_tabular()
    # (FedAvgM at lr 1 takes steps of up to 1 / (1 - 0.9) = 10 averaged updates; lr 0.1 keeps the step size of FedAvg)
    cases = [("none", {})] + [(f"sgd lr {lr:.3g}", dict(server_opt="sgd", server_lr=lr, server_momentum=0.9))
                              for lr in a.sgd_lr]
    for opt in ("adam", "yogi"):
        cases += [(f"{opt} lr {lr:.3g}", dict(server_opt=opt, server_lr=lr, server_tau=1e-3)) for lr in a.adaptive_lr]
    dp = dict(dp_clip=a.dp_clip, dp_noise=a.dp_noise, dp_seed=20240607) if a.dp_clip > 0 else {}
    res = []
    for name, kw in cases:
        cfg = EngineConfig(max_rounds=a.rounds, local_steps=5, early_stop=False, dtype=a.dtype, **kw, **dp)
        g = ClientGroup(ds.X_train, ds.y_train, a.clients, cfg, backend=a.backend, shard_mode="label_skew",
                        alpha=a.alpha, seed=0)
        t0 = time.perf_counter()
        g.run(a.rounds)
        dt = time.perf_counter() - t0
        cm = g.clients[0].confusion(ds.X_test, ds.y_test, flat=g.global_flat())
        h = g.history()
        row = {"backend": a.backend, "dtype": a.dtype, "clients": a.clients, "case": name, "server": kw, "dp": dp,
               "rounds": int(h["rounds_run"]), "train_global_last": [float(x) for x in h["global"][-1]],
               "heldout_accuracy": float(metrics_from_confusion(cm)["accuracy"]), "wall_s": dt}
        res.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

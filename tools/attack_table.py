"""The defence x attack table: which aggregation rule survives which Byzantine attack model on the income data.

``ClientGroup(k=8)`` on the income CSV's 8000 training rows, iid shards, clients 1 and 4 Byzantine, 50 rounds
of the default 14-50-200-2 model in fp32 without early stopping; every cell is the global model's accuracy on
the held-out 20 % split after the last round (and, beside it, the best round's).  Rows: the weighted mean,
the coordinate-wise median, the 0.25-trimmed mean, the geometric median, multi-Krum (f = 2) in front of the
mean.  Columns: no attack, sign_flip (s = 1), gauss (sigma = 1), alie with the default z (for n = 8, f = 2
that is Phi^-1(0.5) = 0: the bad clients publish the honest mean) and with z = 1.5, ipm with eps = 0.1 and
eps = 100, label_flip.  A cell whose model is not finite is recorded as null.

Nothing about these numbers is asserted anywhere: the table records what came out.  ``--out`` is updated in
place, one entry per backend, so the HIP cells (measured on the GPU the entry names) and the torch cells (the
CPU oracle) can be filled by separate runs; every entry carries the digest of the sources it ran from.

    python tools/attack_table.py [--backend hip|torch|both] [--rounds 50] [--out profiles/attack_table.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BAD = (1, 4)
DEFENCES = {
    "mean": dict(aggregator="mean"),
    "median": dict(aggregator="median"),
    "trimmed_mean 0.25": dict(aggregator="trimmed_mean", trim_ratio=0.25),
    "geomed": dict(aggregator="geomed"),
    "multi_krum f=2 + mean": dict(aggregator="mean", screen="multi_krum", screen_byzantine=2),
}
ATTACK_COLUMNS = {
    "none": dict(),
    "sign_flip": dict(attack="sign_flip", attack_clients=BAD),
    "gauss": dict(attack="gauss", attack_clients=BAD),
    "alie": dict(attack="alie", attack_clients=BAD),
    "alie z 1.5": dict(attack="alie", attack_clients=BAD, attack_z=1.5),
    "ipm eps 0.1": dict(attack="ipm", attack_clients=BAD, attack_scale=0.1),
    "ipm eps 100": dict(attack="ipm", attack_clients=BAD, attack_scale=100.0),
    "label_flip": dict(attack="label_flip", attack_clients=BAD),
}


def run_backend(backend: str, rounds: int, ds) -> dict:
    from fedmi.fl.engine import EngineConfig, heldout_metrics
    from fedmi.fl.simulate import ClientGroup
    table = {}
    for dname, dkw in DEFENCES.items():
        table[dname] = {}
        for aname, akw in ATTACK_COLUMNS.items():
            cfg = EngineConfig(max_rounds=rounds, early_stop=False, graph_rounds=0, **dkw, **akw)
            g = ClientGroup(ds.X_train, ds.y_train, 8, cfg, backend=backend, shard_mode="iid", seed=0,
                            heldout=(ds.X_test, ds.y_test))
            g.run(rounds)
            acc = heldout_metrics(g.history())[:, 0]
            ok = bool(np.isfinite(g.global_flat()).all())
            table[dname][aname] = {"final": round(float(acc[-1]), 4) if ok else None,
                                   "best": round(float(np.nanmax(acc)), 4), "best_round": int(np.nanargmax(acc)) + 1}
            print(f"{backend:5s} {dname:22s} {aname:12s} final {table[dname][aname]['final']}  "
                  f"best {table[dname][aname]['best']} @ {table[dname][aname]['best_round']}", flush=True)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["hip", "torch", "both"], default="both")
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attack_table.json"))
    a = ap.parse_args()
    from fedmi.data.tabular import load_tabular
    from fedmi.ops.build import source_digest
    ds = load_tabular(with_mean=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["setup"] = {"data": "income CSV", "train_rows": int(len(ds.X_train)), "heldout_rows": int(len(ds.X_test)),
                    "clients": 8, "shards": "iid", "bad_clients": list(BAD), "rounds": a.rounds, "dtype": "fp32",
                    "model": "14-50-200-2", "metric": "held-out accuracy of the global model (final / best round)",
                    "alie_z": "default: Phi^-1((n - f - s) / (n - f)) for n = 8, f = 2", "sign_flip_s": 1.0,
                    "gauss_sigma": 1.0}
    doc.setdefault("backends", {})
    for backend in (("hip", "torch") if a.backend == "both" else (a.backend,)):
        t0 = time.perf_counter()
        table = run_backend(backend, a.rounds, ds)
        doc["backends"][backend] = {
            "measured_on": torch.cuda.get_device_name(0) if backend == "hip" else "CPU (torch oracle)",
            "source_digest": source_digest(), "wall_s": round(time.perf_counter() - t0, 1), "table": table}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Cost of the coalition launches (fl_coalition.hip) and of a client-group round with contribution scores.

The protocol of tools/robust_trace.py: eager launches with event markers, ``--rounds`` (200) timed after a warm-up,
every case run ``--passes`` (2) times with the cases alternating, one JSON line per case and pass:

* ``kernel``: at the 14-50-200-2 image and 2000 held-out rows, the ``coalition_build`` launch and the
  ``coalition_score`` pair (rows + fold) for "loo" at K = 8 (M = 9), exact Shapley at K = 4 and 8 (M = 16, 256) and
  permutations at K = 16, m = 8 (M = 129); the score pair both with its row slices (one image stage per workgroup)
  and with one workgroup per (coalition, row block);
* ``round``: the whole ``ClientGroup(backend="hip", k=8)`` round on the income CSV's 8000 training rows (fp32)
  with ``contribution`` "none", "loo" and "shapley", scored on the CSV's test rows.

Each interval carries the eager launch + event marker cost.

    python tools/coalition_trace.py [--rounds 200] [--passes 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.robust_trace import DIMS, _stats, _time  # noqa: E402

ROWS, R = 2000, 32
TABLES = [("loo", 8, 0), ("shapley", 4, 0), ("shapley", 8, 0), ("shapley", 16, 8)]


def _kernel_case(m, rounds, mode, K, perms):
    from fedmi.fl.contribution import coalition_masks
    from fedmi.fl.engine import _STATE_DTYPE
    from fedmi.models.mlp import dense_to_image, image_layout, init_flat
    dev, pimg = torch.device("cuda"), image_layout(DIMS)[2]
    stream = torch.cuda.Stream()
    masks = coalition_masks(mode, K, perms, 0)
    M, n_blk = len(masks), -(-ROWS // R)
    base = dense_to_image(init_flat(DIMS, 1), DIMS)
    rng = np.random.default_rng(K)
    bufs = [torch.as_tensor(base * np.float32(1.0 / K) * (1 + 0.01 * rng.standard_normal(pimg).astype(np.float32))).to(dev)
            for _ in range(K)]
    tab = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=dev)
    x, md = torch.as_tensor(base).to(dev), torch.as_tensor(masks.view(np.int64).copy()).to(dev)
    cw = torch.full((K,), 1.0 / K, device=dev)
    X = torch.as_tensor(rng.standard_normal((ROWS, DIMS[0])).astype(np.float32)).to(dev)
    y = torch.as_tensor(rng.integers(0, DIMS[-1], ROWS).astype(np.int32)).to(dev)
    scratch = torch.zeros(m.coalition_scratch_floats(DIMS, M, ROWS, R), device=dev)
    loss, correct = torch.zeros(M, device=dev), torch.zeros(M, dtype=torch.int32, device=dev)
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"] = 1, 0
    state = torch.as_tensor(rec.view(np.uint8).copy()).to(dev)
    bits = (1 << K) - 1
    rt = np.zeros(4, np.uint32)
    rt[0], rt[1], rt[2], rt[3] = np.float32(1).view(np.uint32), np.float32(K).view(np.uint32), bits & 0xFFFFFFFF, bits >> 32
    rtab = torch.as_tensor(rt.view(np.int32)).to(dev)
    torch.cuda.synchronize()

    def build(keep=bufs):   # (the table holds addresses: the closure keeps the buffers)
        m.coalition_build(DIMS, tab.data_ptr(), K, x.data_ptr(), md.data_ptr(), M, cw.data_ptr(), scratch.data_ptr(),
                          state.data_ptr(), rtab.data_ptr(), 1, stream.cuda_stream)

    def score(slices):
        m.coalition_score(DIMS, R, K, M, scratch.data_ptr(), X.data_ptr(), y.data_ptr(), ROWS, loss.data_ptr(),
                          correct.data_ptr(), state.data_ptr(), 1, stream.cuda_stream, slices)

    tag = {"case": "kernel", "mode": mode, "K": K, "M": M, "rows": ROWS}
    return [({**tag, "what": "build", "launches": 1}, lambda: _time(build, rounds, 20, stream)),
            ({**tag, "what": "score", "slices": m.coalition_slices(M, n_blk), "launches": 2},
             lambda: _time(lambda: score(0), rounds, 20, stream)),
            ({**tag, "what": "score, one workgroup per (m, row block)", "slices": n_blk, "launches": 2},
             lambda: _time(lambda: score(n_blk), rounds, 20, stream))]


def round_cases(rounds):
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    for mode in ("none", "loo", "shapley"):
        def run(mode=mode):
            cfg = EngineConfig(max_rounds=rounds + 24, early_stop=False, graph_rounds=0, contribution=mode)
            g = ClientGroup(X, y, 8, cfg, backend="hip", shard_mode="iid", seed=0, heldout=(ds.X_test, ds.y_test))
            state = {"r": 0}

            def one():
                g._round_hip(state["r"])
                state["r"] += 1
            us = _time(one, rounds, 16, g.stream)
            g.rounds = state["r"]
            g.sync_history()
            assert g.history()["rounds_run"] == rounds + 16
            return us
        yield {"case": "round", "contribution": mode, "K": 8, "rows": int(len(X)), "heldout": int(len(ds.X_test))}, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    from fedmi.ops import native
    m = native()
    cases = [c for t in TABLES for c in _kernel_case(m, a.rounds, *t)] + list(round_cases(a.rounds))
    for p in range(a.passes):
        for tag, fn in cases:
            print(json.dumps({**tag, "pass": p, "n": a.rounds, **_stats(fn())}), flush=True)


if __name__ == "__main__":
    main()

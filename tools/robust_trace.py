"""Cost of the robust-aggregation kernel (fl_robust.hip) and of a client-group round around it.

Eager launches with event markers, ``--rounds`` (200) timed launches after a warm-up, every case run
``--passes`` (2) times with the cases alternating, one JSON line per case and pass:

* ``kernel``: one ``robust_aggregate`` launch, in place over K = 4, 8, 64 buffers of the 14-50-200-2
  image + K metric tails (median and trimmed mean), and beside it the sum it replaces in a client
  group -- the ``tot`` fold (1 copy, K - 1 adds) plus K copies, 2 K launches -- on the same buffers;
* ``round``: the whole ``ClientGroup(backend="hip", k=8)`` round on the income CSV's 8000 training
  rows (fp32), with ``aggregator="mean"`` (the fold-and-copy round, unchanged by the robust path),
  ``"median"`` and ``"trimmed_mean"``.

Each interval carries the eager launch + event marker cost.

    python tools/robust_trace.py [--rounds 200] [--passes 2]
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

DIMS = [14, 50, 200, 2]


def _stats(us):
    us = np.sort(np.asarray(us))
    return {"mean_us": round(float(us.mean()), 2), "median_us": round(float(np.median(us)), 2),
            "p10_us": round(float(us[len(us) // 10]), 2), "p90_us": round(float(us[(9 * len(us)) // 10]), 2)}


def _time(fn, n, warm, stream):
    """us of each of ``n`` calls of ``fn`` on ``stream`` (event pair around every call)."""
    with torch.cuda.stream(stream):
        for _ in range(warm):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
    stream.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev]


def _kernel_case(m, rounds, K):
    from fedmi.fl.engine import _STATE_DTYPE
    from fedmi.models.mlp import image_layout
    dev = torch.device("cuda")
    pimg = image_layout(DIMS)[2]
    stream = torch.cuda.Stream()
    tails = K * 5
    g = torch.Generator(device="cpu").manual_seed(K)
    bufs = [torch.randn(pimg + tails, generator=g).to(dev) for _ in range(K)]
    tab = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=dev)
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"] = 1, 0
    state = torch.as_tensor(rec.view(np.uint8).copy()).to(dev)
    bits = (1 << K) - 1
    rt = np.zeros(4, np.uint32)
    rt[0], rt[1] = np.float32(1).view(np.uint32), np.float32(K).view(np.uint32)
    rt[2], rt[3] = bits & 0xFFFFFFFF, bits >> 32
    rtab = torch.as_tensor(rt.view(np.int32)).to(dev)
    tot = torch.empty_like(bufs[0])
    torch.cuda.synchronize()

    def fold_and_copy():   # (the sums grow to inf over the repetitions: an add costs the same)
        tot.copy_(bufs[0])
        for b in bufs[1:]:
            tot.add_(b)
        for b in bufs:
            b.copy_(tot)

    def launch(kind):
        m.robust_aggregate(DIMS, kind, 0.1, tab.data_ptr(), K, tab.data_ptr(), K, state.data_ptr(), rtab.data_ptr(),
                           tails, 1, stream.cuda_stream)

    return [({"case": "kernel", "what": "median", "K": K, "launches": 1},
             lambda: _time(lambda: launch(1), rounds, 20, stream)),
            ({"case": "kernel", "what": "trimmed_mean", "K": K, "launches": 1},
             lambda: _time(lambda: launch(2), rounds, 20, stream)),
            ({"case": "kernel", "what": "fold+copies", "K": K, "launches": 2 * K},
             lambda: _time(fold_and_copy, rounds, 20, stream))]


def kernel_cases(m, rounds):
    return [c for K in (4, 8, 64) for c in _kernel_case(m, rounds, K)]


def round_cases(rounds):
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    for agg in ("mean", "median", "trimmed_mean"):
        def run(agg=agg):
            cfg = EngineConfig(max_rounds=rounds + 24, early_stop=False, graph_rounds=0, aggregator=agg)
            g = ClientGroup(X, y, 8, cfg, backend="hip", shard_mode="iid", seed=0)
            state = {"r": 0}

            def one():
                g._round_hip(state["r"])
                state["r"] += 1
            us = _time(one, rounds, 16, g.stream)
            g.rounds = state["r"]
            g.sync_history()
            assert g.history()["rounds_run"] == rounds + 16
            return us
        yield {"case": "round", "what": agg, "K": 8, "rows": int(len(X)), "dtype": "fp32"}, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    from fedmi.ops import native
    m = native()
    cases = list(kernel_cases(m, a.rounds)) + list(round_cases(a.rounds))
    for p in range(a.passes):
        for tag, fn in cases:
            print(json.dumps({**tag, "pass": p, "n": a.rounds, **_stats(fn())}), flush=True)


if __name__ == "__main__":
    main()

"""Cost of the secure-aggregation kernels (fl_secagg.hip) and of a client-group round around them.

Eager launches with event markers, ``--rounds`` (200) timed launches after a warm-up, every case run
``--passes`` (2) times with the cases alternating, one JSON line per case and pass:

* ``kernel``: one ``secagg_mask`` launch over K = 4, 8, 64 buffers of the 14-50-200-2 image + K metric
  tails (the clear contributions are restored before every timed launch, outside the interval: masking
  masked words again would count clamps no real round has), one ``secagg_open`` launch in place over
  the same buffers, and beside them the sum they replace in a client group -- the ``tot`` fold (1 copy,
  K - 1 adds) plus K copies, 2 K launches -- on the same buffers;
* ``round``: the whole ``ClientGroup(backend="hip", k=8)`` round on the income CSV's 8000 training
  rows (fp32), with ``secagg=False`` (the fold-and-copy round, unchanged by this path) and ``True``.

Each interval carries the eager launch + event marker cost.

    python tools/secagg_trace.py [--rounds 200] [--passes 2] [--out profiles/secagg_trace.jsonl]
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
BITS = 24
SEED = 0x5EC0A66


def _stats(us):
    us = np.sort(np.asarray(us))
    return {"mean_us": round(float(us.mean()), 2), "median_us": round(float(np.median(us)), 2),
            "p10_us": round(float(us[len(us) // 10]), 2), "p90_us": round(float(us[(9 * len(us)) // 10]), 2)}


def _time(fn, n, warm, stream, prep=None):
    """us of each of ``n`` calls of ``fn`` on ``stream`` (event pair around every call; ``prep`` runs
    before each, outside the interval)."""
    with torch.cuda.stream(stream):
        for _ in range(warm):
            if prep is not None:
                prep()
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            if prep is not None:
                prep()
            a.record(stream)
            fn()
            b.record(stream)
    stream.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev]


def _kernel_case(m, rounds, K):
    from fedmi.fl.engine import _STATE_DTYPE
    from fedmi.models.mlp import dense_to_image, image_layout, param_count
    dev = torch.device("cuda")
    pimg = image_layout(DIMS)[2]
    stream = torch.cuda.Stream()
    tails = K * 5
    rng = np.random.default_rng(K)
    rows = np.zeros((K, pimg + tails), np.float32)
    for k in range(K):   # weighted contributions: O(1 / K) at the real parameters, +0 padding
        rows[k, :pimg] = dense_to_image((rng.standard_normal(param_count(DIMS)) / K).astype(np.float32), DIMS)
    rows[:, pimg:] = rng.standard_normal((K, tails))
    clear = torch.as_tensor(rows).to(dev)
    stack = torch.empty_like(clear)
    bufs = [stack[k] for k in range(K)]
    tab = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=dev)
    clamp = torch.zeros((K, 1), dtype=torch.int32, device=dev)
    ctab = torch.tensor([clamp[k].data_ptr() for k in range(K)], dtype=torch.int64, device=dev)
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

    def restore():
        stack.copy_(clear)

    def fold_and_copy():
        tot.copy_(bufs[0])
        for b in bufs[1:]:
            tot.add_(b)
        for b in bufs:
            b.copy_(tot)

    def mask():
        m.secagg_mask(DIMS, BITS, SEED, tab.data_ptr(), K, 0, state.data_ptr(), rtab.data_ptr(), ctab.data_ptr(), 1,
                      stream.cuda_stream)

    def masked():
        restore()
        mask()

    def open_():
        m.secagg_open(DIMS, BITS, tab.data_ptr(), K, tab.data_ptr(), K, state.data_ptr(), rtab.data_ptr(), tails, 1,
                      stream.cuda_stream)

    def checked(fn):
        def run():
            us = fn()
            assert int(clamp.sum()) == 0, "the timed launches clamped"
            return us
        return run

    return [({"case": "kernel", "what": "secagg_mask", "K": K, "launches": 1},
             checked(lambda: _time(mask, rounds, 20, stream, prep=restore))),
            ({"case": "kernel", "what": "secagg_open", "K": K, "launches": 1},
             lambda: _time(open_, rounds, 20, stream, prep=masked)),
            ({"case": "kernel", "what": "fold+copies", "K": K, "launches": 2 * K},
             lambda: _time(fold_and_copy, rounds, 20, stream, prep=restore))]


def kernel_cases(m, rounds):
    return [c for K in (4, 8, 64) for c in _kernel_case(m, rounds, K)]


def round_cases(rounds):
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    for on in (False, True):
        def run(on=on):
            cfg = EngineConfig(max_rounds=rounds + 24, early_stop=False, graph_rounds=0, secagg=on, secagg_bits=BITS,
                               secagg_seed=SEED)
            g = ClientGroup(X, y, 8, cfg, backend="hip", shard_mode="iid", seed=0)
            state = {"r": 0}

            def one():
                g._round_hip(state["r"])
                state["r"] += 1
            us = _time(one, rounds, 16, g.stream)
            g.rounds = state["r"]
            g.sync_history()
            assert g.history()["rounds_run"] == rounds + 16
            assert not on or not g.history()["secagg_clamped"].any()
            return us
        yield {"case": "round", "what": "secagg" if on else "fold+copies", "K": 8, "rows": int(len(X)),
               "dtype": "fp32"}, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    from fedmi.ops import native
    m = native()
    cases = list(kernel_cases(m, a.rounds)) + list(round_cases(a.rounds))
    out = open(a.out, "a") if a.out else None
    for p in range(a.passes):
        for tag, fn in cases:
            line = json.dumps({**tag, "pass": p, "n": a.rounds, **_stats(fn())})
            print(line, flush=True)
            if out is not None:
                out.write(line + "\n")
                out.flush()
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()

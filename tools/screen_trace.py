"""Cost of the multi-Krum screening kernels (fl_screen.hip) and of a client-group round with them.

Eager launches with event markers, ``--rounds`` (200) timed launches after a warm-up, every case run
``--passes`` (2) times with the cases alternating, one JSON line per case and pass:

* ``kernel``: over K = 4, 8, 64 buffers of the 14-50-200-2 image + K metric tails, one ``screen_dist``
  launch at every tile size the kernel is built for (1, 2, 4 clients x clients per workgroup; the matrix
  is the same bits at each), one ``screen_select`` launch (f = the largest the K allows, keep K - f), and
  the ``robust_aggregate`` launch behind them with and without the kept mask;
* ``round``: the whole ``ClientGroup(backend="hip", k=8)`` round on the income CSV's 8000 training
  rows (fp32) with ``screen="multi_krum"`` (f = 2, the unweighted mean of the kept clients) against
  ``aggregator="median"`` and ``aggregator="mean"`` without a screen.

Each interval carries the eager launch + event marker cost.

    python tools/screen_trace.py [--rounds 200] [--passes 2]
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


def _kernel_case(m, rounds, K):
    from fedmi.fl.engine import _STATE_DTYPE
    from fedmi.models.mlp import image_layout
    dev = torch.device("cuda")
    pimg = image_layout(DIMS)[2]
    stream = torch.cuda.Stream()
    tails = K * 5
    g = torch.Generator(device="cpu").manual_seed(K)
    base = torch.randn(pimg + tails, generator=g)
    bufs = [(base + 0.1 * torch.randn(pimg + tails, generator=g)).to(dev) for _ in range(K)]
    dst = [torch.empty_like(bufs[0])]
    tab = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=dev)
    dtab = torch.tensor([b.data_ptr() for b in dst], dtype=torch.int64, device=dev)
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"] = 1, 0
    state = torch.as_tensor(rec.view(np.uint8).copy()).to(dev)
    bits = (1 << K) - 1
    rt = np.zeros(4, np.uint32)
    rt[0], rt[1] = np.float32(1).view(np.uint32), np.float32(K).view(np.uint32)
    rt[2], rt[3] = bits & 0xFFFFFFFF, bits >> 32
    rtab = torch.as_tensor(rt.view(np.int32)).to(dev)
    dist = torch.zeros(K * K, device=dev)
    keep = torch.zeros(1, dtype=torch.int64, device=dev)
    hist = torch.zeros(1, dtype=torch.int64, device=dev)
    f = max(0, (K - 3) // 2)
    s = stream.cuda_stream
    torch.cuda.synchronize()
    # the launches name the buffers by address only (tab / dtab): the closures below hold the tensors, or
    # the allocator hands their memory to the next case's tables and state while this case still writes it
    alive = (bufs, dst)

    def do_dist(tile, alive=alive):
        m.screen_dist(DIMS, tab.data_ptr(), K, dist.data_ptr(), state.data_ptr(), rtab.data_ptr(), 1, s, tile)

    def do_select(alive=alive):
        m.screen_select(dist.data_ptr(), K, f, 0, keep.data_ptr(), hist.data_ptr(), state.data_ptr(), rtab.data_ptr(), 1, s)

    def do_robust(k, alive=alive):   # the unweighted mean of the kept clients (trimmed-mean kind, beta 0), one destination
        m.robust_aggregate(DIMS, 2, 0.0, tab.data_ptr(), K, dtab.data_ptr(), 1, state.data_ptr(), rtab.data_ptr(),
                           tails, 1, s, *k)

    do_dist(0)
    do_select()
    torch.cuda.synchronize()
    out = [({"case": "kernel", "what": f"screen_dist tile {t}", "K": K, "workgroups": ((K + t - 1) // t) * ((K + t - 1) // t + 1) // 2},
            lambda t=t: _time(lambda: do_dist(t), rounds, 20, stream)) for t in (1, 2, 4)]
    out.append(({"case": "kernel", "what": "screen_select", "K": K, "f": f}, lambda: _time(do_select, rounds, 20, stream)))
    out.append(({"case": "kernel", "what": "robust mean, kept mask", "K": K},
                lambda: _time(lambda: do_robust((keep.data_ptr(),)), rounds, 20, stream)))
    out.append(({"case": "kernel", "what": "robust mean, no mask", "K": K},
                lambda: _time(lambda: do_robust(()), rounds, 20, stream)))
    return out


def round_cases(rounds):
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    for what, kw in (("multi_krum f=2 + mean", dict(screen="multi_krum", screen_byzantine=2)),
                     ("median", dict(aggregator="median")), ("mean", dict())):
        def run(kw=kw):
            cfg = EngineConfig(max_rounds=rounds + 24, early_stop=False, graph_rounds=0, **kw)
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
        yield {"case": "round", "what": what, "K": 8, "rows": int(len(X)), "dtype": "fp32"}, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    from fedmi.ops import native
    m = native()
    cases = [c for K in (4, 8, 64) for c in _kernel_case(m, a.rounds, K)] + list(round_cases(a.rounds))
    for p in range(a.passes):
        for tag, fn in cases:
            print(json.dumps({**tag, "pass": p, "n": a.rounds, **_stats(fn())}), flush=True)


if __name__ == "__main__":
    main()

"""Cost of the DnC screening kernels (fl_dnc.hip) beside the multi-Krum ones on the same buffers.

The protocol of tools/screen_trace.py: eager launches with event markers, ``--rounds`` (200) timed launches
after a warm-up, every case run ``--passes`` (2) times with the cases alternating, one JSON line per case and
pass.  Over K = 4, 8, 64 buffers of the 14-50-200-2 image + K metric tails: one ``dnc_gram`` and one
``dnc_select`` launch at ``screen_iters`` 1 and 3 (every coordinate, f = K // 4), and ``screen_dist`` +
``screen_select`` (f = the largest the K allows) in the same run.  Each interval carries the eager launch +
event marker cost.

    python tools/dnc_trace.py [--rounds 200] [--passes 2] > profiles/dnc_trace.jsonl
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
    from fedmi.fl.aggregate import dnc_chunks, dnc_scratch_floats
    from fedmi.fl.engine import _STATE_DTYPE
    from fedmi.models.mlp import image_layout
    dev = torch.device("cuda")
    pimg = image_layout(DIMS)[2]
    stream = torch.cuda.Stream()
    tails = K * 5
    g = torch.Generator(device="cpu").manual_seed(K)
    base = torch.randn(pimg + tails, generator=g)
    bufs = [(base + 0.1 * torch.randn(pimg + tails, generator=g)).to(dev) for _ in range(K)]
    tab = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=dev)
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"] = 1, 0
    state = torch.as_tensor(rec.view(np.uint8).copy()).to(dev)
    bits = (1 << K) - 1
    rt = np.zeros(4, np.uint32)
    rt[0], rt[1] = np.float32(1).view(np.uint32), np.float32(K).view(np.uint32)
    rt[2], rt[3] = bits & 0xFFFFFFFF, bits >> 32
    rtab = torch.as_tensor(rt.view(np.int32)).to(dev)
    dist = torch.zeros(K * K, device=dev)
    scratch = torch.zeros(dnc_scratch_floats(pimg, 3, K), device=dev)
    keep = torch.zeros(1, dtype=torch.int64, device=dev)
    hist = torch.zeros(1, dtype=torch.int64, device=dev)
    f, fk = K // 4, max(0, (K - 3) // 2)
    s = stream.cuda_stream
    torch.cuda.synchronize()
    alive = (bufs,)   # the launches name the buffers by address only: the closures hold the tensors

    def do_gram(iters, alive=alive):
        m.dnc_gram(DIMS, tab.data_ptr(), K, f, f, iters, 0, 0, scratch.data_ptr(), state.data_ptr(), rtab.data_ptr(), 1, s)

    def do_dselect(iters, alive=alive):
        m.dnc_select(DIMS, K, f, f, iters, scratch.data_ptr(), keep.data_ptr(), hist.data_ptr(), state.data_ptr(),
                     rtab.data_ptr(), 1, s)

    def do_dist(alive=alive):
        m.screen_dist(DIMS, tab.data_ptr(), K, dist.data_ptr(), state.data_ptr(), rtab.data_ptr(), 1, s, 0)

    def do_select(alive=alive):
        m.screen_select(dist.data_ptr(), K, fk, 0, keep.data_ptr(), hist.data_ptr(), state.data_ptr(), rtab.data_ptr(), 1, s)

    out = []
    for iters in (1, 3):
        do_gram(iters)
        do_dselect(iters)
        torch.cuda.synchronize()
        tag = {"case": "kernel", "K": K, "iters": iters, "workgroups": dnc_chunks(pimg, K) * iters}
        out.append(({**tag, "what": "dnc_gram"}, lambda i=iters: _time(lambda: do_gram(i), rounds, 20, stream)))
        out.append(({**tag, "what": "dnc_select", "workgroups": 1}, lambda i=iters: _time(lambda: do_dselect(i), rounds, 20, stream)))
    do_dist()
    do_select()
    torch.cuda.synchronize()
    out.append(({"case": "kernel", "what": "screen_dist", "K": K}, lambda: _time(do_dist, rounds, 20, stream)))
    out.append(({"case": "kernel", "what": "screen_select", "K": K, "f": fk}, lambda: _time(do_select, rounds, 20, stream)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    from fedmi.ops import native
    m = native()
    cases = [c for K in (4, 8, 64) for c in _kernel_case(m, a.rounds, K)]
    for p in range(a.passes):
        for tag, fn in cases:
            print(json.dumps({**tag, "pass": p, "n": a.rounds, **_stats(fn())}), flush=True)


if __name__ == "__main__":
    main()

"""Cost of the attack launch (fl_attack.hip) beside the median launch on the same buffers.

The protocol of tools/geomed_trace.py: eager launches with event markers, ``--rounds`` (200) timed after a
warm-up, every case run ``--passes`` (2) times with the cases alternating, one JSON line per case and pass,
printed and appended to ``--out`` (profiles/attack_trace.jsonl):

* ``kernel``: the ``attack_apply`` launch of every kind, in place over K = 4, 8, 64 buffers of the
  14-50-200-2 image + K metric tails with two bad clients (K = 64: eight), without a weight table (the
  robust mode) and, the colluding kinds, with one (the weighted mean: one division per honest model), and
  beside it the one median launch (``robust_aggregate``) on the same buffers in the same session.  The
  buffers are rewritten to K honest clients before every case; the launch runs in place as a client
  group's does, so after the first repetition the bad clients' buffers hold the attack's vector: no launch
  branches on a value, an operation costs the same;
* ``round``: the whole ``ClientGroup(backend="hip", k=8)`` round on the income CSV's 8000 training rows
  (fp32) under ``aggregator="median"`` with ``attack="alie"`` (two bad clients) and with no attack.

Each interval carries the eager launch + event marker cost.

The ``bench_ab`` lines of profiles/attack_trace.jsonl are not written by this tool: they record the headline
``bench.py`` runs of this tree against the parent's (profiles/attack_bench_ab.log).

    python tools/attack_trace.py [--rounds 200] [--passes 2] [--out profiles/attack_trace.jsonl]
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
    from fedmi.fl.attack import ATTACKS
    from fedmi.fl.engine import _STATE_DTYPE
    from fedmi.models.mlp import dense_to_image, image_layout, param_count
    dev = torch.device("cuda")
    pimg = image_layout(DIMS)[2]
    stream = torch.cuda.Stream()
    tails = K * 5
    rng = np.random.default_rng(K)
    P = param_count(DIMS)
    c = rng.standard_normal(P).astype(np.float32)
    init = np.zeros((K, pimg + tails), np.float32)
    for k in range(K):   # honest clients around one model
        init[k, :pimg] = dense_to_image(c + np.float32(0.01) * rng.standard_normal(P).astype(np.float32), DIMS)
    init = torch.as_tensor(init).to(dev)
    x = torch.as_tensor(dense_to_image(c, DIMS)).to(dev)
    bufs = [torch.empty(pimg + tails, device=dev) for _ in range(K)]
    tab = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=dev)
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"] = 1, 0
    live = torch.as_tensor(rec.view(np.uint8).copy()).to(dev)
    bits = (1 << K) - 1
    rt = np.zeros(4, np.uint32)
    rt[0], rt[1] = np.float32(1).view(np.uint32), np.float32(K).view(np.uint32)
    rt[2], rt[3] = bits & 0xFFFFFFFF, bits >> 32
    rtab = torch.as_tensor(rt.view(np.int32)).to(dev)
    wtab = torch.full((1, K), 1.0 / K, dtype=torch.float32, device=dev)
    n_bad = 2 if K < 64 else 8
    bad = sum(1 << k for k in ((1, 3) if K == 4 else [1 + 3 * i for i in range(n_bad)]))
    torch.cuda.synchronize()

    def reset():
        for k, b in enumerate(bufs):
            b.copy_(init[k])
        torch.cuda.synchronize()

    def attack(kind, weighted):
        m.attack_apply(DIMS, ATTACKS.index(kind), 0.5, 0.25, 7, tab.data_ptr(), K, x.data_ptr(),
                       wtab.data_ptr() if weighted else 0, bad, live.data_ptr(), rtab.data_ptr(), 1, stream.cuda_stream)

    def median():
        m.robust_aggregate(DIMS, 1, 0.0, tab.data_ptr(), K, tab.data_ptr(), K, live.data_ptr(), rtab.data_ptr(), tails, 1,
                           stream.cuda_stream)

    def timed(fn):
        def run():
            reset()
            return _time(fn, rounds, 20, stream)
        return run

    out = [({"case": "kernel", "what": "median", "K": K, "launches": 1}, timed(median))]
    for kind in ("alie", "ipm", "sign_flip", "gauss"):
        for weighted in ((False, True) if kind in ("alie", "ipm") else (False,)):
            out.append(({"case": "kernel", "what": kind, "K": K, "bad": n_bad, "weighted": weighted, "launches": 1},
                        timed(lambda kind=kind, weighted=weighted: attack(kind, weighted))))
    return out


def kernel_cases(m, rounds):
    return [c for K in (4, 8, 64) for c in _kernel_case(m, rounds, K)]


def round_cases(rounds):
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    for attack in ("alie", "none"):
        def run(attack=attack):
            kw = dict(attack=attack, attack_clients=(1, 4)) if attack != "none" else {}
            cfg = EngineConfig(max_rounds=rounds + 24, early_stop=False, graph_rounds=0, aggregator="median", **kw)
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
        yield {"case": "round", "what": f"median, attack {attack}", "K": 8, "rows": int(len(X)), "dtype": "fp32"}, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attack_trace.jsonl"))
    a = ap.parse_args()
    from fedmi.ops import native
    m = native()
    cases = list(kernel_cases(m, a.rounds)) + list(round_cases(a.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for p in range(a.passes):
            for tag, fn in cases:
                line = json.dumps({**tag, "pass": p, "n": a.rounds, **_stats(fn())})
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()

"""Cost of the SCAFFOLD launches (fl_scaffold.hip) and of a client-group round with them.

The protocol of tools/robust_trace.py: eager launches with event markers, ``--rounds`` (200) timed after a warm-up,
every case run ``--passes`` (2) times with the cases alternating, one JSON line per case and pass:

* ``capture``: a SCAFFOLD client's own launches of a round at 14-50-200-2 on 8000 synthetic rows with 250 (R = 32)
  and 500 (R = 16) slab rows, through the native engine's trace (an event after every launch behind a gate): the
  ``scaffold`` interval beside the ``train`` and ``adam`` intervals of the same rounds (one local step: the Adam
  interval is the launch that reduces the same rows plus the correction row);
* ``fold``: one ``scaffold_fold`` launch over K = 4, 8, 64 deltas of P = 11352 floats, all K clients owned;
* ``round``: the whole ``ClientGroup(backend="hip", k=8)`` round on the income CSV's 8000 training rows (fp32) with
  ``scaffold`` on and off in the same session.

Each interval carries the eager launch + event marker cost.

    python tools/scaffold_trace.py [--rounds 200] [--passes 2] > profiles/scaffold_trace.jsonl
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

from tools.robust_trace import DIMS, _stats, _time  # noqa: E402  (the same event-pair timer and statistics)


def capture_cases(rounds):
    from fedmi.data.synthetic import make_income_like
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    X, y = make_income_like(16000, seed=1)
    for R in (32, 16):
        def run(R=R):
            cfg = EngineConfig(max_rounds=rounds + 16, early_stop=False, graph_rounds=0, scaffold=True, rows_per_block=R)
            g = ClientGroup(X, y, 2, cfg, backend="hip", shard_mode="contiguous", seed=0)
            e = g.clients[0]   # its own launches, as run_local issues them: train, capture, Adam, eval
            t = dict(e.engine.trace(0, rounds, g.stream.cuda_stream, None, close=True, gate_us=5000.0, warm=10))
            return {k: round(float(t[k]), 2) for k in ("scaffold", "adam", "train", "eval", "round")}
        yield {"case": "capture", "slab_rows": 8000 // R, "R": R, "rows": 8000, "dims": DIMS}, run


def fold_cases(m, rounds):
    from fedmi.fl.engine import _STATE_DTYPE
    from fedmi.models.mlp import param_count
    dev, P = torch.device("cuda"), param_count(DIMS)
    for K in (4, 8, 64):
        stream = torch.cuda.Stream()
        g = torch.Generator(device="cpu").manual_seed(K)
        deltas, ci, c = (torch.randn(K, P, generator=g).to(dev) * 1e-3 for _ in range(3))
        tabs = [torch.tensor([row.data_ptr() for row in t], dtype=torch.int64, device=dev) for t in (deltas, c, ci)]
        rec = np.zeros(1, dtype=_STATE_DTYPE)
        rec["live"], rec["cur_round"] = 1, 0
        state = torch.as_tensor(rec.view(np.uint8).copy()).to(dev)
        bits = (1 << K) - 1
        rt = np.zeros(4, np.uint32)
        rt[0], rt[1] = np.float32(1).view(np.uint32), np.float32(K).view(np.uint32)
        rt[2], rt[3] = bits & 0xFFFFFFFF, bits >> 32
        rtab = torch.as_tensor(rt.view(np.int32)).to(dev)
        torch.cuda.synchronize()

        def launch(K=K, tabs=tabs, state=state, rtab=rtab, stream=stream, keep=(deltas, ci, c)):
            m.scaffold_fold(P, tabs[0].data_ptr(), K, K, tabs[1].data_ptr(), K, tabs[2].data_ptr(), K, 0, state.data_ptr(),
                            rtab.data_ptr(), 1, stream.cuda_stream)
        yield ({"case": "fold", "K": K, "P": P, "launches": 1},
               lambda launch=launch, stream=stream: _stats(_time(launch, rounds, 20, stream)))


def round_cases(rounds):
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    ds = load_tabular(with_mean=True)
    X, y = ds.X_train, ds.y_train
    for on in (False, True):
        def run(on=on):
            # (both from one common model: the server step at lr 1 without momentum)
            cfg = EngineConfig(max_rounds=rounds + 24, early_stop=False, graph_rounds=0, scaffold=on, server_opt="sgd",
                               server_lr=1.0, server_momentum=0.0)
            g = ClientGroup(X, y, 8, cfg, backend="hip", shard_mode="iid", seed=0)
            state = {"r": 0}

            def one():
                g._round_hip(state["r"])
                state["r"] += 1
            us = _time(one, rounds, 16, g.stream)
            g.rounds = state["r"]
            g.sync_history()
            assert g.history()["rounds_run"] == rounds + 16
            return _stats(us)
        yield {"case": "round", "scaffold": on, "K": 8, "rows": int(len(X)), "dtype": "fp32"}, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=2)
    a = ap.parse_args()
    from fedmi.ops import native
    m = native()
    cases = list(capture_cases(a.rounds)) + list(fold_cases(m, a.rounds)) + list(round_cases(a.rounds))
    for p in range(a.passes):
        for tag, fn in cases:
            print(json.dumps({**tag, "pass": p, "n": a.rounds, **fn()}), flush=True)


if __name__ == "__main__":
    main()

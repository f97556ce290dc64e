"""Cost of the centered-clipping launches (fl_cclip.hip), of a client-group round around them, and what the
rule buys under the colluding attacks.

The protocol of tools/robust_trace.py (helpers of tools/geomed_trace.py): eager launches with event markers,
``--rounds`` (200) timed after a warm-up, every case run ``--passes`` (2) times with the cases alternating, one
JSON line per case and pass, printed and appended to ``--out`` (profiles/cclip_trace.jsonl):

* ``kernel``: the ``cclip_aggregate`` sequence (T + 1 launches) at T = 1 and 3, in place over K = 4, 8, 64
  buffers of the 14-50-200-2 image + K metric tails around a centre at about one ``tau`` from the clients, and
  beside it, on the same buffers in the same session, the ``geomed_aggregate`` sequence at the same T and the
  one median launch: the yardsticks.  The buffers are rewritten before every case; in place, the K images are
  equal after the first repetition (no launch branches on a value: an operation costs the same);
* ``round``: the whole ``ClientGroup(backend="hip", k=8)`` round on the income CSV's 8000 training rows (fp32)
  with ``aggregator="cclip"``, ``"geomed"``, ``"median"`` and ``"mean"``;
* ``attack`` (untimed; ``--attack-rounds``, 30): seven clients, clients 1 and 4 Byzantine, ``attack`` "alie"
  (z = 1.5) / "ipm" (eps = 0.5) against ``median``, ``geomed`` and ``cclip`` at ``cclip_tau`` 0.03 .. 3: the
  global model's held-out cross-entropy after the last round (``set_heldout``).

    python tools/cclip_trace.py [--rounds 200] [--passes 2] [--out profiles/cclip_trace.jsonl]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from geomed_trace import DIMS, NU, _stats, _time  # noqa: E402

TAU = 1.0


def _kernel_case(m, rounds, K):
    from fedmi.fl.aggregate import cclip_scratch_floats, geomed_scratch_floats
    from fedmi.fl.engine import _STATE_DTYPE
    from fedmi.models.mlp import dense_to_image, image_layout, param_count
    dev = torch.device("cuda")
    pimg, P = image_layout(DIMS)[2], param_count(DIMS)
    stream = torch.cuda.Stream()
    tails = K * 5
    rng = np.random.default_rng(K)
    c = rng.standard_normal(P).astype(np.float32)
    x = torch.as_tensor(dense_to_image(c, DIMS)).to(dev)
    init = np.zeros((K, pimg + tails), np.float32)
    for k in range(K):   # clients at about 1.07 tau from the centre: clipped and combined, all K of them
        init[k, :pimg] = dense_to_image(c + np.float32(0.01) * rng.standard_normal(P).astype(np.float32), DIMS)
    init = torch.as_tensor(init).to(dev)
    bufs = [torch.empty(pimg + tails, device=dev) for _ in range(K)]
    addrs = [b.data_ptr() for b in bufs]
    tab = torch.tensor(addrs, dtype=torch.int64, device=dev)
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"] = 1, 0
    live = torch.as_tensor(rec.view(np.uint8).copy()).to(dev)
    bits = (1 << K) - 1
    rt = np.zeros(4, np.uint32)
    rt[0], rt[1] = np.float32(1).view(np.uint32), np.float32(K).view(np.uint32)
    rt[2], rt[3] = bits & 0xFFFFFFFF, bits >> 32
    rtab = torch.as_tensor(rt.view(np.int32)).to(dev)
    scratch = torch.zeros(max(cclip_scratch_floats(pimg, 3), geomed_scratch_floats(pimg, 3)), device=dev)
    torch.cuda.synchronize()

    def reset():
        for k, b in enumerate(bufs):
            b.copy_(init[k])
        torch.cuda.synchronize()

    def cclip(T):
        m.cclip_aggregate(DIMS, T, TAU, tab.data_ptr(), K, x.data_ptr(), tab.data_ptr(), K, live.data_ptr(),
                          rtab.data_ptr(), tails, 1, scratch.data_ptr(), stream.cuda_stream, dst_addrs=addrs)

    def geomed(T):
        m.geomed_aggregate(DIMS, T, NU, tab.data_ptr(), K, tab.data_ptr(), K, live.data_ptr(), rtab.data_ptr(), tails, 1,
                           scratch.data_ptr(), stream.cuda_stream)

    def median():
        m.robust_aggregate(DIMS, 1, 0.0, tab.data_ptr(), K, tab.data_ptr(), K, live.data_ptr(), rtab.data_ptr(), tails, 1,
                           stream.cuda_stream)

    def timed(fn):
        def run():
            reset()
            return _time(fn, rounds, 20, stream)
        return run

    out = [({"case": "kernel", "what": "median", "K": K, "launches": 1}, timed(median))]
    for T in (1, 3):
        out.append(({"case": "kernel", "what": "cclip", "K": K, "T": T, "launches": T + 1}, timed(lambda T=T: cclip(T))))
        out.append(({"case": "kernel", "what": "geomed", "K": K, "T": T, "launches": T + 1}, timed(lambda T=T: geomed(T))))
    return out


def round_cases(rounds, ds):
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    for agg in ("cclip", "geomed", "median", "mean"):
        def run(agg=agg):
            cfg = EngineConfig(max_rounds=rounds + 24, early_stop=False, graph_rounds=0, aggregator=agg)
            g = ClientGroup(ds.X_train, ds.y_train, 8, cfg, backend="hip", shard_mode="iid", seed=0)
            state = {"r": 0}

            def one():
                g._round_hip(state["r"])
                state["r"] += 1
            us = _time(one, rounds, 16, g.stream)
            g.rounds = state["r"]
            g.sync_history()
            assert g.history()["rounds_run"] == rounds + 16
            return us
        yield {"case": "round", "what": agg, "K": 8, "rows": int(len(ds.X_train)), "dtype": "fp32"}, run


def attack_lines(rounds, ds):
    from fedmi.fl.engine import EngineConfig
    from fedmi.fl.simulate import ClientGroup
    rules = [("median", {}), ("geomed", {})] + [("cclip", {"cclip_tau": t}) for t in (0.03, 0.1, 0.3, 1.0, 3.0)]
    attacks = {"none": {}, "alie": dict(attack="alie", attack_clients=(1, 4), attack_z=1.5),
               "ipm": dict(attack="ipm", attack_clients=(1, 4), attack_scale=0.5)}
    for name, akw in attacks.items():
        for agg, kw in rules:
            cfg = EngineConfig(max_rounds=rounds, early_stop=False, graph_rounds=0, aggregator=agg, **kw, **akw)
            g = ClientGroup(ds.X_train, ds.y_train, 7, cfg, backend="hip", shard_mode="iid", seed=0,
                            heldout=(ds.X_test, ds.y_test))
            g.run(rounds)
            loss = float(g.history()["heldout_loss"][rounds - 1])
            yield {"case": "attack", "attack": name, "aggregator": agg, **kw, "clients": 7, "bad": [1, 4], "rounds": rounds,
                   "heldout_loss": round(loss, 5) if np.isfinite(loss) else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--attack-rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cclip_trace.jsonl"))
    a = ap.parse_args()
    from fedmi.data.tabular import load_tabular
    from fedmi.ops import native
    m = native()
    ds = load_tabular(with_mean=True)
    cases = [c for K in (4, 8, 64) for c in _kernel_case(m, a.rounds, K)] + list(round_cases(a.rounds, ds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for p in range(a.passes):
            for tag, fn in cases:
                emit({**tag, "pass": p, "n": a.rounds, **_stats(fn())})
        for rec in attack_lines(a.attack_rounds, ds):
            emit(rec)


if __name__ == "__main__":
    main()

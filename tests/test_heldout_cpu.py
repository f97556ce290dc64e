"""Held-out scoring of the global model and the inference API on the CPU: the torch engine's rows against
its own ``confusion`` and a float64 loss, the refusals, state mismatches on load, a checkpoint round trip,
``rounds_to_target`` with and without a held-out set, and the [C] entry point's flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, TorchRoundEngine, heldout_metrics
from fedmi.fl.simulate import ClientGroup, rounds_to_target
from fedmi.models.mlp import init_flat

from .reference_oracle import float64_logits, make_multiclass

DIMS = [5, 7, 3]


def _data(n, seed, dims=DIMS):
    X, y = make_multiclass(n, dims[0], dims[-1], seed)
    return np.ascontiguousarray(X, np.float32), np.asarray(y).astype(np.int64)


def _engine(dims=DIMS, **kw):
    X, y = _data(150, 3, dims)
    kw.setdefault("max_rounds", 12)
    kw.setdefault("early_stop", False)
    return TorchRoundEngine(X, y, dims[-1], EngineConfig(hidden=tuple(dims[1:-1]), **kw), None, init_flat(dims, 1))


def _ce64(flat, dims, X, y):
    z = torch.as_tensor(np.asarray(float64_logits(flat, dims, X), np.float64))
    return float((torch.logsumexp(z, 1) - z.gather(1, torch.as_tensor(y).view(-1, 1)).squeeze(1)).mean())


# ---- rows ----
@pytest.mark.parametrize("dims", [[14, 50, 200, 2], [5, 7, 3], [6, 9, 4, 3]])
@pytest.mark.parametrize("n_val", [1, 17, 100])
def test_torch_rows_are_its_own_confusion_and_a_float64_loss(dims, n_val):
    Xv, yv = _data(n_val, 11, dims)
    a, b = _engine(dims), _engine(dims)
    a.set_heldout(Xv, yv, keep_best=True)
    a.run(5)
    h = a.history()
    flats = []
    for r in range(5):
        b.run(1)
        flats.append(b.global_flat())
        np.testing.assert_array_equal(h["heldout_cm"][r], b.confusion(Xv, yv, flat=flats[-1]))
        np.testing.assert_allclose(h["heldout_loss"][r], _ce64(flats[-1], dims, Xv, yv), rtol=1e-4)
    # nothing else moved
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    for k in ("global", "per_rank", "loss"):
        np.testing.assert_array_equal(h[k], b.history()[k])
    assert set(h) - set(b.history()) == {"heldout_cm", "heldout_loss", "heldout_loss_sum", "heldout_best_round"}
    assert h["heldout_cm"].dtype == np.int64 and h["heldout_loss"].dtype == np.float64
    best = int(np.argmin(h["heldout_loss_sum"]))
    assert h["heldout_best_round"] == best
    np.testing.assert_array_equal(a.best_flat(), flats[best])
    m = heldout_metrics(h)
    assert m.shape == (5, 4)
    np.testing.assert_allclose(m[:, 0], h["heldout_cm"].trace(axis1=1, axis2=2) / n_val)
    with pytest.raises(KeyError, match="set_heldout"):
        heldout_metrics(b.history())


def test_early_stop_cuts_the_rows_and_nan_never_wins():
    X, y = _data(400, 3)
    Xv, yv = _data(33, 11)
    e = TorchRoundEngine(X, y, 3, EngineConfig(hidden=(7,), max_rounds=200, patience=2, tolerance=0.05), None,
                         init_flat(DIMS, 1))
    e.set_heldout(Xv, yv)
    e.run(200)
    h = e.history()
    assert 0 < h["rounds_run"] < 200 and len(h["heldout_cm"]) == len(h["heldout_loss"]) == h["rounds_run"]
    assert (e.hist.ho_cm[h["rounds_run"]:] == 0).all()

    def tamper(r, bufs):
        if r >= 2:
            for b in bufs:
                b[:e.P] = float("nan")

    g = ClientGroup(X, y, 3, EngineConfig(hidden=(7,), max_rounds=6, early_stop=False), backend="torch",
                    shard_mode="iid", tamper=tamper, heldout=(Xv, yv), keep_best=True)
    g.run(5)
    hg = g.history()
    assert np.isnan(hg["heldout_loss"][2:]).all() and np.isfinite(hg["heldout_loss"][:2]).all()
    assert 0 <= hg["heldout_best_round"] <= 1 and np.isfinite(g.best_flat()).all()
    assert all(not c.heldout for c in g.clients[1:]) and g.clients[0].heldout   # only the lead holds the set


# ---- inference ----
@pytest.mark.parametrize("n", [0, 1, 17])
def test_torch_predict(n):
    e = _engine()
    e.run(2)
    X, y = _data(max(n, 1), 21)
    X, y = X[:n], y[:n]
    p = e.predict_proba(X)
    assert p.shape == (n, 3) and p.dtype == np.float32
    pred = e.predict(X, which="local")
    assert pred.shape == (n,) and pred.dtype == np.int64
    if n:
        z = np.asarray(float64_logits(e.global_flat(), DIMS, X))
        np.testing.assert_allclose(p, torch.softmax(torch.as_tensor(z), 1).numpy(), atol=1e-6)
        assert np.abs(p.sum(1) - 1).max() <= 1e-6
    z0 = _engine()
    z0.set_global_flat(np.zeros(z0.P, np.float32))
    np.testing.assert_array_equal(z0.predict(np.ones((4, 5), np.float32)), np.zeros(4, np.int64))   # first maximum
    np.testing.assert_array_equal(z0.predict_proba(np.ones((4, 5), np.float32)), np.full((4, 3), np.float32(1) / 3))
    with pytest.raises(ValueError, match="which"):
        e.predict(X, which="server")


# ---- refusals ----
def test_refusals():
    X, y = _data(64, 3)
    e = _engine()
    for bad_X, bad_y, msg in ((X[:, :4], y, "held-out X"), (X, y[:-1], "held-out y"), (X, y + 2, "labels"),
                              (X, -y - 1, "labels"), (X, y.astype(np.float32), "integers"), (X[:0], y[:0], "rows")):
        with pytest.raises(ValueError, match=msg):
            e.set_heldout(bad_X, bad_y)
    assert not e.heldout and "heldout_cm" not in e.history() and "heldout" not in e.portable_state()
    with pytest.raises(RuntimeError, match="keep_best"):
        e.best_flat()
    e.set_heldout(X, y, keep_best=True)
    with pytest.raises(RuntimeError, match="no round has won"):
        e.best_flat()
    assert "heldout" not in EngineConfig().to_dict() and not hasattr(EngineConfig(), "heldout")   # data, not config
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    grp = FedTrialGroup(X, y, 3, [FedTrial((7,), 0.01, 1)], None, EngineConfig(max_rounds=2), backend="torch")
    with pytest.raises(ValueError, match="fed_sweep"):
        grp.set_heldout(X, y)
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="WideClient"):
        WideClient.set_heldout(object(), X, y)


# ---- state ----
def test_state_mismatch_on_load_raises_both_ways():
    Xv, yv = _data(17, 11)
    a = _engine()
    a.set_heldout(Xv, yv)
    a.run(2)
    b = _engine()
    b.run(2)
    with pytest.raises(ValueError, match="held-out"):
        _engine().load_portable_state(a.portable_state())
    c = _engine()
    c.set_heldout(Xv, yv)
    with pytest.raises(ValueError, match="held-out"):
        c.load_portable_state(b.portable_state())
    c.load_portable_state(a.portable_state())
    np.testing.assert_array_equal(c.history()["heldout_cm"], a.history()["heldout_cm"])


def test_checkpoint_round_trip_continues_rows_and_best(tmp_path):
    from fedmi.ckpt.checkpoint import resume, save_checkpoint
    Xv, yv = _data(33, 11)

    def mk(heldout=True):
        e = _engine()
        if heldout:
            e.set_heldout(Xv, yv, keep_best=True)
        return e

    full = mk()
    full.run(8)
    a = mk()
    a.run(3)
    save_checkpoint(str(tmp_path / "c"), a)
    meta = json.load(open(tmp_path / "c" / "meta.json"))
    assert not any(k.startswith("heldout") for k in meta["history"]) and "heldout" not in json.dumps(meta["config"])
    b = mk()
    assert resume(str(tmp_path / "c"), b) == 3
    np.testing.assert_array_equal(b.history()["heldout_cm"], a.history()["heldout_cm"])
    np.testing.assert_array_equal(b.best_flat(), a.best_flat())
    b.run(5)
    hf, hb = full.history(), b.history()
    np.testing.assert_array_equal(hf["heldout_cm"], hb["heldout_cm"])
    np.testing.assert_array_equal(hf["heldout_loss_sum"], hb["heldout_loss_sum"])
    assert hf["heldout_best_round"] == hb["heldout_best_round"]
    np.testing.assert_array_equal(full.best_flat(), b.best_flat())
    with pytest.raises(ValueError, match="held-out"):
        resume(str(tmp_path / "c"), mk(heldout=False))
    p = mk(heldout=False)
    p.run(2)
    save_checkpoint(str(tmp_path / "p"), p)
    with pytest.raises(ValueError, match="held-out"):
        resume(str(tmp_path / "p"), mk())
    assert resume(str(tmp_path / "p"), mk(heldout=False)) == 2


# ---- rounds_to_target ----
def test_rounds_to_target_with_and_without_heldout():
    X, y = _data(300, 3)
    Xv, yv = _data(60, 11)
    cfg = EngineConfig(hidden=(7,), max_rounds=10, early_stop=False, lr=0.02)
    plain = rounds_to_target(X, y, 2, cfg, backend="torch", targets=(0.4, 2.0))
    assert set(plain) == {"0.40", "2.00", "early_stop_round", "final_acc", "rounds_run"}   # today's result
    ho = rounds_to_target(X, y, 2, cfg, backend="torch", targets=(0.4, 2.0), heldout=(Xv, yv))
    assert ho["metric"] == "heldout_accuracy" and ho["2.00"] is None and ho["rounds_run"] == plain["rounds_run"] == 10
    g = ClientGroup(X, y, 2, cfg, backend="torch", heldout=(Xv, yv))
    g.run(10)
    acc = heldout_metrics(g.history())[:, 0]
    assert ho["final_acc"] == float(acc[-1])
    hit = np.flatnonzero(acc >= 0.4)
    assert ho["0.40"] == (int(hit[0]) + 1 if len(hit) else None)
    np.testing.assert_array_equal(acc * 60, g.history()["heldout_cm"].trace(axis1=1, axis2=2))
    assert plain["final_acc"] == float(g.history()["global"][-1, 0])   # ... and the local-shard mean without it


# ---- the [C] entry point ----
def _run_c(args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(root, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py"),
                           "--device", "cpu", "--backend", "gloo", "--engine", "torch", *args],
                          cwd=root, capture_output=True, text=True, timeout=300, env=env)


def test_entrypoint_flags(tmp_path):
    base = ["--rounds", "3", "--no-early-stop"]
    plain = _run_c([*base, "--jsonl", str(tmp_path / "plain.jsonl")])
    assert plain.returncode == 0, plain.stderr[-2000:]
    r = _run_c([*base, "--heldout", "--keep-best", "--predict-out", str(tmp_path / "p.npy"), "--jsonl",
                str(tmp_path / "ho.jsonl")])
    assert r.returncode == 0, r.stderr[-2000:]
    # the console: today's lines, then one line naming the best held-out round
    lines = r.stdout.splitlines()
    assert lines[:-1] == plain.stdout.splitlines() and lines[-1].startswith("Best held-out round: ")
    rows = {k: [json.loads(l) for l in open(tmp_path / f"{k}.jsonl")] for k in ("plain", "ho")}
    keys = {"heldout_accuracy", "heldout_precision", "heldout_recall", "heldout_f1", "heldout_loss"}
    assert len(rows["ho"]) == 3 and all(keys <= set(row) for row in rows["ho"])
    assert not any(k.startswith("heldout") for row in rows["plain"] for k in row)
    assert [row["loss"] for row in rows["ho"]] == [row["loss"] for row in rows["plain"]]
    p = np.load(tmp_path / "p.npy")
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 2 and np.abs(p.sum(1) - 1).max() <= 1e-6
    best = int(lines[-1].split("round: ")[1].split()[0])
    assert rows["ho"][best - 1]["heldout_loss"] == min(row["heldout_loss"] for row in rows["ho"])
    r = _run_c([*base, "--quiet", "--clients", "2", "--heldout", "--predict-out", str(tmp_path / "q.npy")])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "2 simulated clients (torch): 3 rounds" in r.stdout and "Best held-out round: " in r.stdout
    assert np.load(tmp_path / "q.npy").shape == p.shape
    r = _run_c([*base, "--wide", "--heldout"])
    assert r.returncode != 0 and "--heldout / --keep-best / --predict-out is not supported with --wide" in r.stderr
    r = _run_c([*base, "--keep-best"])
    assert r.returncode != 0 and "--keep-best needs --heldout" in r.stderr

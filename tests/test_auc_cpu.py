"""Held-out ROC AUC off the GPU: the numpy specification ``auc_u2_model`` against the O(n^2) pair count
of its definition, the torch engine's ``heldout_auc_u2`` rows against the model on its own
``predict_proba``, their resume, and the entry point's ``--heldout-auc`` flag."""
import importlib.util
import os

import numpy as np
import pytest

from fedmi.fl.engine import EngineConfig, TorchRoundEngine, heldout_auc_score
from fedmi.fl.metrics import auc_from_u2, auc_u2_model
from fedmi.models.mlp import init_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [14, 50, 200, 2]


def pair_count(s, pos):
    """The definition: NaN becomes the value just above 1.0, then every (positive, negative) pair."""
    s = np.where(np.isnan(s), np.float32(1.0) + np.float32(2.0 ** -23), s).astype(np.float32)
    si, sj = s[pos][:, None], s[~pos][None, :]
    return int((2 * (sj < si).astype(np.int64) + (sj == si).astype(np.int64)).sum())


@pytest.mark.parametrize("scores", ["three_values", "all_equal", "distinct"])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 300])
def test_model_is_the_pair_count(n, scores):
    rng = np.random.default_rng(n)
    s = {"three_values": rng.choice(np.float32([0.25, 0.5, 0.75]), n), "all_equal": np.full(n, 0.5, np.float32),
         "distinct": rng.permutation(n).astype(np.float32) / np.float32(n + 1)}[scores]
    pos = rng.random(n) < 0.5
    if n >= 7:   # a NaN row and a row at exactly 1.0, one of each label
        s[0], s[1], s[2], s[3] = np.nan, 1.0, np.nan, 1.0
        pos[0], pos[1], pos[2], pos[3] = True, False, False, True
    assert auc_u2_model(s, pos) == pair_count(s, pos)
    for empty in (np.zeros(n, bool), np.ones(n, bool)):   # P == 0, N == 0
        assert auc_u2_model(s, empty) == 0
        assert np.isnan(auc_from_u2(0, empty.sum(), n - empty.sum()))


def _engine(auc=True, heldout=True, seed=3):
    rng = np.random.default_rng(seed)
    X, y = rng.standard_normal((256, 14)).astype(np.float32), rng.integers(0, 2, 256)
    Xv, yv = rng.standard_normal((77, 14)).astype(np.float32), rng.integers(0, 2, 77)
    e = TorchRoundEngine(X, y, 2, EngineConfig(max_rounds=8, early_stop=False), None, init_flat(DIMS, 1))
    if heldout:
        e.set_heldout(Xv, yv, auc=auc)
    return e, Xv, yv


def test_torch_engine_rows_and_resume():
    e, Xv, yv = _engine()
    want = []
    for _ in range(3):
        e.run(1)
        p = e.predict_proba(Xv, which="global")
        want.append([auc_u2_model(p[:, c], yv == c) for c in range(2)])
    h = e.history()
    assert h["heldout_auc_u2"].dtype == np.int64 and h["heldout_auc_u2"].tolist() == want
    P = np.bincount(yv, minlength=2)
    assert np.array_equal(h["heldout_auc"], h["heldout_auc_u2"] / (2.0 * P * (77 - P)))
    assert np.array_equal(heldout_auc_score(h), h["heldout_auc"][:, 1])
    assert "heldout_auc_u2" not in _engine(auc=False)[0].history()
    st = e.portable_state()
    e2, _, _ = _engine()
    e2.load_portable_state(st)
    e.run(1), e2.run(1)
    assert e2.history()["heldout_auc_u2"].tolist() == e.history()["heldout_auc_u2"].tolist() and len(want) == 3
    for other in (_engine(auc=False)[0], _engine(heldout=False)[0]):
        with pytest.raises(ValueError, match="disagree on held-out"):
            other.load_portable_state(st)
    with pytest.raises(ValueError, match="disagree on held-out AUC"):
        e2.load_portable_state(_engine(auc=False)[0].portable_state())


def test_flag_implies_heldout():
    spec = importlib.util.spec_from_file_location(
        "fl_c_entry", os.path.join(ROOT, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["--heldout-auc"])
    assert a.heldout_auc and a.heldout
    a = mod.parse_args(["--heldout"])
    assert a.heldout and not a.heldout_auc

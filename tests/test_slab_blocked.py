"""The blocked fp16 gradient-slab row (fl_layout.h FlSlabBlk) against the dense row.

The reference 14-50-200-2 MLP at R = 32 with ``grad_slab="fp16"``: an engine constructed with the switches
unset keeps its slab rows blocked (``layout["slab_blocked"]`` True: the specialised bf16 train kernel stores
each wgrad tile as one aligned 8-byte store per lane, the specialised Adam kernel reads the same order),
engines under ``FEDMI_SHAPE_SPEC=0`` (generic kernels) and ``FEDMI_ADAM_SPEC=0`` (specialised train kernel,
generic Adam kernel) keep dense rows.  Only the place of a partial in its row differs, so everything must
agree BITWISE (``torch.equal`` / ``np.array_equal``, no tolerance): the partials of one train launch
gathered into dense order, and after 3 rounds the local and global weights, both Adam moments, the packed
bf16 image and the history rows.  A slab filled with fp16 NaN patterns before a round leaves the
saturation flag at 0 and the weights those of the dense run: the train kernel writes every position of
the row, pads included, and no pad reaches a parameter.  Shards: 5 rows (one partial workgroup), 33 (two
slab rows, the second of one row) and 300."""
import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass

pytestmark = pytest.mark.gpu

DIMS = (14, 50, 200, 2)
ROWS = [5, 33, 300]
ROUNDS = 3
# switches of the three engines: the blocked one, generic kernels, generic Adam kernel
VARIANTS = {"blocked": {}, "shape_off": {"FEDMI_SHAPE_SPEC": "0"}, "adam_off": {"FEDMI_ADAM_SPEC": "0"}}
_DATA = {}


def _engine(monkeypatch, variant, rows, **kw):
    for k in ("FEDMI_SHAPE_SPEC", "FEDMI_ADAM_SPEC", "FEDMI_SLAB_BLOCKED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    if rows not in _DATA:
        _DATA[rows] = make_multiclass(rows, DIMS[0], DIMS[-1], DATA_SEED)
    X, y = _DATA[rows]
    cfg = EngineConfig(hidden=DIMS[1:-1], max_rounds=ROUNDS + 2, rows_per_block=32, graph_rounds=0, dtype="bf16",
                       grad_slab="fp16", early_stop=False, **kw)
    eng = HipRoundEngine(X, y, DIMS[-1], cfg, None, init_flat(list(DIMS), INIT_SEED))
    assert eng.R == 32 and eng.slab_f16
    assert eng.engine.layout()["slab_blocked"] is (variant == "blocked"), (variant, eng.engine.layout())
    return eng


def _state(eng):
    st = eng.portable_state()
    h = eng.history()
    s = eng.stream.cuda_stream
    return {"local": st["local"], "global": st["global"], "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"],
            "local_image": eng.local.cpu().numpy(), "m_image": eng.mom.cpu().numpy(), "v_image": eng.vel.cpu().numpy(),
            "packed_local": np.frombuffer(eng.engine.packed_local(s), np.uint8),
            "packed_global": np.frombuffer(eng.engine.packed_global(s), np.uint8),
            "loss": h["loss"], "hist_global": h["global"], "hist_rank": h["per_rank"],
            "rounds_run": np.asarray(h["rounds_run"]), "sat": np.asarray(int(eng.sat.item()))}


def _assert_equal(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


@pytest.mark.parametrize("rows", ROWS)
def test_blocked_rows_equal_dense_rows_bitwise(monkeypatch, rows):
    part, out = {}, {}
    for v in VARIANTS:
        eng = _engine(monkeypatch, v, rows)
        eng.run(1)  # one train launch (and its Adam launch, which only reads the slab)
        eng.stream.synchronize()
        part[v] = eng.slab_partials()
        assert part[v].shape == ((rows + 31) // 32, eng.P) and part[v].dtype == torch.float16
        eng.run(ROUNDS - 1)
        out[v] = _state(eng)
    assert bool(torch.isfinite(part["blocked"].float()).all()) and bool((part["blocked"] != 0).any())
    for v in ("shape_off", "adam_off"):
        assert torch.equal(part["blocked"], part[v]), v
        _assert_equal(out["blocked"], out[v], v)
    assert int(out["blocked"]["rounds_run"]) == ROUNDS and int(out["blocked"]["sat"]) == 0
    assert np.all(np.isfinite(out["blocked"]["global"])) and np.all(np.isfinite(out["blocked"]["loss"]))


@pytest.mark.parametrize("rows", ROWS)
def test_nan_filled_slab_is_overwritten_and_no_pad_leaks(monkeypatch, rows):
    out = {}
    for v in ("blocked", "adam_off"):
        eng = _engine(monkeypatch, v, rows)
        eng.run(1)
        eng.stream.synchronize()
        if v == "blocked":  # every half of every row (gradients, pads, row tails, loss slots): an fp16 NaN
            eng.slab.view(torch.int16).fill_(0x7E00)
            torch.cuda.synchronize()
        eng.run(1)
        out[v] = _state(eng)
    assert int(out["blocked"]["sat"]) == 0
    _assert_equal(out["blocked"], out["adam_off"], "nan-filled")
    assert np.all(np.isfinite(out["blocked"]["global"])) and np.all(np.isfinite(out["blocked"]["loss"]))


def test_blocked_rows_with_weight_decay(monkeypatch):
    out = {}
    for v in VARIANTS:
        eng = _engine(monkeypatch, v, 33, weight_decay=0.01)
        eng.run(ROUNDS)
        out[v] = _state(eng)
    for v in ("shape_off", "adam_off"):
        _assert_equal(out["blocked"], out[v], v)
    assert int(out["blocked"]["rounds_run"]) == ROUNDS

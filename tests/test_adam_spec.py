"""The shape-specialised Adam kernel (fl_adam_spec.hip: reference 14-50-200-2 MLP, R = 32, one client)
against the generic one.

Two engines on the same data and seed, the train kernels specialised in both: one constructed with
``FEDMI_ADAM_SPEC`` unset (``layout["adam_spec"]`` True) and one under ``FEDMI_ADAM_SPEC=0`` (the
generic no-exchange kernel), must agree BITWISE -- ``np.array_equal``, no tolerance -- in the global
weights, both Adam moments and the loss / global / per-rank histories: the specialised kernel is the
generic kernel's body with constant descriptors, so it sums the same slab rows in the same order and
applies the same update.  Shards: 32 rows (one slab row), 33, 95 (a partial last block), 4100 (129 slab
rows: the second 16-byte load of a wave) and 8200 (257 slab rows: the second pass of the load loop)."""
import numpy as np
import pytest

from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass

pytestmark = pytest.mark.gpu

DIMS = (14, 50, 200, 2)
ROUNDS = 6
NEAR_MISS = [(14, 50, 200, 3), (15, 50, 200, 2), (14, 50, 208, 2), (14, 48, 200, 2)]
# engine variants: MFMA operand type and gradient-slab format (the three instantiations)
ENGINES = {
    "bf16_f16slab": dict(dtype="bf16", grad_slab="fp16"),
    "bf16_f32slab": dict(dtype="bf16", grad_slab="fp32"),
    "fp32": dict(dtype="fp32"),
}
EXTRA = {
    "weight_decay": dict(early_stop=False, weight_decay=0.01),
    # every metric within 1.0 of the previous round's: the patience of 3 runs out inside the run, and
    # with a counter that low every block of the Adam kernel folds the round state
    "early_stop": dict(early_stop=True, patience=3, tolerance=1.0),
}
_DATA = {}


def _data(rows, F, C):
    if (rows, F, C) not in _DATA:
        _DATA[(rows, F, C)] = make_multiclass(rows, F, C, DATA_SEED)
    return _DATA[(rows, F, C)]


def _engine(monkeypatch, adam_spec, dims, rows, kw):
    monkeypatch.delenv("FEDMI_SHAPE_SPEC", raising=False)
    if adam_spec:
        monkeypatch.delenv("FEDMI_ADAM_SPEC", raising=False)
    else:
        monkeypatch.setenv("FEDMI_ADAM_SPEC", "0")
    X, y = _data(rows, dims[0], dims[-1])
    kw = dict(dict(rows_per_block=32, graph_rounds=0), **kw)
    cfg = EngineConfig(hidden=tuple(dims[1:-1]), max_rounds=ROUNDS + 2, **kw)
    return HipRoundEngine(X, y, dims[-1], cfg, None, init_flat(list(dims), INIT_SEED))


def _outputs(eng):
    eng.run(ROUNDS)
    st = eng.portable_state()
    h = eng.history()
    return {"weights": eng.global_flat(), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"],
            "loss": h["loss"], "global": h["global"], "per_rank": h["per_rank"],
            "stop_round": np.asarray(h["stop_round"]), "rounds_run": np.asarray(h["rounds_run"])}


def _pair(monkeypatch, rows, kw):
    out = {}
    for spec in (True, False):
        eng = _engine(monkeypatch, spec, DIMS, rows, kw)
        assert eng.R == 32
        assert eng.layout["shape_spec"] is True, eng.layout
        assert eng.layout["adam_spec"] is spec, eng.layout
        out[spec] = _outputs(eng)
    for k in out[True]:
        assert np.array_equal(out[True][k], out[False][k]), (k, out[True][k], out[False][k])
    assert np.all(np.isfinite(out[True]["weights"])) and np.all(np.isfinite(out[True]["loss"]))
    return out[True]


@pytest.mark.parametrize("rows", [32, 33, 95, 4100, 8200])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_specialised_adam_is_bitwise_the_generic_adam(monkeypatch, engine, rows):
    out = _pair(monkeypatch, rows, dict(ENGINES[engine], early_stop=False))
    assert int(out["rounds_run"]) == ROUNDS


@pytest.mark.parametrize("case", list(EXTRA))
@pytest.mark.parametrize("engine", list(ENGINES))
def test_specialised_adam_weight_decay_and_early_stop(monkeypatch, engine, case):
    out = _pair(monkeypatch, 95, dict(ENGINES[engine], **EXTRA[case]))
    if case == "early_stop":
        assert 0 < int(out["stop_round"]) < ROUNDS, out["stop_round"]
    else:
        assert int(out["rounds_run"]) == ROUNDS


def _runs_generic(eng):
    assert eng.layout["adam_spec"] is False, eng.layout
    assert eng.run(2) == 2
    assert np.all(np.isfinite(eng.global_flat())) and np.all(np.isfinite(eng.history()["loss"]))


@pytest.mark.parametrize("dims", NEAR_MISS, ids=["-".join(map(str, d)) for d in NEAR_MISS])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_near_miss_shapes_run_the_generic_adam(monkeypatch, dtype, dims):
    _runs_generic(_engine(monkeypatch, True, dims, 95, dict(dtype=dtype, early_stop=False)))


@pytest.mark.parametrize("kw", [dict(rows_per_block=16), dict(server_opt="adam", server_lr=0.1), dict(dp_clip=1.0)],
                         ids=["rows_per_block16", "server_opt", "dp_clip"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_other_round_kinds_run_the_generic_adam(monkeypatch, dtype, kw):
    _runs_generic(_engine(monkeypatch, True, DIMS, 95, dict(dict(dtype=dtype, early_stop=False), **kw)))

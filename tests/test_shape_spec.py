"""The shape-specialised train kernels (reference 14-50-200-2 MLP, R = 32) against the generic ones.

Two engines on the same data and seed, one constructed with the switch unset (specialised kernels,
``layout["shape_spec"]`` True) and one under ``FEDMI_SHAPE_SPEC=0`` (generic kernels), must agree
BITWISE -- ``np.array_equal``, no tolerance -- in the global weights, both Adam moments and the loss /
global / per-rank histories: the specialised kernels run the same MFMAs in the same order into the
same accumulators.  Shards of 32 rows (one full workgroup), 33 (a second workgroup with one live
row) and 95 (a partial last block) are the smallest inputs that exercise the row masking and the
multi-workgroup slab."""
import numpy as np
import pytest

from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass

pytestmark = pytest.mark.gpu

HIDDEN = (50, 200)
ROUNDS = 8
NEAR_MISS = [(14, 50, 200, 3), (15, 50, 200, 2), (14, 50, 208, 2), (14, 48, 200, 2)]
CASES = {
    "eager": dict(graph_rounds=0, early_stop=False),
    "graph4": dict(graph_rounds=4, early_stop=False),
    "local2_prox": dict(graph_rounds=0, early_stop=False, local_steps=2, prox_mu=0.05),
    # every metric within 1.0 of the previous round's: the patience of 3 runs out inside the run
    "early_stop": dict(graph_rounds=0, early_stop=True, patience=3, tolerance=1.0),
}


def _engine(monkeypatch, spec, dims, rows, dtype, kw):
    if spec:
        monkeypatch.delenv("FEDMI_SHAPE_SPEC", raising=False)
    else:
        monkeypatch.setenv("FEDMI_SHAPE_SPEC", "0")
    F, C = dims[0], dims[-1]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    cfg = EngineConfig(hidden=tuple(dims[1:-1]), max_rounds=ROUNDS + 2, rows_per_block=32, dtype=dtype, **kw)
    return HipRoundEngine(X, y, C, cfg, None, init_flat(list(dims), INIT_SEED))


def _outputs(eng):
    eng.run(ROUNDS)
    st = eng.portable_state()
    h = eng.history()
    return {"weights": eng.global_flat(), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"],
            "loss": h["loss"], "global": h["global"], "per_rank": h["per_rank"],
            "stop_round": np.asarray(h["stop_round"]), "rounds_run": np.asarray(h["rounds_run"])}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("rows", [32, 33, 95])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_specialised_round_is_bitwise_the_generic_round(monkeypatch, dtype, rows, case):
    dims = (14, *HIDDEN, 2)
    out = {}
    for spec in (True, False):
        eng = _engine(monkeypatch, spec, dims, rows, dtype, CASES[case])
        assert eng.R == 32
        assert eng.layout["shape_spec"] is spec, eng.layout
        out[spec] = _outputs(eng)
    if case == "early_stop":
        assert 0 < int(out[True]["stop_round"]) < ROUNDS, out[True]["stop_round"]
    else:
        assert int(out[True]["rounds_run"]) == ROUNDS
    for k in out[True]:
        assert np.array_equal(out[True][k], out[False][k]), (k, out[True][k], out[False][k])
    assert np.all(np.isfinite(out[True]["weights"])) and np.all(np.isfinite(out[True]["loss"]))


@pytest.mark.parametrize("dims", NEAR_MISS, ids=["-".join(map(str, d)) for d in NEAR_MISS])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_near_miss_shapes_run_the_generic_kernels(monkeypatch, dtype, dims):
    eng = _engine(monkeypatch, True, dims, 95, dtype, dict(graph_rounds=0, early_stop=False))
    assert eng.layout["shape_spec"] is False, eng.layout
    assert eng.run(2) == 2
    assert np.all(np.isfinite(eng.global_flat())) and np.all(np.isfinite(eng.history()["loss"]))

"""Low-rank update compression (``compress="powersgd"``) without a GPU: validation, layer selection and wire
size, the fp32 host model against its own float64 run, recovery of low-rank updates, torch group resume."""
import numpy as np
import pytest

from fedmi.fl.compress import (ALL_COMPRESSORS, COMPRESSOR_KINDS, compress_id, compress_k, lowrank_layers, lowrank_q0,
                               lowrank_torch, uplink_bytes)
from fedmi.fl.engine import EngineConfig, TorchRoundEngine
from fedmi.fl.simulate import ClientGroup

from .reference_oracle import nerr
from .server_oracle import shape_data

SHAPES = {"small": [17, 24, 3], "14-50-200-2": [14, 50, 200, 2]}
cases = lambda f: pytest.mark.parametrize("shape", sorted(SHAPES))(pytest.mark.parametrize("r", [1, 2, 4, 8])(f))


@pytest.mark.parametrize("kw, field", [(dict(compress_rank=0), "compress_rank"), (dict(compress_rank=9), "compress_rank"),
                                       (dict(compress_rank=2.0), "compress_rank"), (dict(compress_seed=-1), "compress_seed"),
                                       (dict(error_feedback=1), "error_feedback"), (dict(dp_clip=0.5, dp_seed=1), "dp_clip")])
def test_validation_names_the_field(kw, field):
    assert COMPRESSOR_KINDS == ALL_COMPRESSORS + ("powersgd",) and EngineConfig().compress_rank == 4
    assert compress_id(EngineConfig(compress="powersgd")) == 5
    X, y, C, flat = shape_data("small")
    for make in (compress_id, lambda cfg: TorchRoundEngine(X, y, C, cfg, None, flat)):
        with pytest.raises(ValueError, match=field):
            make(EngineConfig(hidden=(24,), max_rounds=2, compress="powersgd", **kw))


# compressed layers by r (N + K) < N K, and 4 (sum r (N + K) + every raw entry) bytes
WIRE = {"14-50-200-2": {1: ([1, 1, 1], 3072), 2: ([1, 1, 0], 5120), 4: ([1, 1, 0], 7632), 8: ([1, 1, 0], 12656)},
        "small": {1: ([1, 1], 380), 2: ([1, 1], 652), 4: ([1, 0], 1052), 8: ([1, 0], 1708)}}


@cases
def test_layer_selection_and_wire_size(shape, r):
    dims, (comp, nbytes) = SHAPES[shape], WIRE[shape][r]
    plan = lowrank_layers(dims, r)
    assert [int(ly["compressed"]) for ly in plan["layers"]] == comp
    assert all(r < min(ly["N"], ly["K"]) for ly in plan["layers"] if ly["compressed"])
    assert plan["q_len"] == r * sum(ly["K"] for ly in plan["layers"] if ly["compressed"]) == len(lowrank_q0(dims, r, 3))
    k = compress_k(EngineConfig(compress="powersgd", compress_rank=r), plan["P"], dims)
    assert uplink_bytes("powersgd", k, plan["P"]) == nbytes < 4 * plan["P"]
    np.testing.assert_array_equal(lowrank_q0(dims, r, 3), lowrank_q0(dims, r, 3))
    assert np.abs(lowrank_q0(dims, r, None) - lowrank_q0(dims, r, None)).max() > 0   # private draws


@cases
def test_fp32_model_against_its_float64_run_and_recovery(shape, r):
    """Gaussian updates of scale 0.05, four warm-started iterations: max|err| / max|ref| of c within the project's
    2e-5 (sequential sums of this rule gave 3.6e-7 .. 9.9e-7).  Then a u whose compressed layers have rank <= r comes
    back (c against u) within 2e-5 (that check gave at most 5.5e-6), the residual correspondingly small, raw entries exact."""
    dims, plan = SHAPES[shape], lowrank_layers(SHAPES[shape], r)
    g = np.random.default_rng(plan["P"] + r)
    q = lowrank_q0(dims, r, 7)
    q64 = q.astype(np.float64)
    for it in range(4):
        u = (0.05 * g.standard_normal(plan["P"])).astype(np.float32)
        c, e, q, s = lowrank_torch(u, q, dims, r)
        c64, _, q64, s64 = lowrank_torch(u.astype(np.float64), q64, dims, r)
        print(f"{shape} r{r} iteration {it}: c {nerr(c.numpy(), c64.numpy()):.3g}  stat {s:.6f} / {s64:.6f}")
        assert nerr(c.numpy(), c64.numpy()) <= 2e-5 and abs(s - s64) <= 2e-5 and 0 < s < 1
        np.testing.assert_array_equal(e.numpy(), u - c.numpy())
    raw = np.ones(plan["P"], bool)
    for ly in (ly for ly in plan["layers"] if ly["compressed"]):
        low = 0.05 * g.standard_normal((ly["N"], r)) @ g.standard_normal((r, ly["K"]))
        u[ly["w_off"]:ly["b_off"]], raw[ly["w_off"]:ly["b_off"]] = low.astype(np.float32).reshape(-1), False
    c, e, _, stat = lowrank_torch(u, lowrank_q0(dims, r, 1), dims, r)
    print(f"{shape} r{r}: c vs u {nerr(c.numpy(), u):.3g}  stat {stat:.3g}")
    assert nerr(c.numpy(), u) <= 2e-5 and np.abs(e.numpy()).max() <= 2e-5 * np.abs(u).max() and stat <= 2e-5
    assert (c.numpy()[raw] == u[raw]).all() and not e.numpy()[raw].any()


def test_torch_group_repeats_and_resumes_through_compress_q():
    X, y, _, _ = shape_data("small")
    mk = lambda **kw: ClientGroup(X, y, 4, EngineConfig(**{**dict(
        hidden=(24,), max_rounds=8, early_stop=False, compress="powersgd", compress_rank=2, compress_seed=9,
        participation=0.75), **kw}), backend="torch")
    state = lambda g: [np.concatenate([e.global_flat(), e.local_flat(), e.compress_residual.numpy(), e.compress_q.numpy(),
                                       e.history()["compress_stat"]]).view(np.uint32) for e in g.clients]
    a, b, c = mk(), mk(), mk()
    a.run(6)
    b.run(3)
    states = [e.portable_state() for e in b.clients]
    assert all(st["compress_q"].shape == (e.compress_q_len,) and "compress_seed" not in st for st, e in zip(states, b.clients))
    for e, st in zip(c.clients, states):
        e.load_portable_state(st)
    c.rounds = 3
    b.run(3)
    c.run(3)
    for sa, sb, sc in zip(state(a), state(b), state(c)):
        np.testing.assert_array_equal(sa, sb)
        np.testing.assert_array_equal(sa, sc)
    assert all(np.abs(e.compress_residual.numpy()).max() > 0 for e in a.clients)
    for kw in (dict(compress_rank=4), dict(compress="sign")):
        with pytest.raises(ValueError, match="compress_q"):
            mk(**kw).clients[0].load_portable_state(states[0])

"""``compress="mx"`` without a GPU: validation, wire size, ``mx_quantize`` on the grid inputs, unbiasedness, resume."""
import numpy as np
import pytest

from fedmi.fl.compress import (ALL_COMPRESSORS, BLOCK_COMPRESSORS, COMPRESSOR_KINDS, COMPRESSOR_NAMES, MX_FORMATS,
                               compress_id, compress_words, mx_grid, mx_quantize, uplink_bytes)
from fedmi.fl.engine import EngineConfig
from fedmi.fl.simulate import ClientGroup

from .server_oracle import shape_data

EMAX = {"e4m3": 8, "e5m2": 15, "e2m1": 2}
SCALES = (-60, -3, 0, 7, 40)   # block scale exponents e of the grid inputs, block b takes SCALES[b % 5]


def grid_inputs(fmt, P):
    """``(u, e, t)``: every block starts with the pilot ``2**emax * 2**e``, which fixes its scale; the other 31
    entries walk, from the top of the grid down, all pairs of adjacent grid values (0 to the smallest subnormal
    and the maximum to ``2**(emax + 1)`` included): the midpoint and its two fp32 neighbours, in both signs."""
    g = np.append(mx_grid(fmt), 2.0 ** (EMAX[fmt] + 1)).astype(np.float32)
    mid = ((g[:-1] + g[1:]) / 2)[::-1]
    t3 = np.stack([np.nextafter(mid, np.float32(0)), mid, np.nextafter(mid, np.float32(np.inf))], 1).reshape(-1)
    vals = np.stack([t3, -t3], 1).reshape(-1)
    nb = -(-P // 32)
    t = np.concatenate([np.full((nb, 1), 2.0 ** EMAX[fmt], np.float32), np.resize(vals, (nb, 31))], 1).reshape(-1)[:P]
    e = np.repeat(np.resize(SCALES, nb), 32)[:P]
    return np.ldexp(t, e).astype(np.float32), e, t


def test_names_validation_and_wire_size():
    assert COMPRESSOR_KINDS == ALL_COMPRESSORS + ("powersgd",) and BLOCK_COMPRESSORS == ("mx",)
    assert COMPRESSOR_NAMES == COMPRESSOR_KINDS + ("mx",) and MX_FORMATS == ("e4m3", "e5m2", "e2m1")
    cfg = EngineConfig(compress="mx")
    assert (cfg.compress_format, cfg.compress_rounding, compress_id(cfg)) == ("e4m3", "nearest", 6)
    assert all(compress_id(EngineConfig(compress="mx", compress_format=f, compress_rounding=r, error_feedback=ef)) == 6
               for f in MX_FORMATS for r in ("nearest", "stochastic") for ef in (True, False))
    for kw, field in [(dict(compress_format="e3m2"), "compress_format"), (dict(compress_format=0), "compress_format"),
                      (dict(compress_rounding="up"), "compress_rounding"), (dict(compress_rounding=True), "compress_rounding"),
                      (dict(error_feedback=1), "error_feedback"), (dict(dp_clip=0.5, dp_seed=1), "dp_clip")]:
        with pytest.raises(ValueError, match=field):
            compress_id(EngineConfig(compress="mx", **kw))
    assert [uplink_bytes("mx", 11352, 11352, fmt=f) for f in MX_FORMATS] == [11707, 11707, 6031]


@pytest.mark.parametrize("fmt", MX_FORMATS)
def test_rule_on_the_grid_inputs(fmt):
    u, e, t = grid_inputs(fmt, 11352)
    grid, w = mx_grid(fmt), compress_words("mx", u.size, 5, 0, 0)
    step = np.diff(grid)[np.minimum(np.searchsorted(grid, np.abs(t), side="right") - 1, len(grid) - 2)]
    for rounding in ("nearest", "stochastic"):
        c, raw, stat = mx_quantize(u, fmt, rounding, w)
        q = np.ldexp(c.numpy().astype(np.float64), -e)
        assert not raw.any() and stat == 2.0 ** max(SCALES) and np.isin(np.abs(q), grid).all()
        assert (np.signbit(q) == np.signbit(u)).all() and (np.abs(q)[np.abs(t) >= grid[-1]] == grid[-1]).all()
        below = np.abs(t) < grid[-1]
        err = np.abs(np.abs(q) - np.abs(t.astype(np.float64)))[below]
        assert (err <= 0.5 * step[below]).all() if rounding == "nearest" else (err < step[below]).all()
        if rounding == "nearest":   # a midpoint between codes i and i + 1 lands on whichever is even
            lo = np.minimum(np.searchsorted(grid, np.abs(t), side="right") - 1, len(grid) - 2)
            tie = below & (np.abs(t) == (grid[lo] + grid[lo + 1]) / 2)
            assert tie.sum() >= 2 * (len(grid) - 1) and (np.searchsorted(grid, np.abs(q)[tie]) % 2 == 0).all()


@pytest.mark.parametrize("fmt", MX_FORMATS)
def test_stochastic_rounding_is_unbiased(fmt):
    """One block over the words of n = 4096 consecutive rounds.  Entry i rounds up with probability frac_i, so
    its mean has the standard error (h - l) sqrt(frac (1 - frac) / n); 5 of them bound |mean - u| (a 5.7e-7 event
    per entry for a fair stream; entries on the grid have no error at all)."""
    n, grid = 4096, mx_grid(fmt)
    g = np.random.default_rng(EMAX[fmt])
    u = np.float32(g.uniform(-1, 1, 32) * grid[-1] * np.exp2(-g.integers(0, 6, 32)))
    u[0] = grid[-1]   # scale 2**0: t = |u|
    mean = np.mean([mx_quantize(u, fmt, "stochastic", compress_words("mx", 32, 7, r, 2))[0].numpy().astype(np.float64)
                    for r in range(n)], 0)
    t = np.abs(u.astype(np.float64))
    lo = np.searchsorted(grid, t, side="right") - 1
    l, h = grid[lo], grid[np.minimum(lo + 1, len(grid) - 1)]
    frac = (t - l) / np.where(h > l, h - l, 1.0)
    se = (h - l) * np.sqrt(frac * (1 - frac) / n)
    assert (se[1:] > 0).all() and (np.abs(mean - u) <= 5 * se).all(), np.abs(mean - u) / np.maximum(se, 1e-300)


def test_torch_group_runs_and_resumes_bit_for_bit_with_stochastic_rounding():
    X, y, _, _ = shape_data("small")
    mk = lambda: ClientGroup(X, y, 3, EngineConfig(hidden=(24,), max_rounds=8, early_stop=False, compress="mx",
                                                   compress_format="e2m1", compress_rounding="stochastic",
                                                   compress_seed=None, participation=0.7), backend="torch")
    state = lambda g: [np.concatenate([e.global_flat(), e.local_flat(), e.compress_residual.numpy(),
                                       e.history()["compress_stat"]]).view(np.uint32) for e in g.clients]
    a, b = mk(), mk()
    a.run(3)
    states = [e.portable_state() for e in a.clients]
    assert len({st["compress_seed"] for st in states}) == 3   # private seeds travel in the state
    for e, st in zip(b.clients, states):
        e.load_portable_state(st)
    b.rounds = 3
    a.run(3)
    b.run(3)
    for sa, sb in zip(state(a), state(b)):
        np.testing.assert_array_equal(sa, sb)
    assert all(np.abs(e.compress_residual.numpy()).max() > 0 and e.history()["compress_stat"].max() > 0 for e in a.clients)
    assert a.clients[0].uplink_bytes() == uplink_bytes("mx", 507, 507, fmt="e2m1") == 16 + 254

"""``compress="mx"`` on the GPU: ``mx_launch`` (fl_mx.hip) against the host rule ``mx_quantize`` on the same inputs,
bitwise; the engine checked in situ from its own buffers; graph replays against eager rounds."""
import numpy as np
import pytest
import torch

from fedmi.fl.compress import MX_FORMATS, compress_round, uplink_bytes
from fedmi.models.mlp import image_to_dense, param_count
from fedmi.privacy import philox

from .test_compress_mx_cpu import EMAX, grid_inputs
from .test_compress_random import (COMM_GARBAGE, MAX_ROUNDS, OUT_GARBAGE, SEED, STAT_GARBAGE, KernelCase, _bits, _engine,
                                   _same_bits)

pytestmark = pytest.mark.gpu

# 17-24-3: P = 507, 16 blocks, the last with 27 entries, one partial workgroup; 14-50-200-2: 355 blocks, 12 workgroups
DIMS = {"17-24-3": [17, 24, 3], "14-50-200-2": [14, 50, 200, 2]}
# "integer": nearest rounding forced onto the integer conversion, whichever path the kernel file chose for it
PATHS = {"nearest": (False, -1), "integer": (False, 0), "stochastic": (True, -1)}
FLT_MAX = np.finfo(np.float32).max


def _inputs(kind, fmt, P):
    g = np.random.default_rng(P)
    if kind == "random":   # exponents spread over 40 binades
        x = g.standard_normal(P).astype(np.float32)
        spread = lambda: np.ldexp(g.standard_normal(P), g.integers(-30, 10, P)).astype(np.float32)
        return x + spread(), x, spread()
    # crafted u: local = -0 and x = +0, so u = (-0) + e = e with the sign of a zero kept
    u = grid_inputs(fmt, P)[0]
    if kind == "special":
        u = np.ldexp(g.standard_normal(P), g.integers(-3, 3, P)).astype(np.float32)
        u[0:32] = np.resize(np.float32([0.0, -0.0, -0.0]), 32)             # a zero block
        u[40], u[70] = np.inf, np.nan                                    # raw blocks
        tiny = np.float32([1.5, -1.0, 0.75, 2.0 ** -30, -(2.0 ** -53), 2.0 ** -31 * 1.999])
        u[96:128] = np.resize(np.ldexp(tiny, -96), 32)                   # E = 31: signed zeros
        u[128:160] = np.resize(np.ldexp(tiny, -95), 32)                  # E = 32: the first quantised scale,
        u[130], u[131] = -(2.0 ** -127), np.nextafter(np.float32(2.0 ** -126), np.float32(0))   # denormal entries
        u[160:192] = np.resize(np.float32([FLT_MAX, -FLT_MAX / 3, 1e38, -1e30, 1.0]), 32)
        u[P - 1] = -FLT_MAX                                              # the largest magnitude, partial block
    return np.full(P, -0.0, np.float32), np.zeros(P, np.float32), u


def _launch(c, fmt, path, ef):
    torch.cuda.synchronize()
    c.m.mx_launch(c.dims, MX_FORMATS.index(fmt), PATHS[path][0], bool(ef), c.local.data_ptr(), c.x.data_ptr(),
                  c.comm.data_ptr(), c.res.data_ptr(), c.stat.data_ptr(), c.state.data_ptr(), c.rtab.data_ptr(), MAX_ROUNDS,
                  torch.cuda.current_stream().cuda_stream, client=c.client, seed=SEED, conv=PATHS[path][1])
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("shape", sorted(DIMS))
@pytest.mark.parametrize("inputs", ["random", "grid", "special"])
@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("fmt", MX_FORMATS)
def test_kernel_is_mx_quantize_bitwise(fmt, path, inputs, shape):
    dims = DIMS[shape]
    P = param_count(dims)
    local, x, e = _inputs(inputs, fmt, P)
    rounding = "stochastic" if PATHS[path][0] else "nearest"
    for r, ef in ((2, True), (3, False), (3, True)):   # both buffer parities
        c = _launch(KernelCase(dims, local, x, e, 0.3, r), fmt, path, ef)
        c.check_untouched(("local", "x"))
        np.testing.assert_array_equal(_bits(c.half(r & 1)), _bits(c.half(r & 1, c.before[2])))   # the old half
        comm, out, stat = c.comm.cpu().numpy(), c.half((r + 1) & 1), c.stat.cpu().numpy()
        assert (comm[:c.Pimg][c.pad] == COMM_GARBAGE).all() and (comm[c.Pimg:] == COMM_GARBAGE).all(), "comm padding"
        assert (out[c.pad] == OUT_GARBAGE).all() and (np.delete(stat, r) == STAT_GARBAGE).all()
        want, e_new, st = compress_round(local, x, e, c.w, "mx", 0, ef, seed=SEED, round=r, client=c.client, fmt=fmt,
                                         rounding=rounding)
        _same_bits(image_to_dense(comm[:c.Pimg], dims), want.numpy(), f"contribution r{r} ef{ef}")
        _same_bits(image_to_dense(out, dims), e_new.numpy(), f"residual r{r} ef{ef}")
        assert stat[r] == np.float32(st) > 0
        if inputs == "special":
            assert stat[r] == 2.0 ** (127 - EMAX[fmt]) and np.isnan(want.numpy()[70]) and not e_new.numpy()[32:96].any()


@pytest.mark.parametrize("shape", sorted(DIMS))
def test_kernel_no_op_cases(shape):
    from fedmi.ops import native
    assert native().MX_STREAM == philox.MX_STREAM and native().COMPRESS_MX == 6
    dims = DIMS[shape]
    local, x, e = _inputs("random", "e4m3", param_count(dims))
    for r in (2, 3):
        c = _launch(KernelCase(dims, local, x, e, 0.0, r), "e5m2", "stochastic", True)   # not sampled
        c.check_untouched(("local", "x", "comm"))
        np.testing.assert_array_equal(_bits(c.half(r & 1)), _bits(c.half(r & 1, c.before[2])))
        out, stat = c.half((r + 1) & 1), c.stat.cpu().numpy()
        assert (out[c.pad] == OUT_GARBAGE).all() and stat[r] == 0 and (np.delete(stat, r) == STAT_GARBAGE).all()
        np.testing.assert_array_equal(_bits(image_to_dense(out, dims)), _bits(e))
        _launch(KernelCase(dims, local, x, e, 0.3, r, live=False), "e2m1", "nearest", True).check_untouched(
            ("local", "x", "residual", "comm", "stat"))                                  # not live


@pytest.mark.parametrize("shape", sorted(DIMS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("fmt, rounding", [("e4m3", "nearest"), ("e5m2", "stochastic"), ("e2m1", "nearest"), ("e2m1", "stochastic")])
def test_engine_rounds_follow_the_rule_bitwise(fmt, rounding, dtype, shape):
    """Step API, three local steps, four rounds: each round's contribution and residual against the rule applied
    to the engine's own local model, round input and old residual."""
    e = _engine(shape, compress="mx", compress_format=fmt, compress_rounding=rounding, dtype=dtype, local_steps=3)
    lay, d = e.layout["compress"], lambda t: image_to_dense(t.cpu().numpy(), e.dims)
    assert (lay["kind"], lay["format"], lay["rounding"], lay["dense_bytes"]) == ("mx", fmt, rounding, 4 * e.P)
    assert lay["uplink_bytes"] == uplink_bytes("mx", e.P, e.P, fmt=fmt) == e.uplink_bytes() < 4 * e.P
    assert e.compress_random == (rounding == "stochastic") and not e.engine.fused
    for r in range(4):
        e.step_train()
        e.stream.synchronize()
        old, new = (e.cp_res[q * e.Pimg:(q + 1) * e.Pimg] for q in (r & 1, (r + 1) & 1))
        w = float(e.rtab.cpu().numpy().view(np.float32)[4 * r])
        want, e_new, st = compress_round(d(e.local), d(e.params[r & 1][:e.Pimg]), d(old), w, "mx", 0, True, fmt=fmt,
                                         rounding=rounding, round=r, client=e.rank,
                                         seed=e.compress_seed if e.compress_random else 0)
        _same_bits(d(e.params[(r + 1) & 1][:e.Pimg]), want.numpy(), f"round {r}: contribution")
        _same_bits(d(new), e_new.numpy(), f"round {r}: residual")
        assert float(e.cp_stat[r]) == np.float32(st) > 0 and new.any()
        e.step_eval()
        e.step_aggregate()
    e.sync_history()
    assert e.history()["rounds_run"] == 4 and np.isfinite(e.global_flat()).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("fmt", MX_FORMATS)
def test_graph_replays_equal_eager_rounds_with_stochastic_rounding(fmt, dtype):
    """A two-round graph replayed twice against four eager rounds: the round word comes from the device state."""
    out = []
    for g in (0, 2):
        e = _engine("14-50-200-2", compress="mx", compress_format=fmt, compress_rounding="stochastic", dtype=dtype,
                    graph_rounds=g)
        e.run(4)
        assert (e.engine.graph_captures > 0) == (g > 0)
        out.append((e.global_flat(), e.compress_residual, e.history()["compress_stat"], e.history()["loss"]))
    for a, b in zip(*out):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert np.abs(out[1][1]).max() > 0 and (out[1][2] > 0).all()


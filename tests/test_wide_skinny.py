"""skinny_wgrad (the three instantiations the launcher knows, <14, 1, 0> included, which no caller
uses) and colsum_split against the float64 models of wide_oracle.py.

Conventions of test_layered_ops.py: seeded inputs, ldw = Nw + 8 and lds in {C, 64} with NaN pads,
outputs and slabs over-allocated and pre-filled (beta = 0 runs over NaN-filled outputs; the slab
starts as NaN everywhere), everything not owned keeps its bits.

Tolerance: ``lo.nerr`` against the float64 model within ``lo.bound`` of the transcription's own
error, the largest over the cases of the test.  The results are ALSO bit-equal to the
transcription, in every case here: a product of two bf16 values is exact in fp32, so the kernel's
fma and the transcription's multiply-then-add round once, identically; the column sums only add;
the partition, the per-split row order and the in-order slab fold are transcribed; and beta * out
is exact for beta in {1, 0.5}, so contracting it into the final add changes nothing.  (It would
not hold for a beta whose product rounds, e.g. 0.3.)"""
import numpy as np
import pytest
import torch

from fedmi.ops import native

from . import layered_oracle as lo
from . import wide_oracle as wo
from .test_layered_ops import SENT, TAIL, _s, assert_untouched, bits, dbuf, put2d, region, to_dev

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
BETAS = (0.0, 1.0, 0.5)
NAN_BITS = np.array([NAN], dtype=F32).view(np.int32)[0]      # what torch.full(nan) stores


@pytest.fixture(scope="module")
def m():
    return native()


def _out_buffer(o0, beta):
    """Flat output + sentinel tail: o0 for beta != 0, NaN (never to be read) for beta = 0."""
    n = o0.size
    buf = dbuf(n + TAIL, fill=NAN if beta == 0.0 else SENT)
    if beta != 0.0:
        buf[:n] = to_dev(o0.ravel())
    else:
        buf[n:] = SENT
    return buf


def _f32_bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ----------------------------------------------------------------------------- skinny_wgrad
INSTANCES = [(2, 0, False), (14, 1, True), (14, 1, False)]


@pytest.mark.parametrize("Nw", [8, 264, 2056])
@pytest.mark.parametrize("C,trans,bias", INSTANCES, ids=["C2", "C14_bias", "C14"])
def test_skinny_wgrad(m, C, trans, bias, Nw):
    """rows in {1, 5, 255, 256, 1000} x splits in {1, 3, rows, rows + 3} (empty row ranges, whose
    slabs must be zeros) x lds in {C, 64} x beta in {0, 1, 0.5}; Nw = 8 is one thread, 264 a
    partial block, 2056 a second block of one thread."""
    rng = np.random.RandomState(Nw + C)
    ldw = Nw + 8
    stride = (C + int(bias)) * Nw
    runs, e_tr = [], 0.0
    for rows in (1, 5, 255, 256, 1000):
        W = lo.bf16_round((rng.randn(rows, Nw) * 10.0 ** rng.randint(-2, 2, (rows, 1))).astype(F32))
        S = lo.bf16_round(rng.randn(rows, C).astype(F32))
        o0 = rng.randn(Nw, C).astype(F32) if trans else rng.randn(C, Nw).astype(F32)
        b0 = rng.randn(Nw).astype(F32)
        for splits in sorted({1, 3, rows, rows + 3}):
            slab = wo.skinny_slab(W, S, C, rows, trans, splits, bias)
            for beta in BETAS:
                r = wo.skinny_wgrad(W, S, C, rows, trans, splits, beta, o0, b0 if bias else None, slab=slab)
                e_tr = max([e_tr, lo.nerr(r["out"][1], r["out"][0], r["out"][2])] +
                           ([lo.nerr(r["bias"][1], r["bias"][0], r["bias"][2])] if bias else []))
                if slab.size > (1 << 22):
                    r["slab"] = None                          # recomputed below, not kept alive
                runs.append((rows, splits, beta, W, S, o0, b0, r))
    tb = lo.bound(e_tr)
    worst = 0.0
    for rows, splits, beta, W, S, o0, b0, r in runs:
        for lds in (C, 64):
            Wd, Sd = put2d(W, ldw, torch.bfloat16), put2d(S, lds, torch.bfloat16)
            out = _out_buffer(o0, beta)
            bout = _out_buffer(b0, beta) if bias else None
            sl = dbuf(splits * stride + TAIL, fill=NAN)
            b_out, b_b = bits(out), (bits(bout) if bias else None)
            m.skinny_wgrad(Wd.data_ptr(), ldw, Nw, Sd.data_ptr(), lds, C, rows, trans, splits, sl.data_ptr(),
                           out.data_ptr(), beta, bout.data_ptr() if bias else 0, _s())
            what = f"skinny C={C} Nw={Nw} rows={rows} splits={splits} lds={lds} beta={beta}"
            assert_untouched(out, b_out, region(out.numel(), 0, 1, C * Nw, C * Nw), what + " out")
            want_slab = r["slab"] if r["slab"] is not None else wo.skinny_slab(W, S, C, rows, trans, splits, bias)
            gs = _f32_bits(sl.cpu().numpy())
            assert (gs[splits * stride:] == NAN_BITS).all(), what + ": slab written past splits * stride"
            got = out[:C * Nw].cpu().numpy().reshape(r["out"][0].shape)
            assert np.isfinite(got).all(), what
            e = lo.nerr(got, r["out"][0], r["out"][2])
            worst = max(worst, e)
            assert e <= tb, f"{what}: err {e:.3e} > bound {tb:.3e}"
            np.testing.assert_array_equal(_f32_bits(got), _f32_bits(r["out"][1]), err_msg=what + " vs transcription")
            gs = gs[:splits * stride].reshape(splits, stride)
            np.testing.assert_array_equal(gs, _f32_bits(want_slab), err_msg=what + " slab")
            rc = -(-rows // splits)
            assert (gs[[z for z in range(splits) if z * rc >= rows]] == 0).all(), what + " empty ranges"   # +0 bits
            if bias:
                assert_untouched(bout, b_b, region(bout.numel(), 0, 1, Nw, Nw), what + " bias_out")
                gb = bout[:Nw].cpu().numpy()
                assert np.isfinite(gb).all(), what
                e = lo.nerr(gb, r["bias"][0], r["bias"][2])
                worst = max(worst, e)
                assert e <= tb, f"{what}: bias err {e:.3e} > bound {tb:.3e}"
                np.testing.assert_array_equal(_f32_bits(gb), _f32_bits(r["bias"][1]), err_msg=what + " bias")
    print(f"skinny_wgrad C={C} trans={trans} bias={bias} Nw={Nw}: worst err {worst:.3e} (transcription {e_tr:.3e}) "
          f"bound {tb:.3e}, err / bound {worst / tb:.3f}")


SKINNY_BAD = {
    "Nw%8": dict(Nw=12), "ldw%8": dict(ldw=20), "W_misaligned": dict(woff=4), "splits<1": dict(splits=0),
    "lds<C": dict(lds=1), "C2_trans1": dict(trans=1), "C14_trans0": dict(C=14, lds=14), "C3": dict(C=3, lds=3),
}


@pytest.mark.parametrize("bad", sorted(SKINNY_BAD))
def test_skinny_wgrad_guards(m, bad):
    """Each guard raises and writes nothing (the buffers would fit the launch if it ran)."""
    kw = dict(Nw=16, ldw=24, woff=0, splits=2, lds=2, C=2, trans=0, rows=8)
    kw.update(SKINNY_BAD[bad])
    W, S = dbuf(8 + kw["rows"] * 32, torch.bfloat16, 1.0), dbuf(kw["rows"] * 64, torch.bfloat16, 1.0)
    out, sl = dbuf(16 * 32), dbuf(4 * 16 * 32, fill=NAN)
    b_out, b_sl = bits(out), bits(sl)
    with pytest.raises(RuntimeError):
        m.skinny_wgrad(W[kw["woff"]:].data_ptr(), kw["ldw"], kw["Nw"], S.data_ptr(), kw["lds"], kw["C"], kw["rows"],
                       kw["trans"], kw["splits"], sl.data_ptr(), out.data_ptr(), 0.0, 0, _s())
    torch.cuda.synchronize()
    assert_untouched(out, b_out, np.zeros(out.numel(), dtype=bool), bad)
    assert_untouched(sl, b_sl, np.zeros(sl.numel(), dtype=bool), bad)


# ----------------------------------------------------------------------------- colsum_split
@pytest.mark.parametrize("N", [1, 2, 3, 14, 64])
def test_colsum_split(m, N):
    """M in {1, 7, 1000, 4097} x splits in {1, 7, M, M + 5} x beta in {0, 1, 0.5}.  The launcher
    runs eff = ceil(M / ceil(M / splits)) blocks: the slab's rows past eff keep their bits."""
    rng = np.random.RandomState(N)
    runs, e_tr = [], 0.0
    for M in (1, 7, 1000, 4097):
        X = (rng.randn(M, N) * 10.0 ** rng.randint(-3, 3, (M, 1))).astype(F32)
        o0 = rng.randn(N).astype(F32)
        for splits in sorted({1, 7, M, M + 5}):
            pre = wo.colsum_slab(X, splits)
            for beta in BETAS:
                (ref, tr, scale), slab, eff = wo.colsum_split(X, splits, beta, o0, slab=pre)
                e_tr = max(e_tr, lo.nerr(tr, ref, scale))
                runs.append((M, splits, beta, X, o0, ref, tr, scale, slab, eff))
    tb = lo.bound(e_tr)
    worst = 0.0
    for M, splits, beta, X, o0, ref, tr, scale, slab, eff in runs:
        Xd = dbuf(M * N + TAIL, fill=NAN)
        Xd[:M * N] = to_dev(X.ravel())
        out = _out_buffer(o0, beta)
        sl = dbuf(splits * N + TAIL, fill=NAN)
        b_out, b_sl = bits(out), bits(sl)
        m.colsum_split(Xd.data_ptr(), M, N, splits, sl.data_ptr(), out.data_ptr(), beta, _s())
        what = f"colsum_split M={M} N={N} splits={splits} beta={beta}"
        assert_untouched(out, b_out, region(out.numel(), 0, 1, N, N), what + " out")
        assert_untouched(sl, b_sl, region(sl.numel(), 0, 1, eff * N, eff * N), what + " slab")
        got = out[:N].cpu().numpy()
        assert np.isfinite(got).all(), what
        e = lo.nerr(got, ref, scale)
        worst = max(worst, e)
        assert e <= tb, f"{what}: err {e:.3e} > bound {tb:.3e}"
        np.testing.assert_array_equal(_f32_bits(got), _f32_bits(tr), err_msg=what + " vs transcription")
        np.testing.assert_array_equal(_f32_bits(sl[:eff * N].cpu().numpy()), _f32_bits(slab.ravel()), err_msg=what)
    print(f"colsum_split N={N}: worst err {worst:.3e} (transcription {e_tr:.3e}) bound {tb:.3e}, "
          f"err / bound {worst / tb:.3f}")


@pytest.mark.parametrize("N", [0, 65])
def test_colsum_split_guards(m, N):
    X, out, sl = dbuf(8 * 80, fill=1.0), dbuf(80), dbuf(4 * 80, fill=NAN)
    b_out, b_sl = bits(out), bits(sl)
    with pytest.raises(RuntimeError):
        m.colsum_split(X.data_ptr(), 8, N, 2, sl.data_ptr(), out.data_ptr(), 0.0, _s())
    torch.cuda.synchronize()
    assert_untouched(out, b_out, np.zeros(80, dtype=bool), f"N={N}")
    assert_untouched(sl, b_sl, np.zeros(4 * 80, dtype=bool), f"N={N}")

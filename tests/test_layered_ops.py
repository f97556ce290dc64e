"""The layered-path HIP kernels one by one (mlp_ops.hip, the small kernels of gemm_mfma.hip, the
helpers at the end of gemm_nt_bf16.hip) against the float64 models of layered_oracle.py.

Conventions of every case: seeded inputs; outputs live in over-allocated buffers pre-filled with a
sentinel, and every element the operation does not own (past n, past C within lddz / ldo, past N
within ld, an inactive trial) must keep its bits; input pads hold NaN or 1e30 so that a read past
the logical width shows in the result.

Tolerances.  Conversions, gathers, counts and the stopping rule are compared exactly.  For the
fp32 arithmetic kernels the bound is computed from the inputs: the float32 transcription of the
same formula (layered_oracle.*_f32, the kernel's operation order) is measured against the float64
model, each element's error in units of the magnitude of its own terms (``lo.nerr``: for a sum,
sum |terms|), and the kernel is allowed four times the largest such error over the inputs of the
test (``lo.bound``).  That margin covers fma contraction, expf / logf / sqrtf differing from
numpy's by an ulp or two and a different but fixed summation order, nothing else.  Double
accumulators fed by atomics get float64 epsilon x (blocks + in-block roundings) x sum |terms|."""
import numpy as np
import pytest
import torch

from fedmi.ops import native

from . import layered_oracle as lo

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = -1234.5
EPS64 = float(np.finfo(np.float64).eps)
TAIL = 8                       # sentinel elements past every buffer's logical end


@pytest.fixture(scope="module")
def m():
    return native()


def _dev():
    return torch.device("cuda", 0)


def _s():
    return torch.cuda.current_stream().cuda_stream


def dbuf(total, dtype=torch.float32, fill=SENT):
    return torch.full((int(total),), fill, dtype=dtype, device=_dev())


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(device=_dev(), dtype=dtype if dtype is not None else t.dtype).contiguous()


def put2d(store, ld, dtype=torch.float32, fill=float("nan"), tail=TAIL):
    """[rows][cols] -> flat device buffer [rows * ld + tail] with row stride ld, pads = fill."""
    rows, cols = store.shape
    buf = dbuf(rows * ld + tail, dtype, fill)
    buf[:rows * ld].view(rows, ld)[:, :cols] = to_dev(store).to(dtype)
    return buf


_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    torch.cuda.synchronize()
    c = t.detach().cpu().contiguous()
    return c.view(_INT[c.element_size()]).numpy().copy()


def region(total, start, rows, ld, cols):
    """Mask of the elements of a [rows][ld] matrix at `start` that lie in its first `cols` columns."""
    w = np.zeros(int(total), dtype=bool)
    if rows and cols:
        w[(start + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).ravel()] = True
    return w


def assert_untouched(buf, before, owned, what=""):
    after = bits(buf)
    bad = np.flatnonzero((after != before) & ~owned)
    assert bad.size == 0, f"{what}: {bad.size} elements outside the output changed, first at {bad[:8]}"


def cpu_bf16_bits(x: torch.Tensor):
    return x.to(torch.bfloat16).view(torch.int16).numpy()


SPECIAL_BITS = np.array(
    [0x3F808000, 0x3F818000,              # exact ties below an even / an odd bf16 mantissa
     0xBF808000, 0xBF818000,
     0x3FFFFFFF, 0x3F7FFFFF, 0x477FFFFF,  # round up into the next binade
     0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
     0x7F7FFFFF, 0xFF7FFFFF,              # largest finite fp32
     0x7FC00000, 0xFFC00001,              # NaN
     0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00400000],   # subnormals
    dtype=np.uint32).view(F32)


def special_values(rng, n):
    x = (rng.randn(n) * 10.0 ** rng.randint(-6, 6, n)).astype(F32)
    k = min(n, len(SPECIAL_BITS))
    x[rng.permutation(n)[:k]] = SPECIAL_BITS[rng.permutation(len(SPECIAL_BITS))[:k]]
    return x


def assert_bf16_equal(got_bits, want_bits, what=""):
    """Bit equality, NaN compared by isnan (bf16 bits: exponent all ones, mantissa non-zero)."""
    g, w = got_bits.view(np.uint16), want_bits.view(np.uint16)
    gn, wn = (g & 0x7FFF) > 0x7F80, (w & 0x7FFF) > 0x7F80
    np.testing.assert_array_equal(gn, wn, err_msg=what + " (NaN positions)")
    np.testing.assert_array_equal(g[~gn], w[~wn], err_msg=what)


# ----------------------------------------------------------------------------- bf16 conversions
@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_to_bf16_is_round_to_nearest_even(m, scale):
    """y = bf16(scale * x) bit-equal to torch's CPU cast of the fp32 product, ties / carries /
    zeros / infinities / NaN / subnormals included (subnormals are kept, as torch keeps them)."""
    rng = np.random.RandomState(1)
    for n in (1, 255, 256, 257, 1025):
        for rep in range(3 if n == 1 else 1):
            x = special_values(rng, n) if n > 1 else SPECIAL_BITS[[0, 1, 15][rep]:][:1].copy()
            want = cpu_bf16_bits(torch.from_numpy(x) * torch.tensor(scale, dtype=torch.float32))
            xd = to_dev(x)
            y = dbuf(n + TAIL, torch.bfloat16)
            before = bits(y)
            m.to_bf16(xd.data_ptr(), y.data_ptr(), n, _s(), scale)
            assert_untouched(y, before, region(n + TAIL, 0, 1, n, n), f"to_bf16 n={n}")
            assert_bf16_equal(bits(y)[:n], want, f"to_bf16 n={n} scale={scale}")
    # every special value, in order (n = 21)
    xd, y = to_dev(SPECIAL_BITS.copy()), dbuf(len(SPECIAL_BITS) + TAIL, torch.bfloat16)
    m.to_bf16(xd.data_ptr(), y.data_ptr(), len(SPECIAL_BITS), _s(), scale)
    want = cpu_bf16_bits(torch.from_numpy(SPECIAL_BITS.copy()) * torch.tensor(scale, dtype=torch.float32))
    assert_bf16_equal(bits(y)[:len(SPECIAL_BITS)], want, "to_bf16 specials")


@pytest.mark.parametrize("R,C,ldo", [(1, 1, 8), (5, 14, 64), (7, 64, 64), (33, 2, 64)])
@pytest.mark.parametrize("transposing", [False, True])
def test_pad_bf16(m, R, C, ldo, transposing):
    """out[r][c] = bf16(in[r*rs + c*cs]) for c < C, pad columns exactly +0, nothing past R*ldo."""
    rng = np.random.RandomState(R * 100 + C)
    logical = special_values(rng, R * C).reshape(R, C)
    store = np.ascontiguousarray(logical.T) if transposing else logical      # (rs, cs) = (1, R) reads [C][R]
    rs, cs = (1, R) if transposing else (C, 1)
    xd = to_dev(store)
    out = dbuf(R * ldo + TAIL, torch.bfloat16)
    before = bits(out)
    m.pad_bf16(xd.data_ptr(), R, C, rs, cs, out.data_ptr(), ldo, _s())
    assert_untouched(out, before, region(R * ldo + TAIL, 0, R, ldo, ldo), "pad_bf16")
    got = bits(out)[:R * ldo].reshape(R, ldo)
    assert_bf16_equal(np.ascontiguousarray(got[:, :C]), cpu_bf16_bits(torch.from_numpy(logical.copy())), "pad_bf16")
    assert (got[:, C:] == 0).all()


@pytest.mark.parametrize("R,C", [(1, 1), (31, 33), (32, 32), (65, 7)])
def test_transpose_bf16(m, R, C):
    """out[c][r] = bf16(in[r][c]) with ldi > C and ldo > R; the columns past R keep their bits."""
    rng = np.random.RandomState(R + C)
    ldi, ldo = C + 3, R + 5
    x = special_values(rng, R * C).reshape(R, C)
    xd = put2d(x, ldi, fill=1e30)
    out = dbuf(C * ldo + TAIL, torch.bfloat16)
    before = bits(out)
    m.transpose_bf16(xd.data_ptr(), R, C, ldi, out.data_ptr(), ldo, _s())
    assert_untouched(out, before, region(C * ldo + TAIL, 0, C, ldo, R), "transpose_bf16")
    got = np.ascontiguousarray(bits(out)[:C * ldo].reshape(C, ldo)[:, :R])
    assert_bf16_equal(got, cpu_bf16_bits(torch.from_numpy(np.ascontiguousarray(x.T))), "transpose_bf16")


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
def test_rowsum_bf16(m, beta):
    """out[n] = beta*out[n] + sum_r dT[n][r].  Nrows covers a partial last block of 4 rows; M one
    lane (8), exactly one pass (512) and a second pass for some lanes (520).  Bound: 4x the error
    of a sequential fp32 sum (+ the beta product and add), relative to sum |terms|."""
    rng = np.random.RandomState(7)
    cases = []
    for Nrows in (1, 4, 5):
        for M in (8, 512, 520):
            d = lo.bf16_round((rng.randn(Nrows, M) * 10.0 ** rng.randint(-2, 3, (Nrows, 1))).astype(F32))
            o0 = rng.randn(Nrows).astype(F32)
            ref = beta * o0.astype(float) + d.astype(float).sum(1)
            scale = np.abs(beta * o0) + np.abs(d).astype(float).sum(1)
            acc = lo.sum_f32(d, 1)
            trans = F32(beta) * o0 + acc if beta != 0.0 else acc
            cases.append((Nrows, M, d, o0, ref, scale, lo.nerr(trans, ref, scale)))
    tb = lo.bound(max(c[-1] for c in cases))
    for Nrows, M, d, o0, ref, scale, _ in cases:
        ld = M + 8
        dT = put2d(d, ld, torch.bfloat16, fill=1e30)
        out = dbuf(Nrows + TAIL)
        out[:Nrows] = to_dev(o0)
        before = bits(out)
        m.rowsum_bf16(dT.data_ptr(), Nrows, M, ld, out.data_ptr(), beta, _s())
        assert_untouched(out, before, region(Nrows + TAIL, 0, 1, Nrows, Nrows), "rowsum_bf16")
        e = lo.nerr(out[:Nrows].cpu().numpy(), ref, scale)
        print(f"rowsum_bf16 Nrows={Nrows} M={M} beta={beta}: err {e:.3e} bound {tb:.3e}")
        assert e <= tb


def test_rowsum_bf16_rejects_m_not_multiple_of_8(m):
    dT, out = dbuf(64, torch.bfloat16, 1.0), dbuf(4)
    with pytest.raises(RuntimeError):
        m.rowsum_bf16(dT.data_ptr(), 1, 12, 16, out.data_ptr(), 0.0, _s())
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- FedAvg deltas
ALIGN = {"vector": (4, 8), "w_g_off_one_float": (5, 8), "d_off_one_bf16": (4, 9)}
FED_N = (1, 3, 4, 5, 1023, 1024, 1027)


@pytest.mark.parametrize("align", sorted(ALIGN))
def test_fedavg_delta_bf16(m, align):
    """d = bf16(scale * (w - g)) bit-equal to the fp32 CPU computation (a subtract then a multiply:
    nothing to contract), on the 4-wide vector path and on both scalar paths; the neighbours of
    the segment, which in a flat parameter buffer are the next layer, keep their bits."""
    rng = np.random.RandomState(11)
    fo, bo = ALIGN[align]
    scale = 0.37
    for n in FED_N:
        g = rng.randn(n).astype(F32)
        w = (g + rng.randn(n).astype(F32) * F32(1e-2)).astype(F32)
        wb, gb, db = dbuf(n + 16), dbuf(n + 16), dbuf(n + 24, torch.bfloat16)
        wb[fo:fo + n], gb[fo:fo + n] = to_dev(w), to_dev(g)
        assert (wb[fo:].data_ptr() % 16 == 0) == (fo == 4) and (db[bo:].data_ptr() % 8 == 0) == (bo == 8)
        before = bits(db)
        m.fedavg_delta_bf16(wb[fo:].data_ptr(), gb[fo:].data_ptr(), db[bo:].data_ptr(), n, scale, _s())
        assert_untouched(db, before, region(n + 24, bo, 1, n, n), f"fedavg_delta n={n}")
        want = cpu_bf16_bits((torch.from_numpy(w) - torch.from_numpy(g)) * torch.tensor(scale, dtype=torch.float32))
        np.testing.assert_array_equal(bits(db)[bo:bo + n], want, err_msg=f"n={n}")


@pytest.mark.parametrize("align", sorted(ALIGN))
def test_fedavg_apply_delta(m, align):
    """g_new = g + float(d) (one fp32 add) and w_new = g_new, bit for bit; neighbours untouched."""
    rng = np.random.RandomState(12)
    fo, bo = ALIGN[align]
    for n in FED_N:
        g = rng.randn(n).astype(F32)
        d = lo.bf16_round((rng.randn(n) * 1e-2).astype(F32))
        wb, gb, db = dbuf(n + 16), dbuf(n + 16), dbuf(n + 24, torch.bfloat16)
        gb[fo:fo + n] = to_dev(g)
        db[bo:bo + n] = to_dev(d).to(torch.bfloat16)
        bw, bg, bd = bits(wb), bits(gb), bits(db)
        m.fedavg_apply_delta(wb[fo:].data_ptr(), gb[fo:].data_ptr(), db[bo:].data_ptr(), n, _s())
        own = region(n + 16, fo, 1, n, n)
        assert_untouched(wb, bw, own, f"apply w n={n}")
        assert_untouched(gb, bg, own, f"apply g n={n}")
        assert_untouched(db, bd, np.zeros(n + 24, dtype=bool), f"apply d n={n}")
        want = (g + d).astype(F32)
        np.testing.assert_array_equal(bits(gb)[fo:fo + n], want.view(np.int32), err_msg=f"g n={n}")
        np.testing.assert_array_equal(bits(wb)[fo:fo + n], want.view(np.int32), err_msg=f"w n={n}")


def test_fedavg_bf16_round_trip_error_is_relative_to_the_update(m):
    """K = 4 clients, weights s_i summing to 1: d_i = bf16(s_i (w_i - g)), summed in bf16 on the
    host (the wire format), applied to g.  With U = max |w_i - g| and u = 2^-9 (bf16 unit roundoff):
    the K deltas' roundings total <= u sum_i s_i U = u U, the K - 1 bf16 partial sums add <= u U
    each (every partial sum is <= U in magnitude), so the bf16 error is <= K u U to first order;
    the fp32 steps (the subtract, the scale, the final add) add <= 4 * 2^-24 max |g_new|.  The bound
    scales with the UPDATE, not with the weights: |g| here is ~1000 times U."""
    rng = np.random.RandomState(13)
    n, K = 1027, 4
    s = [0.1, 0.2, 0.3, 0.4]
    g = rng.randn(n).astype(F32)
    ws = [(g + rng.randn(n).astype(F32) * F32(1e-3)).astype(F32) for _ in range(K)]
    gd = to_dev(g.copy())
    acc = None
    for w, si in zip(ws, s):
        d = dbuf(n, torch.bfloat16)
        wdev = to_dev(w)
        m.fedavg_delta_bf16(wdev.data_ptr(), gd.data_ptr(), d.data_ptr(), n, si, _s())
        torch.cuda.synchronize()
        d = d.cpu()
        acc = d if acc is None else (acc + d)          # torch CPU bf16 add: rounded to bf16 each time
    assert acc.dtype == torch.bfloat16
    wd = dbuf(n)
    accd = to_dev(acc)
    m.fedavg_apply_delta(wd.data_ptr(), gd.data_ptr(), accd.data_ptr(), n, _s())
    torch.cuda.synchronize()
    ref = g.astype(float) + sum(float(F32(si)) * (w.astype(float) - g.astype(float)) for w, si in zip(ws, s))
    U = max(np.abs(w.astype(float) - g.astype(float)).max() for w in ws)
    tol = K * 2.0 ** -9 * U * (1 + 2.0 ** -7) + 4 * 2.0 ** -24 * np.abs(ref).max()
    err = np.abs(gd.cpu().numpy().astype(float) - ref).max()
    print(f"fedavg round trip: err {err:.3e} bound {tol:.3e} U {U:.3e} max|g| {np.abs(g).max():.2f}")
    assert err <= tol and tol < 1e-2 * 2.0 ** -9 * np.abs(g).max()
    assert torch.equal(wd, gd)


# ----------------------------------------------------------------------------- confusion counts
def _logits_with_ties(rng, M, C):
    return rng.randint(0, 3, (M, C)).astype(F32)       # three distinct values: ties in most rows


@pytest.mark.parametrize("C", [1, 2, 3, 16])
def test_logits_confusion_counts(m, C):
    """cm[y][argmax z] += 1 with the first maximum on ties, exact, accumulated over two calls."""
    rng = np.random.RandomState(C)
    ldz = C + 3
    for M in (1, 255, 256, 257):
        z, y = _logits_with_ties(rng, M, C), rng.randint(0, C, M).astype(np.int32)
        zd, yd = put2d(z, ldz, fill=1e30), to_dev(y)
        cm = dbuf(C * C + TAIL, fill=0.0)
        cm[C * C:] = SENT
        before = bits(cm)
        for _ in range(2):
            m.logits_confusion(zd.data_ptr(), ldz, yd.data_ptr(), M, C, cm.data_ptr(), _s())
        assert_untouched(cm, before, region(C * C + TAIL, 0, 1, C * C, C * C), "logits_confusion")
        want = 2 * lo.confusion(np.argmax(z, axis=1), y, C)
        np.testing.assert_array_equal(cm[:C * C].cpu().numpy().reshape(C, C), want, err_msg=f"M={M}")


@pytest.mark.parametrize("C", [1, 2, 3, 16])
def test_logits_confusion_grid_stride(m, C):
    """One row more than 1024 blocks x 256 threads: the grid-stride loop takes a second trip
    (C = 16 is the one case of this module above a few MB: 17 MB of logits)."""
    rng = np.random.RandomState(5)
    M, ldz = 262145, C + 1
    z, y = _logits_with_ties(rng, M, C), rng.randint(0, C, M).astype(np.int32)
    zd, yd = put2d(z, ldz, fill=1e30), to_dev(y)
    cm = dbuf(C * C, fill=0.0)
    m.logits_confusion(zd.data_ptr(), ldz, yd.data_ptr(), M, C, cm.data_ptr(), _s())
    got = cm.cpu().numpy().reshape(C, C)
    np.testing.assert_array_equal(got, lo.confusion(np.argmax(z, axis=1), y, C))
    assert got.sum() == M


def test_logits_confusion_rejects_more_than_16_classes(m):
    z, y, cm = dbuf(64, fill=0.0), dbuf(4, torch.int32, 0), dbuf(17 * 17, fill=0.0)
    with pytest.raises(RuntimeError):
        m.logits_confusion(z.data_ptr(), 17, y.data_ptr(), 1, 17, cm.data_ptr(), _s())
    torch.cuda.synchronize()


def test_confusion_of_packed_predictions(m):
    """cm[t][y[idx[i]]][pred[t][i]] += 1 for T = 3 trials through a row indirection."""
    rng = np.random.RandomState(6)
    T, M, C, nshard = 3, 257, 3, 400
    y = rng.randint(0, C, nshard).astype(np.int32)
    idx = rng.permutation(nshard)[:M].astype(np.int32)
    pred = rng.randint(0, C, (T, M)).astype(np.int32)
    cm = dbuf(T * C * C + TAIL, fill=0.0)
    cm[T * C * C:] = SENT
    before = bits(cm)
    predd, yd, idxd = to_dev(pred), to_dev(y), to_dev(idx)      # held: the launch is asynchronous
    m.confusion(predd.data_ptr(), yd.data_ptr(), idxd.data_ptr(), M, C, T, cm.data_ptr(), _s())
    assert_untouched(cm, before, region(T * C * C + TAIL, 0, 1, T * C * C, T * C * C), "confusion")
    got = cm[:T * C * C].cpu().numpy().reshape(T, C, C)
    for t in range(T):
        np.testing.assert_array_equal(got[t], lo.confusion(pred[t], y[idx], C))
    # identity rows when idx is null
    cm2 = dbuf(T * C * C, fill=0.0)
    m.confusion(predd.data_ptr(), yd.data_ptr(), 0, M, C, T, cm2.data_ptr(), _s())
    np.testing.assert_array_equal(cm2.cpu().numpy().reshape(T, C, C)[1], lo.confusion(pred[1], y[:M], C))


# ----------------------------------------------------------------------------- loss heads
def _ce_logits(rng, M, C):
    z = (rng.randn(M, C) * 3.0).astype(F32)
    y = rng.randint(0, C, M).astype(np.int32)
    special = [np.full(C, 1.25, dtype=F32),                       # all logits equal
               np.linspace(-5e3, 5e3, C).astype(F32),             # 1e4 spread: softmax is exactly 0 / 1
               np.linspace(2.0, -3.0, C).astype(F32)[::-1].copy()]
    for i, row in enumerate(special[:M] if M >= 3 else special[M - 1:M]):
        z[i] = row
    if M >= 3:
        y[1] = 0                                                  # the true class at the minimum logit
        y[2] = 0
    else:
        y[0] = int(np.argmin(z[0]))
    return z, y


def _ce_rowscale(z, y):
    z = z.astype(float)
    mx = z.max(1)
    return np.abs(mx) + np.abs(np.log(np.exp(z - mx[:, None]).sum(1))) + np.abs(z[np.arange(len(y)), y])


@pytest.mark.parametrize("C", [2, 3, 16])
def test_xent_softmax_head(m, C):
    """Mode 0 vs the float64 model for every M x scale: dz within 4x the fp32 transcription's
    error in units of `scale`; the double loss accumulator (two calls on a non-zero start) within
    the same per-row figure x sum of the rows' term magnitudes, plus eps64 x blocks x sum |loss|
    for the atomics; all-equal, saturated and true-class-at-minimum rows finite with sum_k dz = 0."""
    rng = np.random.RandomState(20 + C)
    ldz, lddz = C + 3, C + 2
    cases = []
    for M in (1, 255, 256, 257, 513):
        for scale in (1.0, 1.0 / M):
            scale = float(F32(scale))
            z, y = _ce_logits(rng, M, C)
            rows, dz, _ = lo.ce_head(z, y, scale)
            r32, d32 = lo.ce_head_f32(z, y, scale)
            cases.append(dict(M=M, scale=scale, z=z, y=y, rows=rows, dz=dz, e_dz=lo.nerr(d32, dz, scale),
                              e_row=lo.nerr(r32, rows, _ce_rowscale(z, y))))
    tb_dz, tb_row = lo.bound(max(c["e_dz"] for c in cases)), lo.bound(max(c["e_row"] for c in cases))
    for c in cases:
        M, scale, z, y = c["M"], c["scale"], c["z"], c["y"]
        zd, yd = put2d(z, ldz, fill=1e30), to_dev(y)
        dzb = dbuf(M * lddz + TAIL)
        acc = dbuf(2, torch.float64)
        acc[0] = 0.75
        b_dz, b_acc = bits(dzb), bits(acc)
        for _ in range(2):
            m.xent(zd.data_ptr(), ldz, yd.data_ptr(), M, C, 0, scale, dzb.data_ptr(), lddz, acc.data_ptr(), _s())
        assert_untouched(dzb, b_dz, region(M * lddz + TAIL, 0, M, lddz, C), "xent dz")
        assert_untouched(acc, b_acc, region(2, 0, 1, 1, 1), "xent loss_acc")
        got = dzb[:M * lddz].view(M, lddz)[:, :C].cpu().numpy()
        loss = float(acc[0].item())
        assert np.isfinite(got).all() and np.isfinite(loss)
        e = lo.nerr(got, c["dz"], scale)
        blocks = (M + 255) // 256
        want = 0.75 + 2.0 * c["rows"].sum()
        tol = 2.0 * tb_row * _ce_rowscale(z, y).sum() + EPS64 * (2 * blocks + 10) * (0.75 + 2 * np.abs(c["rows"]).sum())
        print(f"xent C={C} M={M} scale={scale:.3g}: dz err {e:.3e} bound {tb_dz:.3e}; "
              f"loss err {abs(loss - want):.3e} bound {tol:.3e}")
        assert e <= tb_dz
        assert abs(loss - want) <= tol
        assert np.abs(got.astype(float).sum(1)).max() <= C * tb_dz * scale


def test_xent_batched_trials(m):
    """T = 3 trials with trial strides, a label indirection and active = [1, 0, 1]: the active
    trials match the model (dz, loss, first-maximum argmax), the inactive one keeps every bit."""
    rng = np.random.RandomState(31)
    T, M, C, nshard = 3, 257, 3, 300
    ldz, lddz = C + 2, C + 1
    sZ, sDz = M * ldz + 5, M * lddz + 7
    yshard = rng.randint(0, C, nshard).astype(np.int32)
    idx = rng.permutation(nshard)[:M].astype(np.int32)
    scale = float(F32(1.0 / M))
    zs = [np.round(rng.randn(M, C) * 2.0, 1).astype(F32) for _ in range(T)]     # 0.1 grid: ties occur
    zb = dbuf(T * sZ + TAIL, fill=1e30)
    for t in range(T):
        zb[t * sZ:t * sZ + M * ldz].view(M, ldz)[:, :C] = to_dev(zs[t])
    dzb, pred, acc = dbuf(T * sDz + TAIL), dbuf(T * M + TAIL, torch.int32, -7), dbuf(T + 1, torch.float64)
    acc[:T] = to_dev(np.array([0.5, 1.5, 2.5]))
    active = to_dev(np.array([1, 0, 1], dtype=np.int32))
    b_dz, b_pred, b_acc = bits(dzb), bits(pred), bits(acc)
    yd, idxd = to_dev(yshard), to_dev(idx)
    m.xent_batched(zb.data_ptr(), ldz, sZ, yd.data_ptr(), idxd.data_ptr(), M, C, 0, scale,
                   dzb.data_ptr(), lddz, sDz, acc.data_ptr(), pred.data_ptr(), active.data_ptr(), T, _s())
    own_dz = region(T * sDz + TAIL, 0, M, lddz, C) | region(T * sDz + TAIL, 2 * sDz, M, lddz, C)
    own_pred = region(T * M + TAIL, 0, 1, M, M) | region(T * M + TAIL, 2 * M, 1, M, M)
    own_acc = np.array([True, False, True, False])
    assert_untouched(dzb, b_dz, own_dz, "xent_batched dz")
    assert_untouched(pred, b_pred, own_pred, "xent_batched pred")
    assert_untouched(acc, b_acc, own_acc, "xent_batched loss_acc")
    y = yshard[idx]
    ref = {t: lo.ce_head(zs[t], y, scale) for t in (0, 2)}
    tr = {t: lo.ce_head_f32(zs[t], y, scale) for t in (0, 2)}
    tb_dz = lo.bound(max(lo.nerr(tr[t][1], ref[t][1], scale) for t in (0, 2)))
    tb_row = lo.bound(max(lo.nerr(tr[t][0], ref[t][0], _ce_rowscale(zs[t], y)) for t in (0, 2)))
    assert any((np.sort(zs[t], 1)[:, -1] == np.sort(zs[t], 1)[:, -2]).any() for t in (0, 2))   # ties present
    for t in (0, 2):
        rows, dz, am = ref[t]
        got = dzb[t * sDz:t * sDz + M * lddz].view(M, lddz)[:, :C].cpu().numpy()
        assert lo.nerr(got, dz, scale) <= tb_dz
        np.testing.assert_array_equal(pred[t * M:(t + 1) * M].cpu().numpy(), am)
        start = [0.5, 1.5, 2.5][t]
        tol = tb_row * _ce_rowscale(zs[t], y).sum() + EPS64 * 12 * (start + np.abs(rows).sum())
        assert abs(acc[t].item() - (start + rows.sum())) <= tol


def test_xent_binary_head(m):
    """Mode 1 (one logit per row) at logits {0, +-1e-3, +-20, +-100} for both labels, one row per
    trial so that every row's loss is visible: the loss clips at -log(eps32), pred is p > 0.5, and
    dz uses the unclipped p.  57 logits drawn from [-8, 8] ride along so that the transcription's
    error is measured on more than the two inexact rows of the fixed set.  Bounds: 4x the fp32
    transcription's error, dz in units of `scale`, the loss in units of 1 + |loss|."""
    rng = np.random.RandomState(32)
    zs = np.concatenate([[0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0], rng.uniform(-8, 8, 57)]).astype(F32)
    T, scale, ldz, lddz = len(zs), 0.5, 2, 3
    cap = -np.log(lo.EPS32)
    for yv in (0, 1):
        y = np.full(T, yv)
        rows, dz, pr = lo.binary_head(zs, y, scale)
        r32, d32 = lo.binary_head_f32(zs, y, scale)
        tb_dz = lo.bound(lo.nerr(d32, dz, scale))
        tb_row = lo.bound(lo.nerr(r32, rows, 1.0 + np.abs(rows)))
        zb = put2d(zs[:, None], ldz, fill=1e30)
        dzb, pred, acc = dbuf(T * lddz + TAIL), dbuf(T + TAIL, torch.int32, -7), dbuf(T + 1, torch.float64, 0.0)
        acc[T] = SENT
        b_dz, b_pred, b_acc = bits(dzb), bits(pred), bits(acc)
        yd = to_dev(np.array([yv], dtype=np.int32))
        m.xent_batched(zb.data_ptr(), ldz, ldz, yd.data_ptr(), 0, 1, 1, 1, scale, dzb.data_ptr(), lddz, lddz,
                       acc.data_ptr(), pred.data_ptr(), 0, T, _s())
        assert_untouched(dzb, b_dz, region(T * lddz + TAIL, 0, T, lddz, 1), "xent mode 1 dz")
        assert_untouched(pred, b_pred, region(T + TAIL, 0, 1, T, T), "xent mode 1 pred")
        assert_untouched(acc, b_acc, region(T + 1, 0, 1, T, T), "xent mode 1 loss_acc")
        got_dz = dzb[:T * lddz].view(T, lddz)[:, 0].cpu().numpy()
        got_loss = acc[:T].cpu().numpy()
        assert np.isfinite(got_dz).all() and np.isfinite(got_loss).all()
        assert lo.nerr(got_dz, dz, scale) <= tb_dz
        assert lo.nerr(got_loss, rows, 1.0 + np.abs(rows)) <= tb_row
        np.testing.assert_array_equal(pred[:T].cpu().numpy(), pr)
        # the clip: the wrong-side saturated rows cost exactly -log(eps32), never more
        wrong = zs * (1 - 2 * yv) >= 20
        np.testing.assert_allclose(got_loss[wrong], cap, rtol=1e-15)
        assert got_loss.max() <= cap * (1 + 1e-15)
        # dz is not clipped: exactly -+scale / 0 on the saturated rows
        np.testing.assert_array_equal(got_dz[np.abs(zs) >= 100], ((zs[np.abs(zs) >= 100] > 0) - yv) * F32(scale))
    # the single-problem binding, M = 7 rows of one trial: the sum of the rows
    y = (np.arange(T) % 2).astype(np.int32)
    rows, dz, _ = lo.binary_head(zs, y, scale)
    r32, d32 = lo.binary_head_f32(zs, y, scale)
    dzb, acc = dbuf(T * lddz + TAIL), dbuf(1, torch.float64, 0.0)
    zb = put2d(zs[:, None], ldz, fill=1e30)
    yd = to_dev(y)
    m.xent(zb.data_ptr(), ldz, yd.data_ptr(), T, 1, 1, scale, dzb.data_ptr(), lddz, acc.data_ptr(), _s())
    assert lo.nerr(dzb[:T * lddz].view(T, lddz)[:, 0].cpu().numpy(), dz, scale) <= lo.bound(lo.nerr(d32, dz, scale))
    tol = lo.bound(lo.nerr(r32, rows, 1.0 + np.abs(rows))) * (1.0 + np.abs(rows)).sum() + EPS64 * 12 * rows.sum()
    assert abs(acc.item() - rows.sum()) <= tol


# ----------------------------------------------------------------------------- Adam
ADAM_N = (1, 1023, 1024, 1025, 4097)          # a block covers 4 x 256 elements
ADAM = dict(lr=0.004, beta1=0.9, beta2=0.999, eps=1e-8)


def _adam_state(rng, n):
    g = (10.0 ** rng.uniform(-8, 3, n) * rng.choice([-1.0, 1.0], n)).astype(F32)     # |g| from 1e-8 to 1e3
    p = rng.randn(n).astype(F32)
    m0 = (rng.randn(n) * np.abs(g)).astype(F32)
    v0 = (rng.rand(n) * g.astype(float) ** 2).astype(F32)
    z = rng.permutation(n)[:max(1, n // 8)] if n > 1 else np.array([], dtype=int)
    g[z], m0[z], v0[z] = 0.0, 0.0, 0.0                                                # g = 0 and v = 0 entries
    return p, m0, v0, g


def _adam_errs(got, ref, p0, m0, v0, geff):
    """(p, m, v) errors in units of |p0| + |update|, |m0| + |g| and v0 + g^2."""
    p, mm, v = ref[:3]
    return (lo.nerr(got[0], p, np.abs(p0) + np.abs(p - p0)), lo.nerr(got[1], mm, np.abs(m0) + np.abs(geff)),
            lo.nerr(got[2], v, v0.astype(float) + geff ** 2))


def _adam_bufs(n, T, p, m0, v0, g):
    out = []
    for a in (p, m0, v0):
        b = dbuf(T * n + TAIL)
        b[:T * n] = to_dev(np.ascontiguousarray(a).reshape(-1))
        out.append(b)
    gb = dbuf(T * n + TAIL, fill=1e30)
    gb[:T * n] = to_dev(np.ascontiguousarray(g).reshape(-1))
    return out + [gb]


@pytest.mark.parametrize("t", [1, 2, 1000, 10 ** 6])
def test_adam_flat_single_steps(m, t):
    """torch-style Adam, one step at t (t = 1: the largest bias correction; 10^6: beta2^t
    underflows to 0) for every n around the 1024-element block: p, m, v within 4x the fp32
    transcription's error, nothing written past n."""
    rng = np.random.RandomState(40)
    cases = []
    for n in ADAM_N:
        p, m0, v0, g = _adam_state(rng, n)
        ref = lo.adam_step(p, m0, v0, g, style=0, t=t, **ADAM)
        tr = lo.adam_step_f32(p, m0, v0, g, style=0, t=t, **ADAM)
        cases.append((n, p, m0, v0, g, ref, _adam_errs(tr, ref, p, m0, v0, g.astype(float))))
    tb = [lo.bound(max(c[-1][k] for c in cases)) for k in range(3)]
    for n, p, m0, v0, g, ref, _ in cases:
        pb, mb, vb, gb = _adam_bufs(n, 1, p, m0, v0, g)
        before = [bits(b) for b in (pb, mb, vb)]
        m.adam_flat(pb.data_ptr(), mb.data_ptr(), vb.data_ptr(), gb.data_ptr(), n, ADAM["lr"], ADAM["beta1"],
                    ADAM["beta2"], ADAM["eps"], t, _s())
        for b, b0 in zip((pb, mb, vb), before):
            assert_untouched(b, b0, region(n + TAIL, 0, 1, n, n), f"adam_flat n={n}")
        got = [b[:n].cpu().numpy() for b in (pb, mb, vb)]
        assert all(np.isfinite(a).all() for a in got)
        e = _adam_errs(got, ref, p, m0, v0, g.astype(float))
        print(f"adam_flat t={t} n={n}: err p/m/v {e[0]:.3e} {e[1]:.3e} {e[2]:.3e} bounds {tb[0]:.3e} {tb[1]:.3e} {tb[2]:.3e}")
        assert e[0] <= tb[0] and e[1] <= tb[1] and e[2] <= tb[2]


def test_adam_flat_fifty_steps(m):
    """50 steps from zero moments on a fixed gradient sequence vs 50 float64 steps; the errors
    are in units of |p0| + sum_t |update_t|, max_t |g_t| and max_t g_t^2."""
    rng = np.random.RandomState(41)
    n, steps = 1025, 50
    p0 = rng.randn(n).astype(F32)
    base = (10.0 ** rng.uniform(-4, 1, n)).astype(F32)
    gs = [(rng.randn(n) * base).astype(F32) for _ in range(steps)]
    ref, tr = (p0, np.zeros(n), np.zeros(n)), (p0, np.zeros(n, F32), np.zeros(n, F32))
    travel = np.abs(p0).astype(float)
    pb, mb, vb, gb = _adam_bufs(n, 1, p0, np.zeros(n, F32), np.zeros(n, F32), gs[0])
    before = [bits(b) for b in (pb, mb, vb)]
    for t, g in enumerate(gs, 1):
        new = lo.adam_step(*ref, g, style=0, t=t, **ADAM)[:3]
        travel += np.abs(new[0] - ref[0])
        ref = new
        tr = lo.adam_step_f32(*tr, g, style=0, t=t, **ADAM)
        gb[:n] = to_dev(g)
        m.adam_flat(pb.data_ptr(), mb.data_ptr(), vb.data_ptr(), gb.data_ptr(), n, ADAM["lr"], ADAM["beta1"],
                    ADAM["beta2"], ADAM["eps"], t, _s())
    for b, b0 in zip((pb, mb, vb), before):
        assert_untouched(b, b0, region(n + TAIL, 0, 1, n, n), "adam_flat 50 steps")
    gmax = np.max(np.abs(np.stack(gs)).astype(float), axis=0)
    scales = (travel, gmax, gmax ** 2)
    for name, buf, r, t32, sc in zip("pmv", (pb, mb, vb), ref, tr, scales):
        e, tb = lo.nerr(buf[:n].cpu().numpy(), r, sc), lo.bound(lo.nerr(t32, r, sc))
        print(f"adam_flat 50 steps {name}: err {e:.3e} bound {tb:.3e}")
        assert e <= tb


def test_adam_batched_sklearn_style(m):
    """Style 1 over T = 3 trials with their own lr and step, trial 1 inactive (every bit kept), a
    weight-decay mask of a prefix and a middle run, FedProx mu with anchor != p, the L2 loss term
    of the masked PRE-update weights, and the bf16 shadow of the kernel's own new p.  The L2 term
    is accumulated in double from exact fp32 squares: its bound is eps64 x (blocks + 16 in-block
    roundings) x the accumulator's magnitude."""
    rng = np.random.RandomState(42)
    T = 3
    lrs, steps, start = [0.001, 0.004, 0.02], [1, 7, 300], [1.5, 2.5, 3.5]
    wd, mu, l2 = 0.01, 0.1, 0.05
    kw = dict(style=1, beta1=0.9, beta2=0.999, eps=1e-8, wd=wd, mu=mu)
    cases = []
    for n in ADAM_N:
        st = [_adam_state(rng, n) for _ in range(T)]
        p, m0, v0, g = (np.stack([s[k] for s in st]) for k in range(4))
        anchor = (p + rng.randn(T, n).astype(F32) * F32(0.1)).astype(F32)
        mask = np.zeros(n, dtype=np.uint8)
        mask[:n // 5 + 1] = 1
        mask[n // 2:n // 2 + n // 7 + 1] = 1
        refs, errs = {}, []
        for t in (0, 2):
            geff = g[t].astype(float) + wd * mask * p[t].astype(float) + mu * (p[t].astype(float) - anchor[t])
            refs[t] = lo.adam_step(p[t], m0[t], v0[t], g[t], lr=lrs[t], t=steps[t], wd_mask=mask, anchor=anchor[t],
                                   l2_coef=l2, **kw)
            tr = lo.adam_step_f32(p[t], m0[t], v0[t], g[t], lr=lrs[t], t=steps[t], wd_mask=mask, anchor=anchor[t], **kw)
            errs.append(_adam_errs(tr, refs[t], p[t], m0[t], v0[t], geff))
            refs[t] = refs[t] + (geff,)
        cases.append((n, p, m0, v0, g, anchor, mask, refs, errs))
    tb = [lo.bound(max(e[k] for c in cases for e in c[-1])) for k in range(3)]
    for n, p, m0, v0, g, anchor, mask, refs, _ in cases:
        pb, mb, vb, gb = _adam_bufs(n, T, p, m0, v0, g)
        shadow = dbuf(T * n + TAIL, torch.bfloat16)
        acc = dbuf(T + 1, torch.float64)
        acc[:T] = to_dev(np.array(start))
        stepd = to_dev(np.array(steps, dtype=np.int64))
        lrd = to_dev(np.array(lrs, dtype=np.float64))
        active = to_dev(np.array([1, 0, 1], dtype=np.int32))
        before = [bits(b) for b in (pb, mb, vb, shadow, acc)]
        anchord, maskd = to_dev(anchor), to_dev(mask)
        m.adam_batched(pb.data_ptr(), mb.data_ptr(), vb.data_ptr(), gb.data_ptr(), anchord.data_ptr(),
                       maskd.data_ptr(), n, 1, lrd.data_ptr(), 0.9, 0.999, 1e-8, wd, mu, stepd.data_ptr(),
                       acc.data_ptr(), l2, active.data_ptr(), shadow.data_ptr(), T, _s())
        own = region(T * n + TAIL, 0, 1, n, n) | region(T * n + TAIL, 2 * n, 1, n, n)
        for b, b0 in zip((pb, mb, vb, shadow), before):
            assert_untouched(b, b0, own, f"adam_batched n={n}")
        assert_untouched(acc, before[4], np.array([True, False, True, False]), "adam_batched loss_acc")
        assert stepd.cpu().tolist() == steps                         # Adam reads the step, never writes it
        blocks = (n + 1023) // 1024
        for t in (0, 2):
            got = [b[t * n:(t + 1) * n].cpu().numpy() for b in (pb, mb, vb)]
            e = _adam_errs(got, refs[t], p[t], m0[t], v0[t], refs[t][4])
            print(f"adam_batched n={n} trial {t}: err p/m/v {e[0]:.3e} {e[1]:.3e} {e[2]:.3e} "
                  f"bounds {tb[0]:.3e} {tb[1]:.3e} {tb[2]:.3e}")
            assert e[0] <= tb[0] and e[1] <= tb[1] and e[2] <= tb[2]
            want = start[t] + refs[t][3]
            assert abs(acc[t].item() - want) <= EPS64 * (blocks + 16) * want
            np.testing.assert_array_equal(bits(shadow)[t * n:(t + 1) * n], cpu_bf16_bits(torch.from_numpy(got[0])))


# ----------------------------------------------------------------------------- GEMM
GEMM_SHAPES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 63, 33), (130, 70, 300)]
LAYOUTS = [(1, 1), (1, 0), (0, 0), (0, 1)]


def _operands(rng, M, N, K, dtype, akc, bkc, pad):
    """Logical A [M][K], B [K][N] (bf16-rounded for dtype 1) and their device buffers in the asked
    storage order with leading dimension width + pad (pads hold NaN)."""
    A, B = rng.randn(M, K).astype(F32), rng.randn(K, N).astype(F32)
    if dtype:
        A, B = lo.bf16_round(A), lo.bf16_round(B)
    tdt = torch.bfloat16 if dtype else torch.float32
    As = A if akc else np.ascontiguousarray(A.T)
    Bs = np.ascontiguousarray(B.T) if bkc else B
    lda, ldb = As.shape[1] + pad, Bs.shape[1] + pad
    return A, B, put2d(As, lda, tdt), lda, put2d(Bs, ldb, tdt), ldb


def _gemm_models(A, B, epi, alpha, beta, bias, mask, C0):
    """(float64 model, float32 transcription in the epilogue's order, per-element term magnitudes)."""
    A64, B64 = A.astype(float), B.astype(float)
    ref = alpha * (A64 @ B64)
    tr = lo.matmul_f32(A, B) * F32(alpha)
    scale = abs(alpha) * (np.abs(A64) @ np.abs(B64))
    if epi in (1, 2):
        ref, tr, scale = ref + bias.astype(float), tr + bias, scale + np.abs(bias).astype(float)
    if epi == 2:
        ref, tr = np.maximum(ref, 0.0), np.maximum(tr, F32(0.0))
    if epi == 3:
        ref, tr = np.where(mask > 0, ref, 0.0), np.where(mask > 0, tr, F32(0.0))
    if beta != 0.0:
        ref, tr, scale = ref + beta * C0.astype(float), tr + F32(beta) * C0, scale + np.abs(beta * C0.astype(float))
    return ref, tr, scale


def gemm_case(m, rng, M, N, K, dtype, akc, bkc, epi=0, alpha=1.0, beta=0.0, pad=0, cbf16=False, mask_bf16=0,
              splits=1):
    """Run one single-problem GEMM; checks the guards and the bf16 copy; returns (kernel error,
    transcription error), both against the float64 product of the operands as cast."""
    A, B, Ad, lda, Bd, ldb = _operands(rng, M, N, K, dtype, akc, bkc, pad)
    ldc = ldmask = N + pad
    bias = rng.randn(N).astype(F32)
    mask = rng.randn(M, N).astype(F32)
    if mask_bf16:
        mask = lo.bf16_round(mask)
    C0 = rng.randn(M, N).astype(F32)
    ref, tr, scale = _gemm_models(A, B, epi, alpha, beta, bias, mask, C0)
    Cd = put2d(C0, ldc, fill=SENT) if beta != 0.0 else dbuf(M * ldc + TAIL)
    Cb = dbuf(M * ldc + TAIL, torch.bfloat16) if cbf16 else None
    maskd = put2d(mask, ldmask, torch.bfloat16 if mask_bf16 else torch.float32)
    slab = dbuf(splits * M * ldc + TAIL, fill=float("nan")) if splits > 1 else None
    b_c, b_cb = bits(Cd), (bits(Cb) if cbf16 else None)
    biasd = to_dev(bias)
    m.gemm(M, N, K, Ad.data_ptr(), lda, akc, Bd.data_ptr(), ldb, bkc, Cd.data_ptr(), ldc, epi, biasd.data_ptr(),
           maskd.data_ptr(), ldmask, mask_bf16, alpha, beta, dtype, splits, slab.data_ptr() if splits > 1 else 0,
           Cb.data_ptr() if cbf16 else 0, _s())
    own = region(M * ldc + TAIL, 0, M, ldc, N)
    assert_untouched(Cd, b_c, own, "gemm C")
    got = Cd[:M * ldc].view(M, ldc)[:, :N].cpu().numpy()
    assert np.isfinite(got).all()
    if cbf16:
        assert_untouched(Cb, b_cb, own, "gemm Cbf16")
        gb = np.ascontiguousarray(bits(Cb)[:M * ldc].reshape(M, ldc)[:, :N])
        np.testing.assert_array_equal(gb, cpu_bf16_bits(torch.from_numpy(got.copy())))
    if splits > 1:
        sl = slab[:splits * M * ldc].view(splits, M, ldc).cpu().numpy()
        assert np.isfinite(sl[:, :, :N]).all()                       # every slab written, empty k-ranges too
        BK = 32 if dtype else 16
        kper = -(-K // (splits * BK)) * BK
        for z in range(splits):
            if z * kper >= K:
                assert (sl[z, :, :N] == 0).all()
        assert np.isnan(bits_f32(slab)[splits * M * ldc:]).all()
    return lo.nerr(got, ref, scale), lo.nerr(tr, ref, scale)


def bits_f32(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _check(errs, what):
    tb = lo.bound(max(e[2] for e in errs))
    for name, ek, et in errs:
        print(f"{what} {name}: err {ek:.3e} (transcription {et:.3e}) bound {tb:.3e}")
    worst = max(errs, key=lambda e: e[1])
    assert worst[1] <= tb, f"{what} {worst[0]}: {worst[1]:.3e} > {tb:.3e}"


@pytest.mark.parametrize("dtype", [0, 1])
def test_gemm_shapes_layouts_epilogues(m, dtype):
    """Every shape (one element; one short of / exactly / one past the 64x64 tile with K below, at
    and past BK; several tiles) x the four operand layouts x the four epilogues.  Bound: 4x the
    error of a k-ordered fp32 accumulation with the epilogue in the kernel's order, relative to
    sum_k |a||b| (+ |bias|), over all of the test's cases."""
    rng = np.random.RandomState(50 + dtype)
    errs = []
    for (M, N, K) in GEMM_SHAPES:
        for akc, bkc in LAYOUTS:
            for epi in (0, 1, 2, 3):
                if epi == 3 and not akc:
                    continue                                           # the dgrad form reads A k-contiguous
                errs.append((f"{M}x{N}x{K} akc={akc} bkc={bkc} epi={epi}",
                             *gemm_case(m, rng, M, N, K, dtype, akc, bkc, epi=epi)))
    _check(errs, f"gemm dtype={dtype}")


@pytest.mark.parametrize("dtype", [0, 1])
def test_gemm_alpha_beta_bf16_copy_mask_and_leading_dimensions(m, dtype):
    """alpha = 0.5; beta = 1 on a random C; the bf16 copy bit-equal to bf16 of the fp32 output;
    a bf16 mask; every leading dimension = width + 3 (pads NaN on the inputs, sentinel on C)."""
    rng = np.random.RandomState(60 + dtype)
    errs = []
    for (M, N, K) in GEMM_SHAPES:
        for name, kw in (("alpha", dict(alpha=0.5)), ("beta", dict(beta=1.0)), ("alpha+beta+bias", dict(alpha=0.5, beta=1.0, epi=1)),
                         ("Cbf16", dict(cbf16=True, epi=2)), ("mask_bf16", dict(epi=3, mask_bf16=1)),
                         ("all", dict(alpha=0.5, beta=1.0, epi=3, mask_bf16=1, cbf16=True, pad=3))):
            errs.append((f"{M}x{N}x{K} {name}", *gemm_case(m, rng, M, N, K, dtype, 1, 0, **kw)))
        for akc, bkc in LAYOUTS:
            errs.append((f"{M}x{N}x{K} ld+3 akc={akc} bkc={bkc}",
                         *gemm_case(m, rng, M, N, K, dtype, akc, bkc, pad=3, epi=1, cbf16=True)))
    _check(errs, f"gemm options dtype={dtype}")


@pytest.mark.parametrize("dtype", [0, 1])
def test_gemm_split_k(m, dtype):
    """Split-K into slabs + the fixed-order reduce, splits in {2, 4} at K in {40, 300}; K = 40 in 4
    splits leaves empty k-ranges whose slabs must be zeros (the slabs start as NaN); beta = 0.5
    on the reduce.  The slabs are [splits][M][ldc] with ldc = N, as the callers use them."""
    rng = np.random.RandomState(70 + dtype)
    errs = []
    for K in (40, 300):
        for splits in (2, 4):
            for beta in (0.0, 0.5):
                for akc, bkc in ((0, 0), (1, 1)):
                    errs.append((f"K={K} splits={splits} beta={beta} akc={akc}",
                                 *gemm_case(m, rng, 65, 63, K, dtype, akc, bkc, beta=beta, splits=splits)))
    _check(errs, f"gemm split-K dtype={dtype}")


def test_gemm_split_k_rejects_epilogue_and_bf16_copy(m):
    M = N = K = 64
    A, B, C = dbuf(M * K, fill=1.0), dbuf(K * N, fill=1.0), dbuf(M * N)
    slab, bias, Cb = dbuf(2 * M * N), dbuf(N, fill=0.0), dbuf(M * N, torch.bfloat16)
    with pytest.raises(RuntimeError):
        m.gemm(M, N, K, A.data_ptr(), K, 1, B.data_ptr(), K, 1, C.data_ptr(), N, 1, bias.data_ptr(), 0, 0, 0, 1.0, 0.0,
               0, 2, slab.data_ptr(), 0, _s())
    with pytest.raises(RuntimeError):
        m.gemm(M, N, K, A.data_ptr(), K, 1, B.data_ptr(), K, 1, C.data_ptr(), N, 0, 0, 0, 0, 0, 1.0, 0.0, 0, 2,
               slab.data_ptr(), Cb.data_ptr(), _s())
    torch.cuda.synchronize()
    assert (bits(C) == bits(dbuf(M * N))).all()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("form", ["forward", "dgrad"])
def test_gemm_batched_problems(m, dtype, form):
    """The packed trainer's form: blockIdx.z = problem, A shared by all (sA = 0), per-problem B,
    C, bias and mask; problem 1 inactive, its C untouched.  forward: bias + ReLU, W k-contiguous;
    dgrad: ReLU mask, W n-contiguous."""
    rng = np.random.RandomState(80 + dtype)
    T, M, N, K, pad = 3, 65, 70, 33, 3
    akc, bkc, epi = (1, 1, 2) if form == "forward" else (1, 0, 3)
    tdt = torch.bfloat16 if dtype else torch.float32
    rnd = lo.bf16_round if dtype else (lambda a: a)
    A = rnd(rng.randn(M, K).astype(F32))
    Bs = [rnd(rng.randn(K, N).astype(F32)) for _ in range(T)]
    biases = rng.randn(T, N).astype(F32)
    masks = rng.randn(T, M, N).astype(F32)
    lda, ldc, ldmask = K + pad, N + pad, N + pad
    ldb = (K if bkc else N) + pad
    brows = N if bkc else K
    sB, sC, sBias, sMask = brows * ldb + 5, M * ldc + 7, N + 3, M * ldmask + 9
    Ad = put2d(A, lda, tdt)
    Bd = dbuf(T * sB + TAIL, tdt, float("nan"))
    maskd = dbuf(T * sMask + TAIL, fill=float("nan"))
    biasd = dbuf(T * sBias + TAIL, fill=float("nan"))
    for t in range(T):
        st = np.ascontiguousarray(Bs[t].T) if bkc else Bs[t]
        Bd[t * sB:t * sB + brows * ldb].view(brows, ldb)[:, :st.shape[1]] = to_dev(st).to(tdt)
        maskd[t * sMask:t * sMask + M * ldmask].view(M, ldmask)[:, :N] = to_dev(masks[t])
        biasd[t * sBias:t * sBias + N] = to_dev(biases[t])
    Cd = dbuf(T * sC + TAIL)
    active = to_dev(np.array([1, 0, 1], dtype=np.int32))
    before = bits(Cd)
    m.gemm(M, N, K, Ad.data_ptr(), lda, akc, Bd.data_ptr(), ldb, bkc, Cd.data_ptr(), ldc, epi, biasd.data_ptr(),
           maskd.data_ptr(), ldmask, 0, 1.0, 0.0, dtype, 1, 0, 0, _s(), batch=T, sA=0, sB=sB, sC=sC, sBias=sBias,
           sMask=sMask, active=active.data_ptr())
    own = region(T * sC + TAIL, 0, M, ldc, N) | region(T * sC + TAIL, 2 * sC, M, ldc, N)
    assert_untouched(Cd, before, own, "batched gemm C")
    errs = []
    for t in (0, 2):
        ref, tr, scale = _gemm_models(A, Bs[t], epi, 1.0, 0.0, biases[t], masks[t], None)
        got = Cd[t * sC:t * sC + M * ldc].view(M, ldc)[:, :N].cpu().numpy()
        errs.append((f"problem {t}", lo.nerr(got, ref, scale), lo.nerr(tr, ref, scale)))
    _check(errs, f"batched gemm {form} dtype={dtype}")


# ----------------------------------------------------------------------------- colsum
def _colsum_case(m, rng, M, N, ld, beta):
    X = (rng.randn(M, N) * 10.0 ** rng.randint(-2, 3, (1, N))).astype(F32)
    o0 = rng.randn(N).astype(F32)
    ref = beta * o0.astype(float) + X.astype(float).sum(0)
    scale = np.abs(beta * o0.astype(float)) + np.abs(X).astype(float).sum(0)
    acc = lo.sum_f32(X, 0)
    tr = F32(beta) * o0 + acc if beta != 0.0 else acc
    Xd = put2d(X, ld, fill=1e30)
    out = dbuf(N + TAIL)
    out[:N] = to_dev(o0)
    before = bits(out)
    m.colsum(Xd.data_ptr(), M, N, ld, out.data_ptr(), beta, _s())
    assert_untouched(out, before, region(N + TAIL, 0, 1, N, N), "colsum")
    return lo.nerr(out[:N].cpu().numpy(), ref, scale), lo.nerr(tr, ref, scale)


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
def test_colsum_padded_rows_and_flat_switch(m, beta):
    """out[n] = beta*out[n] + sum_m X[m][n].  ld > N as the trainer calls it (ld = maxw), with
    fewer / exactly / more rows than the 16 row-splitting waves and N around one 64-column block;
    then ld = N with M * N on both sides of the 4096 switch to the flat kernel, at N that do not
    divide 1024.  Bound: 4x a sequential fp32 column sum's error relative to sum |terms|."""
    rng = np.random.RandomState(90)
    errs = []
    for M in (1, 15, 16, 17):
        for N in (1, 64, 65):
            errs.append((f"M={M} N={N} ld={N + 3}", *_colsum_case(m, rng, M, N, N + 3, beta)))
    for N in (3, 14):
        lo_m = 4095 // N
        assert lo_m * N < 4096 <= (lo_m + 1) * N
        for M in (lo_m, lo_m + 1):
            errs.append((f"M={M} N={N} flat-switch", *_colsum_case(m, rng, M, N, N, beta)))
    _check(errs, f"colsum beta={beta}")


def test_colsum_batched_with_inactive_problem(m):
    rng = np.random.RandomState(91)
    T, M, N, ld = 3, 17, 65, 70
    sX, sOut = M * ld + 5, N + 3
    Xs = rng.randn(T, M, N).astype(F32)
    Xd = dbuf(T * sX + TAIL, fill=1e30)
    for t in range(T):
        Xd[t * sX:t * sX + M * ld].view(M, ld)[:, :N] = to_dev(Xs[t])
    out = dbuf(T * sOut + TAIL)
    before = bits(out)
    active = to_dev(np.array([1, 0, 1], dtype=np.int32))
    m.colsum(Xd.data_ptr(), M, N, ld, out.data_ptr(), 0.0, _s(), batch=T, sX=sX, sOut=sOut, active=active.data_ptr())
    assert_untouched(out, before, region(T * sOut + TAIL, 0, 1, N, N) | region(T * sOut + TAIL, 2 * sOut, 1, N, N),
                     "batched colsum")
    errs = []
    for t in (0, 2):
        ref, scale = Xs[t].astype(float).sum(0), np.abs(Xs[t]).astype(float).sum(0)
        errs.append((f"problem {t}", lo.nerr(out[t * sOut:t * sOut + N].cpu().numpy(), ref, scale),
                     lo.nerr(lo.sum_f32(Xs[t], 0), ref, scale)))
    _check(errs, "batched colsum")


# ----------------------------------------------------------------------------- minibatch plumbing
@pytest.mark.parametrize("epoch", [0, 2])
def test_gather_rows(m, epoch):
    """Rows perms[epoch_ctr][off : off + M] -> out[i][:F] (zero padded to ldo), the bf16 copy and
    the labels, exactly; identity order when perms is null."""
    rng = np.random.RandomState(100)
    n, F, ld, ldo, off, M = 40, 6, 8, 9, 5, 7
    X = special_values(rng, n * F).reshape(n, F)
    X[np.isnan(X)] = 3.0
    y = rng.randint(0, 4, n).astype(np.int32)
    perms = np.stack([rng.permutation(n) for _ in range(3)]).astype(np.int32)
    Xd, yd, pd = put2d(X, ld, fill=1e30), to_dev(y), to_dev(perms)
    ctr = to_dev(np.array([epoch], dtype=np.int32))
    for use_perms in (True, False):
        out, outb, yb = dbuf(M * ldo + TAIL), dbuf(M * ldo + TAIL, torch.bfloat16), dbuf(M + TAIL, torch.int32, -7)
        before = [bits(b) for b in (out, outb, yb)]
        m.gather_rows(Xd.data_ptr(), ld, yd.data_ptr(), pd.data_ptr() if use_perms else 0,
                      ctr.data_ptr() if use_perms else 0, n, off, M, F, out.data_ptr(), ldo, outb.data_ptr(),
                      yb.data_ptr(), _s())
        assert_untouched(out, before[0], region(M * ldo + TAIL, 0, M, ldo, ldo), "gather out")
        assert_untouched(outb, before[1], region(M * ldo + TAIL, 0, M, ldo, ldo), "gather outb")
        assert_untouched(yb, before[2], region(M + TAIL, 0, 1, M, M), "gather yb")
        want, wy = lo.gather_rows(X, y, perms if use_perms else None, epoch, off, M, F, ldo)
        np.testing.assert_array_equal(bits(out)[:M * ldo].reshape(M, ldo), want.view(np.int32))
        np.testing.assert_array_equal(bits(outb)[:M * ldo].reshape(M, ldo),
                                      cpu_bf16_bits(torch.from_numpy(want.copy())))
        np.testing.assert_array_equal(yb[:M].cpu().numpy(), wy)
        assert ctr.item() == epoch                                     # read, never written


@pytest.mark.parametrize("T", [1, 64, 65, 200])
def test_step_count_covers_every_trial(m, T):
    """step[t] += 1 for every active trial, for any number of packed trials (more than one
    64-thread block included); an inactive trial and the elements past T keep their values."""
    rng = np.random.RandomState(T)
    step0 = rng.randint(0, 1000, T).astype(np.int64)
    active = np.ones(T, dtype=np.int32)
    if T > 1:
        active[T // 2] = 0
    step = dbuf(T + TAIL, torch.int64, -7)
    step[:T] = to_dev(step0)
    before = bits(step)
    actived = to_dev(active)
    m.step_count(step.data_ptr(), actived.data_ptr(), T, _s())
    assert_untouched(step, before, region(T + TAIL, 0, 1, T, T), "step_count")
    np.testing.assert_array_equal(step[:T].cpu().numpy(), step0 + active)
    m.step_count(step.data_ptr(), 0, T, _s())                          # no flags: every trial
    np.testing.assert_array_equal(step[:T].cpu().numpy(), step0 + active + 1)


def _loss_scripts(T, calls, rng):
    """Per-trial mean-loss sequences, by t % 6: steady improvement (runs to max_iter); improvement
    then a plateau inside tol (tol stop); a plateau of n_iter_no_change epochs, a fresh improvement
    (reset), a plateau again; rising losses (earliest tol stop); noise; a slow descent whose steps
    are smaller than tol (non-improvements although the best keeps falling)."""
    out = np.empty((T, calls))
    e = np.arange(calls)
    for t in range(T):
        k = t % 6
        if k == 0:
            s = 2.0 - 0.1 * e
        elif k == 1:
            s = np.where(e < 3, 1.0 - 0.2 * e, 0.6 - 1e-3 * (e - 2))
        elif k == 2:
            s = np.where(e < 2, 1.0 - 0.3 * e, np.where(e < 4, 0.7 - 1e-4 * e, 0.3 + 1e-4 * e))
        elif k == 3:
            s = 0.5 + 0.05 * e
        elif k == 4:
            s = 1.0 + 0.3 * rng.rand(calls)
        else:
            s = 1.0 - 2e-3 * e
        out[t] = s + 1e-3 * (t // 6)
    return out


@pytest.mark.parametrize("tol_stop", [1, 0])
def test_epoch_end_rule(m, tol_stop):
    """T = 70 trials x 15 epoch ends against the float64 rule, everything compared exactly after
    every call: the curve, best, count, n_iter, active, the accumulator's reset (a stopped trial's
    accumulator is left alone) and ONE increment of the epoch counter per launch."""
    rng = np.random.RandomState(110)
    T, calls, n, tol, nic, max_iter = 70, 15, 100, 1e-2, 2, 12
    scripts = _loss_scripts(T, calls, rng)
    models = [lo.EpochEnd(n, tol, nic, max_iter, tol_stop) for _ in range(T)]
    G = 3
    ctr = dbuf(1 + G, torch.int32, 0)
    ctr[1:] = -7
    acc, best = dbuf(T + G, torch.float64), dbuf(T + G, torch.float64)
    best[:T] = float("inf")
    count, n_iter, active = dbuf(T + G, torch.int32, -7), dbuf(T + G, torch.int32, -7), dbuf(T + G, torch.int32, -7)
    count[:T], n_iter[:T], active[:T] = 0, 0, 1
    curve = dbuf(T * max_iter + G, torch.float64)
    before = {k: bits(b) for k, b in dict(ctr=ctr, acc=acc, best=best, count=count, n_iter=n_iter, active=active,
                                          curve=curve).items()}
    seen = set()
    for c in range(calls):
        sums = scripts[:, c] * n
        acc[:T] = to_dev(sums)
        m.epoch_end(T, ctr.data_ptr(), acc.data_ptr(), best.data_ptr(), count.data_ptr(), n_iter.data_ptr(),
                    active.data_ptr(), curve.data_ptr(), n, tol, nic, max_iter, tol_stop, _s())
        was_active = [mo.active for mo in models]
        want_acc = np.array([mo.update(a) for mo, a in zip(models, sums)])
        assert ctr[0].item() == c + 1, f"call {c}: epoch_ctr {ctr[0].item()}"
        got = {k: v[:T].cpu().numpy() for k, v in dict(acc=acc, best=best, count=count, n_iter=n_iter,
                                                       active=active).items()}
        np.testing.assert_array_equal(got["acc"], want_acc, err_msg=f"call {c} loss_acc")
        np.testing.assert_array_equal(got["best"], [mo.best for mo in models], err_msg=f"call {c} best")
        np.testing.assert_array_equal(got["count"], [mo.count for mo in models], err_msg=f"call {c} count")
        np.testing.assert_array_equal(got["n_iter"], [mo.n_iter for mo in models], err_msg=f"call {c} n_iter")
        np.testing.assert_array_equal(got["active"], [mo.active for mo in models], err_msg=f"call {c} active")
        cv = curve[:T * max_iter].view(T, max_iter).cpu().numpy()
        for t, mo in enumerate(models):
            np.testing.assert_array_equal(cv[t, :len(mo.curve)], mo.curve, err_msg=f"call {c} curve of trial {t}")
            assert (cv[t, len(mo.curve):] == SENT).all()
            if was_active[t]:
                seen.add("improved" if mo.count == 0 else "stalled")
                if not mo.active:
                    seen.add("max_iter" if mo.n_iter >= max_iter else "tol")
    # the scripts reached every branch of the rule, for trials past the first 64 too
    assert {"improved", "stalled", "max_iter"} <= seen and (("tol" in seen) == bool(tol_stop))
    stops = {mo.n_iter for mo in models[64:]}
    assert (len(stops) > 1) == bool(tol_stop) and all(not mo.active for mo in models)
    for k, b in dict(ctr=ctr, acc=acc, best=best, count=count, n_iter=n_iter, active=active).items():
        tot = (1 if k == "ctr" else T) + G
        assert_untouched(b, before[k], region(tot, 0, 1, tot - G, tot - G), f"epoch_end {k}")
    assert_untouched(curve, before["curve"], region(T * max_iter + G, 0, 1, T * max_iter, T * max_iter), "curve")

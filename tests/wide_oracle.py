"""Float64 models of the wide-MLP path: the bf16 NT GEMM of gemm_nt_bf16.hip with its fused
epilogue, its column-sum epilogue, the skinny weight gradient, the split column sums, and the
stages of one ``WideClient`` micro-batch (fedmi/fl/wide.py), each stage a function of that stage's
own inputs.  Plain numpy, no GPU import.  ``test_wide_oracle_cpu.py`` pins the models to torch
float64; the ``test_wide_*`` GPU files compare the kernels with them.

As in ``layered_oracle``, every model comes with a float32 TRANSCRIPTION in the kernel's operation
order.  A transcription is not a reference: its distance from the float64 model on a test's own
inputs (``lo.nerr``) is what a correct fp32 implementation shows there, and the kernel is allowed
``lo.bound`` of it.
"""
from __future__ import annotations

import numpy as np

from . import layered_oracle as lo

F32 = np.float32
F64 = np.float64


def _f(x) -> float:
    """A scalar as the kernels receive it: rounded to float32."""
    return float(F32(x))


def keep_of(mask) -> np.ndarray:
    """The NT epilogue's mask rule ``mask > 0 ? v : 0``: +0, -0, negatives and NaN drop."""
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, dtype=F32) > 0


# ----------------------------------------------------------------------------- NT GEMM
def nt_product(A, B):
    """The epilogue-independent part of nt_gemm, to be shared by the epilogues of one operand pair:
    (A . B^T in float64, sum_k |a||b|, the k-ordered float32 accumulation)."""
    A32, B32 = np.asarray(A, dtype=F32), np.asarray(B, dtype=F32)
    return (A32.astype(F64) @ B32.astype(F64).T, np.abs(A32).astype(F64) @ np.abs(B32).astype(F64).T,
            lo.matmul_f32(A32, B32.T))


def nt_gemm(A, B, alpha=1.0, bias=None, relu=False, mask=None, beta=0.0, C0=None, prod=None, pre=False):
    """C = epilogue(alpha * A[M][K] . B[N][K]^T); epilogue order: alpha, + bias[n], ReLU,
    mask > 0 ? v : 0, + beta * C0.  -> (ref64, transcription32, scale) with
    scale = |alpha| sum_k |a||b| + |bias| + |beta C0| (a masked-out or ReLU-clamped element keeps
    the scale of its terms; where the model is 0 because of the mask the kernel must be 0 too).
    ``prod``: nt_product(A, B) computed earlier.  ``pre``: also return, fourth, the float64 value
    before the ReLU / mask step (what bf16_interval takes)."""
    p64, pabs, acc32 = nt_product(A, B) if prod is None else prod
    a, b = _f(alpha), _f(beta)
    ref = a * p64
    scale = abs(a) * pabs
    tr = acc32 * F32(alpha)
    if pre:
        before = ref + (0.0 if bias is None else np.asarray(bias, dtype=F32).astype(F64))
        return (*nt_gemm(A, B, alpha, bias, relu, mask, beta, C0, prod=(p64, pabs, acc32)), before)
    if bias is not None:
        bias = np.asarray(bias, dtype=F32)
        ref, tr, scale = ref + bias.astype(F64), tr + bias, scale + np.abs(bias).astype(F64)
    if relu:
        ref, tr = np.maximum(ref, 0.0), np.maximum(tr, F32(0))
    if mask is not None:
        keep = keep_of(mask)
        ref, tr = np.where(keep, ref, 0.0), np.where(keep, tr, F32(0))
    if b != 0.0:
        C0 = np.asarray(C0, dtype=F32)
        ref, tr, scale = ref + b * C0.astype(F64), tr + F32(beta) * C0, scale + np.abs(b * C0.astype(F64))
    return ref, tr.astype(F32), scale


def nt_csum(Cb):
    """Column sums of each 128-row group of a bf16 output [M][N] (M % 128 == 0), in float64
    -> (sums [M / 128][N], sum |terms| [M / 128][N])."""
    Cb = np.asarray(Cb, dtype=F64)
    g = Cb.reshape(Cb.shape[0] // 128, 128, Cb.shape[1])
    return g.sum(axis=1), np.abs(g).sum(axis=1)


def bf16_interval(ref, E, relu=False, keep=None):
    """What the bf16 image of a correct fp32 epilogue value can be.  ``ref`` is the float64 value
    BEFORE the ReLU / mask step f, E its per-element error allowance: rounding is monotone and so
    is f, so the result lies in [bf16(f(ref - E)), bf16(f(ref + E))] -> (lo, hi) as float32."""
    ref, E = np.asarray(ref, dtype=F64), np.asarray(E, dtype=F64)
    a, b = ref - E, ref + E
    if relu:
        a, b = np.maximum(a, 0.0), np.maximum(b, 0.0)
    if keep is not None:
        a, b = np.where(keep, a, 0.0), np.where(keep, b, 0.0)
    # float64 -> float32 is monotone as well, so rounding twice keeps the interval property
    return lo.bf16_round(a.astype(F32)), lo.bf16_round(b.astype(F32))


# ----------------------------------------------------------------------------- skinny kernels
def skinny_slab(W, S, C, rows, trans, splits, bias):
    """The transcription's partial sums [splits][(C + bias) * Nw] of skinny_wgrad: split z adds
    its rows' products to one fp32 accumulator per output, in row order (all splits step together
    here; rows past a split's range are zeros, and x + 0 is exact)."""
    W32 = np.asarray(W, dtype=F32)[:rows]
    S32 = np.asarray(S, dtype=F32)[:rows, :C]
    Nw = W32.shape[1]
    rc = -(-rows // splits)
    Wz, Sz = np.zeros((splits * rc, Nw), dtype=F32), np.zeros((splits * rc, C), dtype=F32)
    Wz[:rows], Sz[:rows] = W32, S32
    Wz, Sz = Wz.reshape(splits, rc, Nw), Sz.reshape(splits, rc, C)
    acc, bs = np.zeros((splits, C, Nw), dtype=F32), np.zeros((splits, Nw), dtype=F32)
    for i in range(rc):
        acc = acc + Sz[:, i, :, None] * Wz[:, i, None, :]
        bs = bs + Wz[:, i]
    slab = np.zeros((splits, (C + int(bias)) * Nw), dtype=F32)
    slab[:, :C * Nw] = (acc.transpose(0, 2, 1) if trans else acc).reshape(splits, C * Nw)
    if bias:
        slab[:, C * Nw:] = bs
    return slab


def skinny_wgrad(W, S, C, rows, trans, splits, beta, out0, bias0=None, slab=None):
    """out = beta * out0 + sum_r S[r][c] W[r][n] (trans = 0: out[c][n]; trans = 1: out[n][c]) and,
    with bias0, bias = beta * bias0 + sum_r W[r][n].  W [rows][Nw] and S [rows][>= C] hold bf16
    values.  -> dict with ``out`` / ``bias`` = (ref64, transcription32, scale) and ``slab``: the
    transcription's [splits][(C + b) * Nw] partial sums.

    Transcription: split z contracts rows [z * rc, min(rows, (z + 1) * rc)), rc = ceil(rows /
    splits), one accumulator per output, row by row (a product of two bf16 values is exact in
    fp32, so fma and multiply-add agree); the slabs are folded in order from 0 and beta * out is
    added last.  ``slab``: skinny_slab of the same arguments computed earlier (it does not depend on
    beta)."""
    W32 = np.asarray(W, dtype=F32)[:rows]
    S32 = np.asarray(S, dtype=F32)[:rows, :C]
    Nw = W32.shape[1]
    b = _f(beta)
    nb = 0 if bias0 is None else 1
    if slab is None:
        slab = skinny_slab(W32, S32, C, rows, trans, splits, bool(nb))
    fold = lo.sum_f32(slab, 0)

    def finish(ref, scale, s, o0):
        o0 = np.asarray(o0, dtype=F32).reshape(ref.shape)
        if b != 0.0:
            return (ref + b * o0.astype(F64), (F32(beta) * o0 + s.reshape(ref.shape)).astype(F32),
                    scale + np.abs(b * o0.astype(F64)))
        return ref, s.reshape(ref.shape).astype(F32), scale

    ref = S32.astype(F64).T @ W32.astype(F64)
    scale = np.abs(S32).astype(F64).T @ np.abs(W32).astype(F64)
    if trans:
        ref, scale = ref.T, scale.T
    res = {"out": finish(ref, scale, fold[:C * Nw], out0), "slab": slab, "bias": None}
    if nb:
        res["bias"] = finish(W32.astype(F64).sum(0), np.abs(W32).astype(F64).sum(0), fold[C * Nw:], bias0)
    return res


def colsum_slab(X, splits):
    """The transcription's partial sums of colsum_split -> (slab [eff][N], eff): block z owns the
    flat elements of rows [z * rc, min(M, (z + 1) * rc)), rc = ceil(M / splits), and
    eff = ceil(M / rc) blocks run; thread t < S = 1024 - 1024 % N adds elements t, t + S, ... in
    order; column n then adds the partial sums n, n + N, ... < S in order.  (All blocks step
    together here; the zeros that square the arrays off add exactly.)"""
    X32 = np.asarray(X, dtype=F32)
    M, N = X32.shape
    rc = -(-M // splits)
    eff = -(-M // rc)
    S = 1024 - 1024 % N
    chunks = -(-(rc * N) // S)
    flat = np.zeros((eff, chunks * S), dtype=F32)
    rows = np.zeros((eff * rc, N), dtype=F32)
    rows[:M] = X32
    flat[:, :rc * N] = rows.reshape(eff, rc * N)
    part = lo.sum_f32(flat.reshape(eff, chunks, S), 1)
    return lo.sum_f32(part.reshape(eff, S // N, N), 1), eff


def colsum_split(X, splits, beta, out0, slab=None):
    """out[n] = beta * out0[n] + sum_m X[m][n] for a dense fp32 [M][N], N <= 64.
    -> ((ref64, transcription32, scale), slab [eff][N], eff); the transcription folds
    colsum_slab's rows in order from 0 and adds beta * out last."""
    X32 = np.asarray(X, dtype=F32)
    b = _f(beta)
    slab, eff = colsum_slab(X32, splits) if slab is None else slab
    s = lo.sum_f32(slab, 0)
    ref, scale = X32.astype(F64).sum(0), np.abs(X32).astype(F64).sum(0)
    o0 = np.asarray(out0, dtype=F32)
    if b != 0.0:
        return (ref + b * o0.astype(F64), (F32(beta) * o0 + s).astype(F32), scale + np.abs(b * o0.astype(F64))), slab, eff
    return (ref, s, scale), slab, eff


# ----------------------------------------------------------------------------- WideClient stages
def stage_forward(inp, Wq, b):
    """Hidden layer before its rounding: relu(in . Wq^T + b); the layer's output is bf16 of it."""
    return nt_gemm(inp, Wq, 1.0, bias=b, relu=True)


def stage_logits(h, Wq, b):
    """fp32 logits h . Wq^T + b."""
    return nt_gemm(h, Wq, 1.0, bias=b)


def stage_head(z, y, n):
    """Softmax cross-entropy delta (p - onehot) / n -> (ref64, transcription32, scale = 1 / n:
    every term of p - onehot is at most 1 in magnitude)."""
    ref = lo.ce_head(z, y, 1.0 / n)[1]
    tr = lo.ce_head_f32(z, y, 1.0 / n)[1]
    return ref, tr, np.full(ref.shape, 1.0 / n)


def stage_pad_delta(dz, rp, width, rnd=lo.bf16_round):
    """The head delta as a GEMM operand: rnd(dz) in the first C columns of [rp][width], zeros in
    the pad columns and in the rows past the micro-batch's own."""
    dz = np.asarray(dz, dtype=F32)
    out = np.zeros((rp, width), dtype=F32)
    out[:dz.shape[0], :dz.shape[1]] = rnd(dz)
    return out


def stage_dgrad(dZ, Wq, act):
    """Delta of the layer below before its rounding: (dZ[rows][N] . Wq[N][K]) where act > 0."""
    return nt_gemm(dZ, np.asarray(Wq, dtype=F32).T, 1.0, mask=act)


def stage_wgrad(dZ, inp, beta, g0):
    """gW[N][K] = beta * g0 + dZ^T . in."""
    return nt_gemm(np.asarray(dZ, dtype=F32).T, np.asarray(inp, dtype=F32).T, 1.0, beta=beta, C0=g0)


def stage_bgrad(dZ, beta, g0):
    """gb[N] = beta * g0 + column sums of the delta AS STORED (the bf16 delta of a hidden layer,
    the fp32 dz_out of the head); transcription: a row-ordered fp32 sum."""
    d = np.asarray(dZ, dtype=F32)
    b = _f(beta)
    ref, scale, tr = d.astype(F64).sum(0), np.abs(d).astype(F64).sum(0), lo.sum_f32(d, 0)
    if b != 0.0:
        g0 = np.asarray(g0, dtype=F32)
        return ref + b * g0.astype(F64), (F32(beta) * g0 + tr).astype(F32), scale + np.abs(b * g0.astype(F64))
    return ref, tr, scale


def micro_batch(Ws, bs, x, y, n, beta, gW0, gb0, rnd=lo.bf16_round):
    """The stage models chained over one micro-batch, float64 throughout, every bf16 rounding the
    wide client performs replaced by ``rnd`` -> (gW list, gb list, logits).  With rnd = identity
    this is plain back-propagation of the mean cross-entropy (scale 1 / n), accumulated as
    beta * g0 + this micro-batch's share."""
    L = len(Ws)
    r64 = lambda v: np.asarray(rnd(v), dtype=F64)
    Wq = [r64(w) for w in Ws]
    acts = [r64(x)]
    for l in range(L - 1):
        acts.append(r64(np.maximum(acts[l] @ Wq[l].T + np.asarray(bs[l], dtype=F64), 0.0)))
    z = acts[-1] @ Wq[-1].T + np.asarray(bs[-1], dtype=F64)
    dz_out = lo.ce_head(z, y, 1.0 / n)[1]
    gW, gb = [None] * L, [None] * L
    gb[L - 1] = beta * np.asarray(gb0[L - 1], dtype=F64) + dz_out.sum(0)
    d = r64(dz_out)
    for l in range(L - 1, -1, -1):
        gW[l] = beta * np.asarray(gW0[l], dtype=F64) + d.T @ acts[l]
        if l < L - 1:
            gb[l] = beta * np.asarray(gb0[l], dtype=F64) + d.sum(0)
        if l > 0:
            d = r64(np.where(acts[l] > 0, d @ Wq[l], 0.0))
    return gW, gb, z


# ----------------------------------------------------------------------------- launch plan
def wide_plan(dims, mb, rows):
    """Which kernels one bf16 micro-batch of ``rows`` rows runs on, from the rules wide.py states:

    * the NT GEMM takes M % 128 == N % 128 == K % 64 == 0; transposed operands need mb % 128 == 0;
    * the K = 14 input and the C-class head delta are zero-padded to 64 (and the logits head to 256
      classes) when there are two or more layers, F <= 64, C <= 64 and mb, the first and the last
      hidden width are multiples of 128;
    * on that padded path a micro-batch of rows % 128 == 0 runs as it is; another one runs as
      rp = min(roundup(rows, 256 if mb % 256 == 0 else 128), mb) rows if EVERY hidden width is a
      multiple of 128, and otherwise on the generic path with no padding at all;
    * a dgrad emits column sums when it writes a transposed delta and rp and its width are
      multiples of 256;
    * the skinny kernels take layer 0's and the head's weight gradient for F = 14, C = 2, two or
      more layers and first / last hidden widths that are multiples of 8; layer 0's delta then has
      no transposed copy."""
    dims = [int(d) for d in dims]
    L = len(dims) - 1
    nt_ok = lambda M, N, K: M % 128 == 0 and N % 128 == 0 and K % 64 == 0
    t_ok = mb % 128 == 0
    padded = (t_ok and L >= 2 and dims[0] <= 64 and dims[-1] <= 64 and nt_ok(mb, dims[1], 64)
              and nt_ok(mb, dims[-2], 64))
    skinny = L >= 2 and dims[0] == 14 and dims[-1] == 2 and dims[1] % 8 == 0 and dims[-2] % 8 == 0
    rp = None
    if padded:
        if rows % 128 == 0:
            rp = rows
        elif all(d % 128 == 0 for d in dims[1:-1]):
            g = 256 if mb % 256 == 0 else 128
            rp = min(-(-rows // g) * g, mb)
    pad = rp is not None
    re = rp if pad else rows
    fwd = []
    for l in range(L):
        if (l == 0 or l == L - 1) and pad:
            fwd.append(True)
        elif l == L - 1:
            fwd.append(False)
        else:
            fwd.append(t_ok and nt_ok(re, dims[l + 1], dims[l]))
    # dgrad[l]: the GEMM producing the delta of hidden layer l (output of layer l), l = 0 .. L-2
    dgrad, csum, wgrad = [False] * max(L - 1, 0), [False] * max(L - 1, 0), [False] * L
    cs_ok = lambda n: L >= 2 and re % 256 == 0 and n % 256 == 0
    if L >= 2 and pad:
        dgrad[L - 2], csum[L - 2] = True, cs_ok(dims[L - 1])
    for l in range(L - 2, -1, -1):
        wgrad[l] = t_ok and l > 0 and nt_ok(dims[l + 1], dims[l], re)
        if l > 0 and t_ok and nt_ok(re, dims[l], dims[l + 1]):
            dgrad[l - 1] = True
            csum[l - 1] = not (l == 1 and skinny) and cs_ok(dims[l])
    # bias gradient of hidden layer l: skinny kernel / column sums of the dgrad / row sums / generic
    bias = []
    for l in range(L - 1):
        if l == 0 and skinny:
            bias.append("skinny")
        elif csum[l]:
            bias.append("csum")
        elif rows % 8 == 0:
            bias.append("rowsum")
        else:
            bias.append("colsum")
    return {"rp": rp, "rows_eff": re, "padded": padded, "skinny": skinny, "forward_nt": fwd, "dgrad_nt": dgrad,
            "csum": csum, "wgrad_nt": wgrad, "bias": bias, "nt_calls": sum(fwd) + sum(dgrad) + sum(wgrad)}

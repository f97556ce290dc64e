"""wide_oracle.py against independent implementations (no GPU): the chained stage models with the
bf16 rounding taken out are torch float64 autograd of the same MLP; nt_gemm is a torch float64
expression for every epilogue; the float32 transcriptions differ from their models by a rounding
error and no more; wide_plan matches the launch counts one can read off wide.py by hand."""
import numpy as np
import pytest
import torch

from . import layered_oracle as lo
from . import wide_oracle as wo

F32 = np.float32


def _mlp(rng, dims):
    Ws = [(rng.randn(dims[l + 1], dims[l]) / np.sqrt(dims[l])).astype(F32) for l in range(len(dims) - 1)]
    bs = [(rng.randn(dims[l + 1]) * 0.1).astype(F32) for l in range(len(dims) - 1)]
    return Ws, bs


@pytest.mark.parametrize("dims", [[14, 24, 16, 2], [5, 9, 3], [7, 4]])
def test_stage_models_without_rounding_are_float64_autograd(dims):
    """Two micro-batches (8 rows, then a tail of 5) accumulated with beta = 0 then 1, rounding
    replaced by identity: the gradients of the mean cross-entropy over all 13 rows, to 1e-12
    relative to the largest entry of each tensor's own float64 gradient."""
    rng = np.random.RandomState(len(dims))
    Ws, bs = _mlp(rng, dims)
    n, mb = 13, 8
    x, y = rng.randn(n, dims[0]).astype(F32), rng.randint(0, dims[-1], n)
    ident = lambda v: np.asarray(v, dtype=np.float64)
    gW = [np.full(w.shape, np.nan) for w in Ws]          # beta = 0 must not read them
    gb = [np.full(b.shape, np.nan) for b in bs]
    for r0 in range(0, n, mb):
        beta = 0.0 if r0 == 0 else 1.0
        if beta == 0.0:
            gW0, gb0 = [np.zeros_like(g) for g in gW], [np.zeros_like(g) for g in gb]
        else:
            gW0, gb0 = gW, gb
        gW, gb, _ = wo.micro_batch(Ws, bs, x[r0:r0 + mb], y[r0:r0 + mb], n, beta, gW0, gb0, rnd=ident)
    tW = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in Ws]
    tb = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for b in bs]
    h = torch.tensor(x, dtype=torch.float64)
    for l in range(len(Ws)):
        h = h @ tW[l].T + tb[l]
        if l + 1 < len(Ws):
            h = torch.relu(h)
    torch.nn.functional.cross_entropy(h, torch.tensor(y), reduction="mean").backward()
    for got, t in zip(gW + gb, tW + tb):
        want = t.grad.numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_stage_functions_compose_to_micro_batch():
    """The per-stage functions the GPU test applies to snapshots, chained with the same rounding,
    give micro_batch's gradients (float64 both ways: equal to 1e-12)."""
    rng = np.random.RandomState(3)
    dims, n = [14, 24, 16, 2], 11
    Ws, bs = _mlp(rng, dims)
    x, y = rng.randn(n, 14).astype(F32), rng.randint(0, 2, n)
    gW0, gb0 = [rng.randn(*w.shape).astype(F32) for w in Ws], [rng.randn(*b.shape).astype(F32) for b in bs]
    want_W, want_b, _ = wo.micro_batch(Ws, bs, x, y, n, 0.5, gW0, gb0)
    Wq = [lo.bf16_round(w) for w in Ws]
    acts = [lo.bf16_round(x)]
    for l in range(2):
        acts.append(lo.bf16_round(wo.stage_forward(acts[l], Wq[l], bs[l])[0].astype(F32)))
    z = wo.stage_logits(acts[2], Wq[2], bs[2])[0]
    dz = wo.stage_head(z, y, n)[0]
    got_b = {2: wo.stage_bgrad(dz, 0.5, gb0[2])[0]}
    d = wo.stage_pad_delta(dz.astype(F32), n, 2)
    got_W = {}
    for l in (2, 1, 0):
        got_W[l] = wo.stage_wgrad(d, acts[l], 0.5, gW0[l])[0]
        if l < 2:
            got_b[l] = wo.stage_bgrad(d, 0.5, gb0[l])[0]
        if l > 0:
            d = lo.bf16_round(wo.stage_dgrad(d, Wq[l], acts[l])[0].astype(F32))
    for l in range(3):
        # (the chain above rounds float64 -> float32 -> bf16, micro_batch float64 -> bf16 through
        # the same float32 cast inside bf16_round: identical values)
        assert np.abs(got_W[l] - want_W[l]).max() <= 1e-12 * np.abs(want_W[l]).max()
        # (the head's bias gradient sums dz_out as stored, in fp32: one rounding per term)
        tol = 2.0 ** -24 if l == 2 else 1e-12
        assert np.abs(got_b[l] - want_b[l]).max() <= tol * np.abs(want_b[l]).max()


EPILOGUES = [dict(), dict(alpha=0.5), dict(bias=True), dict(bias=True, relu=True), dict(mask=True),
             dict(beta=1.0), dict(alpha=0.3, beta=0.5, bias=True, relu=True, mask=True)]


@pytest.mark.parametrize("K", [64, 192])
def test_nt_gemm_is_the_torch_float64_expression(K):
    """Every epilogue, in the kernel's order; the mask holds zeros of both signs, negatives,
    infinities and NaN.  The transcription's error is a rounding error: non-zero and below
    K * 2^-24 of sum |terms|."""
    rng = np.random.RandomState(K)
    M, N = 24, 40
    A, B = lo.bf16_round(rng.randn(M, K).astype(F32)), lo.bf16_round(rng.randn(N, K).astype(F32))
    bias, C0 = rng.randn(N).astype(F32), rng.randn(M, N).astype(F32)
    mask = lo.bf16_round(rng.randn(M, N).astype(F32))
    mask.ravel()[:7] = np.array([0.0, -0.0, -1.0, 2.0 ** -126, np.inf, -np.inf, np.nan], dtype=F32)
    for e in EPILOGUES:
        alpha, beta = e.get("alpha", 1.0), e.get("beta", 0.0)
        ref, tr, scale = wo.nt_gemm(A, B, alpha, bias if e.get("bias") else None, e.get("relu", False),
                                    mask if e.get("mask") else None, beta, C0)
        t = float(F32(alpha)) * (torch.tensor(A, dtype=torch.float64) @ torch.tensor(B, dtype=torch.float64).T)
        if e.get("bias"):
            t = t + torch.tensor(bias, dtype=torch.float64)
        if e.get("relu"):
            t = torch.relu(t)
        if e.get("mask"):
            t = torch.where(torch.tensor(mask) > 0, t, torch.zeros_like(t))
        if beta:
            t = t + float(F32(beta)) * torch.tensor(C0, dtype=torch.float64)
        assert np.abs(ref - t.numpy()).max() <= 1e-13 * np.abs(t.numpy()).max()
        assert (scale >= np.abs(ref) * (1 - 1e-12)).all()
        err = lo.nerr(tr, ref, scale)
        assert 0.0 < err < K * 2.0 ** -24, (e, err)
    keep = wo.keep_of(mask)
    assert list(keep.ravel()[:7]) == [False, False, False, True, True, False, False]


def test_nt_csum_and_bf16_interval():
    rng = np.random.RandomState(1)
    Cb = lo.bf16_round(rng.randn(256, 5).astype(F32))
    s, a = wo.nt_csum(Cb)
    assert s.shape == (2, 5)
    np.testing.assert_allclose(s[1], Cb[128:].astype(float).sum(0), rtol=1e-14)
    np.testing.assert_allclose(a[0], np.abs(Cb[:128]).astype(float).sum(0), rtol=1e-14)
    ref = np.array([1.0, -1.0, 1e-3, 0.5])
    lo_, hi = wo.bf16_interval(ref, np.full(4, 2e-3), relu=True, keep=np.array([True, True, True, False]))
    assert lo_[0] <= 1.0 <= hi[0] and lo_[0] < hi[0]
    assert lo_[1] == hi[1] == 0.0 and lo_[3] == hi[3] == 0.0
    assert lo_[2] == 0.0 and hi[2] > 0.0


@pytest.mark.parametrize("C,trans,bias", [(2, 0, False), (14, 1, True), (14, 1, False)])
@pytest.mark.parametrize("rows,splits", [(1, 3), (37, 1), (37, 5), (37, 40)])
@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
def test_skinny_wgrad_model_and_transcription(C, trans, bias, rows, splits, beta):
    rng = np.random.RandomState(rows + splits)
    Nw = 16
    W, S = lo.bf16_round(rng.randn(rows, Nw).astype(F32)), lo.bf16_round(rng.randn(rows, C + 3).astype(F32))
    out0 = rng.randn(C, Nw).astype(F32) if not trans else rng.randn(Nw, C).astype(F32)
    b0 = rng.randn(Nw).astype(F32) if bias else None
    r = wo.skinny_wgrad(W, S, C, rows, trans, splits, beta, out0, b0)
    ref, tr, scale = r["out"]
    t = torch.tensor(S[:, :C], dtype=torch.float64).T @ torch.tensor(W, dtype=torch.float64)
    t = (t.T if trans else t) + beta * torch.tensor(out0, dtype=torch.float64)
    assert np.abs(ref - t.numpy()).max() <= 1e-13 * max(1.0, np.abs(t.numpy()).max())
    assert lo.nerr(tr, ref, scale) < (rows + 2) * 2.0 ** -24
    rc = -(-rows // splits)
    for z in range(splits):
        if z * rc >= rows:
            assert (r["slab"][z] == 0).all()
    assert (r["bias"] is not None) == bias
    if bias:
        bref, btr, bscale = r["bias"]
        np.testing.assert_allclose(bref, W.astype(float).sum(0) + beta * b0, rtol=1e-13, atol=1e-15)
        assert lo.nerr(btr, bref, bscale) < (rows + 2) * 2.0 ** -24
    if rows == 37 and splits == 5 and beta == 0.5:
        assert lo.nerr(tr, ref, scale) > 0.0


@pytest.mark.parametrize("N", [1, 3, 14, 64])
@pytest.mark.parametrize("M,splits", [(1, 1), (7, 9), (1000, 7), (4097, 3)])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_colsum_split_model_and_transcription(N, M, splits, beta):
    rng = np.random.RandomState(N + M)
    X, out0 = rng.randn(M, N).astype(F32), rng.randn(N).astype(F32)
    (ref, tr, scale), slab, eff = wo.colsum_split(X, splits, beta, out0)
    np.testing.assert_allclose(ref, X.astype(float).sum(0) + beta * out0, rtol=1e-13, atol=1e-15)
    assert eff == -(-M // -(-M // splits)) and slab.shape == (eff, N)
    e = lo.nerr(tr, ref, scale)
    assert e < (M + 2) * 2.0 ** -24
    if M >= 1000:
        assert e > 0.0


def test_stage_transcriptions_are_rounding_errors():
    rng = np.random.RandomState(9)
    K = 128
    dZ, inp = lo.bf16_round(rng.randn(K, 24).astype(F32) * 1e-3), lo.bf16_round(rng.randn(K, 40).astype(F32))
    g0 = rng.randn(24, 40).astype(F32)
    for beta in (0.0, 1.0):
        ref, tr, scale = wo.stage_wgrad(dZ, inp, beta, g0)
        assert ref.shape == (24, 40) and 0.0 < lo.nerr(tr, ref, scale) < K * 2.0 ** -24
        ref, tr, scale = wo.stage_bgrad(dZ, beta, g0[:, 0])
        # (128 bf16 values of one magnitude add exactly in fp32; only the beta term rounds)
        e = lo.nerr(tr, ref, scale)
        assert ref.shape == (24,) and e < K * 2.0 ** -24 and (e > 0.0) == (beta != 0.0)
    z, y = rng.randn(50, 3).astype(F32), rng.randint(0, 3, 50)
    ref, tr, scale = wo.stage_head(z, y, 456)
    assert 0.0 < lo.nerr(tr, ref, scale) < 16 * 2.0 ** -24
    p = wo.stage_pad_delta(ref.astype(F32), 64, 8)
    assert (p[50:] == 0).all() and (p[:, 3:] == 0).all()
    np.testing.assert_array_equal(p[:50, :3], lo.bf16_round(ref.astype(F32)))


PLANS = [
    # dims, mb, rows -> rp, forward_nt, dgrad_nt, csum, wgrad_nt, bias, skinny, nt_calls
    ([14, 256, 128, 256, 2], 256, 256, 256, [1, 1, 1, 1], [1, 1, 1], [0, 0, 1], [0, 1, 1, 0],
     ["skinny", "rowsum", "csum"], True, 9),
    ([14, 256, 128, 256, 2], 256, 200, 256, [1, 1, 1, 1], [1, 1, 1], [0, 0, 1], [0, 1, 1, 0],
     ["skinny", "rowsum", "csum"], True, 9),
    ([14, 256, 256, 2], 128, 128, 128, [1, 1, 1], [1, 1], [0, 0], [0, 1, 0], ["skinny", "rowsum"], True, 6),
    ([14, 256, 256, 2], 128, 72, 128, [1, 1, 1], [1, 1], [0, 0], [0, 1, 0], ["skinny", "rowsum"], True, 6),
    ([17, 128, 256, 3], 256, 256, 256, [1, 1, 1], [1, 1], [0, 1], [0, 1, 0], ["rowsum", "csum"], False, 6),
    ([17, 128, 256, 3], 256, 128, 128, [1, 1, 1], [1, 1], [0, 0], [0, 1, 0], ["rowsum", "rowsum"], False, 6),
    ([14, 200, 72, 2], 256, 256, None, [0, 0, 0], [0, 0], [0, 0], [0, 0, 0], ["skinny", "rowsum"], True, 0),
    ([14, 200, 72, 2], 256, 100, None, [0, 0, 0], [0, 0], [0, 0], [0, 0, 0], ["skinny", "colsum"], True, 0),
    ([14, 256, 192, 256, 2], 256, 256, 256, [1, 0, 1, 1], [1, 0, 1], [0, 0, 1], [0, 0, 0, 0],
     ["skinny", "rowsum", "csum"], True, 5),
    ([14, 256, 192, 256, 2], 256, 100, None, [0, 0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0, 0],
     ["skinny", "colsum", "colsum"], True, 0),
]


@pytest.mark.parametrize("case", PLANS, ids=lambda c: f"{'-'.join(map(str, c[0]))}/mb{c[1]}/rows{c[2]}")
def test_wide_plan_matches_a_hand_count(case):
    """The launches of each row were counted by hand from wide.py's _forward / _backward."""
    dims, mb, rows, rp, fwd, dg, cs, wg, bias, skinny, calls = case
    p = wo.wide_plan(dims, mb, rows)
    assert p["rp"] == rp and p["skinny"] == skinny
    assert [int(v) for v in p["forward_nt"]] == fwd
    assert [int(v) for v in p["dgrad_nt"]] == dg
    assert [int(v) for v in p["csum"]] == cs
    assert [int(v) for v in p["wgrad_nt"]] == wg
    assert p["bias"] == bias and p["nt_calls"] == calls

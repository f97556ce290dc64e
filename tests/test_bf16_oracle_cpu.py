"""The host models of tests/bf16_oracle.py against each other, without a GPU: what the bf16 scoring
tests take for granted.  For every shape of tests/test_bf16_scoring.py: the split-bf16 model sits
within 5e-5 max|z| of exact float64 (measured worst 1.6e-5, 14-33-17-9-5) and agrees with it on
every sure row; the plain (hi.hi) model is at least 1e-3 max|z| away; every planted shard holds at
least 4 rows the two models score differently, at the block edges first, so their confusion
matrices and metric vectors differ; and the loss tolerance of the GPU test is at most 1/8 of the
distance between the two models' losses and at least the fp32 noise allowance."""
import numpy as np
import pytest

from . import bf16_oracle as bo
from .reference_oracle import (BF16_GRAD_CASES, DATA_SEED, INIT_SEED, _split_bf16_reference_grad, float64_logits,
                               make_multiclass)

SHAPES = sorted({dims for dims, _ in bo.SCORING_CASES})
SHARDS = [(dims, R, n) for dims, R in bo.SCORING_CASES for n in bo.shard_sizes(R)]


@pytest.mark.parametrize("dims", SHAPES, ids=["-".join(map(str, d)) for d in SHAPES])
def test_split_model_is_exact_to_16_bits_and_plain_is_not(dims):
    c = bo.candidates(bo.trained_flat(dims), dims)
    zs, zp, ze = (c.z[m] for m in bo.MODES)
    d_exact, d_plain = np.abs(zs - ze).max() / c.sc, np.abs(zp - zs).max() / c.sc
    print(dims, "sc", c.sc, "split-exact", d_exact, "plain-split", d_plain, "discriminating", int(c.disc.sum()),
          "unsure", int((~c.sure).sum()))
    assert d_exact <= 5e-5, d_exact
    assert d_plain >= 1e-3, d_plain
    assert (~c.sure).sum() <= 4   # of 20 000
    np.testing.assert_array_equal(np.argmax(zs, 1)[c.sure], np.argmax(ze, 1)[c.sure])
    assert c.disc.sum() >= 4
    # the teacher's labels, not the model's predictions: every class, and rows the model gets wrong
    assert len(np.unique(c.y)) == dims[-1] and (np.argmax(zs, 1) != c.y).mean() > 0.05


@pytest.mark.parametrize("dims,R,n", SHARDS, ids=[bo.case_id(*s) for s in SHARDS])
def test_planted_shard(dims, R, n):
    flat, s = bo.scoring_shard(dims, R, n)
    c = bo.candidates(flat, dims)
    assert s.X.shape == (n, dims[0]) and s.y.shape == (n,)
    # rows of the candidates, each once, none of them unsure; the rows' own labels
    assert len(set(s.index.tolist())) == n and c.sure[s.index].all()
    np.testing.assert_array_equal(s.X, c.X[s.index])
    np.testing.assert_array_equal(s.y, c.y[s.index])
    # the discriminating rows: at least 4, all there are up to n // 2, the block edges first
    assert len(s.disc_rows) == min(int(c.disc.sum()), n // 2) >= 4
    np.testing.assert_array_equal(np.flatnonzero(c.disc[s.index]), s.disc_rows)
    edges = bo.edge_rows(n, R)
    assert set(edges) == {0, R - 1, n - 1, ((n - 1) // R) * R} and set(edges) <= set(s.disc_rows.tolist())
    # what the models make of the shard, recomputed from the rows (a float64 product of n rows
    # and one of 20 000 may block their sums differently: 1e-12, not bit for bit)
    z = {m: bo.bf16_logits(flat, dims, s.X, m) for m in bo.MODES}
    for m in bo.MODES:
        np.testing.assert_allclose(z[m], c.z[m][s.index], rtol=0, atol=1e-12 * c.sc)
    C = dims[-1]
    np.testing.assert_array_equal(s.cm_split, bo.confusion(s.y, z["split"], C))
    np.testing.assert_array_equal(s.cm_split, bo.confusion(s.y, z["exact"], C))
    np.testing.assert_array_equal(s.cm_plain, bo.confusion(s.y, z["plain"], C))
    assert s.cm_split.sum() == s.cm_plain.sum() == n
    assert (s.cm_split != s.cm_plain).sum() >= 2
    assert np.abs(s.metrics("split") - s.metrics("plain")).max() > 1e-9
    assert (s.cm_split - np.diag(np.diag(s.cm_split))).sum() > 0   # off-diagonal mass
    for m, ce in zip(bo.MODES, (s.ce_split, s.ce_plain, s.ce_exact)):
        assert abs(ce - bo.cross_entropy(z[m], s.y)) <= 1e-12 * ce
    # the loss: the split model is the exact one to 1/8 of the tolerance, the plain one 8 tolerances away
    tol = bo.loss_tolerance(s)
    print(bo.case_id(dims, R, n), "CE split", s.ce_split, "gap", s.ce_gap, "tolerance", tol,
          "exact-split", abs(s.ce_exact - s.ce_split) / s.ce_split)
    assert bo.LOSS_NOISE <= tol <= bo.LOSS_RTOL
    assert s.ce_gap >= 8 * tol
    assert abs(s.ce_exact - s.ce_split) / s.ce_split <= tol / 2


def test_planted_shard_is_cached_and_read_only():
    dims, R = bo.SCORING_CASES[0]
    a, b = bo.scoring_shard(dims, R, R + 1), bo.scoring_shard(dims, R, R + 1)
    assert a[0] is b[0] and a[1] is b[1] and bo.trained_flat(dims) is a[0]
    with pytest.raises(ValueError):
        a[1].X[0, 0] = 0.0
    with pytest.raises(ValueError):
        a[0][0] = 0.0


def test_bf16_logits_modes():
    dims = (14, 7, 2)
    flat = bo.trained_flat(dims)
    X, _ = make_multiclass(50, 14, 2, DATA_SEED + 2)
    np.testing.assert_array_equal(bo.bf16_logits(flat, dims, X, "exact"), float64_logits(flat, list(dims), X))
    with pytest.raises(ValueError):
        bo.bf16_logits(flat, dims, X, "hi")
    # one Linear layer whose parameters and inputs ARE bf16 numbers has no lo parts: the three
    # models coincide
    import torch
    from fedmi.models.mlp import init_flat
    bf = lambda a: torch.as_tensor(a).to(torch.bfloat16).to(torch.float32).numpy()
    one = bf(init_flat([14, 3], INIT_SEED))
    one[14 * 3:] = init_flat([14, 3], INIT_SEED)[14 * 3:]   # the bias stays fp32 in every model
    zs, zp, ze = (bo.bf16_logits(one, (14, 3), bf(X), m) for m in bo.MODES)
    np.testing.assert_array_equal(zs, zp)
    np.testing.assert_allclose(zs, ze, rtol=0, atol=1e-12 * np.abs(ze).max())
    # ... and with a hidden layer the split model still carries the lo part of its fp32 activations
    zs, zp, ze = (bo.bf16_logits(bf(flat), dims, bf(X), m) for m in bo.MODES)
    assert np.abs(zs - ze).max() < 0.1 * np.abs(zp - ze).max()


@pytest.mark.parametrize("rows,F,C,hidden,R,slab", BF16_GRAD_CASES[:3])
def test_reference_gradient_plain_flag(rows, F, C, hidden, R, slab):
    """plain=True is off by default and moves the host gradient (the forward it back-propagates from
    changed, and with it which bf16 number a delta rounds to) by more than the 1e-3 the kernel's
    gradient is held to, so a GPU test can tell which forward a train kernel ran (measured 0.8e-2
    to 1.1e-2), and by no more than a few bf16 roundings."""
    from fedmi.models.mlp import init_flat
    dims = [F, *hidden, C]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    flat = init_flat(dims, INIT_SEED)
    g = _split_bf16_reference_grad(flat, X, y, dims, scaled_delta=slab == "fp32")
    np.testing.assert_array_equal(g, _split_bf16_reference_grad(flat, X, y, dims, slab == "fp32", plain=False))
    gp = _split_bf16_reference_grad(flat, X, y, dims, scaled_delta=slab == "fp32", plain=True)
    d = np.linalg.norm(gp - g) / np.linalg.norm(g)
    print((rows, F, C, hidden), "plain vs split gradient", d)
    assert 2e-3 < d < 5e-2, d

"""The float64 oracle of the layered-path op tests (layered_oracle.py) against independent
implementations: torch autograd, torch.optim.Adam, scikit-learn's AdamOptimizer and stopping
rule, torch's CPU bf16 cast.  No GPU: the op tests trust the oracle, so it is checked here."""
import warnings

import numpy as np
import pytest
import torch

from . import layered_oracle as lo


def test_bf16_rounding_is_torchs_cpu_cast():
    rng = np.random.RandomState(0)
    x = np.concatenate([
        rng.randn(4096).astype(np.float32) * np.float32(10.0) ** rng.randint(-30, 30, 4096).astype(np.float32),
        # exact ties (…8000 below an even and an odd bf16 mantissa), carries into the next binade,
        # +-0, +-inf, the largest finite fp32, subnormals
        np.array([0x3F808000, 0x3F818000, 0x3F7F8000, 0x3FFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000, 0x80000000,
                  0x7F800000, 0xFF800000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF],
                 dtype=np.uint32).view(np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(lo.bf16_bits(x), want)
    np.testing.assert_array_equal(lo.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert np.isnan(lo.bf16_round(np.array([np.nan, -np.nan], dtype=np.float32))).all()


@pytest.mark.parametrize("C", [2, 3, 16])
def test_ce_head_is_torch_cross_entropy(C):
    rng = np.random.RandomState(C)
    M = 37
    z = rng.randn(M, C) * 3.0
    z[0] = 1.25                                   # all equal
    z[1] = np.linspace(-5e3, 5e3, C)              # saturated
    y = rng.randint(0, C, M)
    y[1] = 0                                      # true class at the minimum logit
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    loss = torch.nn.functional.cross_entropy(zt, torch.as_tensor(y), reduction="sum")
    loss.backward()
    rows, dz, pred = lo.ce_head(z, y, 0.25)
    np.testing.assert_allclose(rows.sum(), loss.item(), rtol=1e-13)
    np.testing.assert_allclose(dz, 0.25 * zt.grad.numpy(), rtol=1e-12, atol=1e-16)
    np.testing.assert_array_equal(pred, zt.detach().argmax(dim=1).numpy())
    assert pred[0] == 0                           # ties: the first maximum
    assert np.isfinite(rows).all() and np.isfinite(dz).all()


def test_binary_head_is_clipped_log_loss():
    from math import exp, log
    z = np.array([0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0, 3.0, -2.0, 15.0, 745.0, -745.0])
    for yv in (0, 1):
        y = np.full(len(z), yv)
        rows, dz, pred = lo.binary_head(z, y, 0.5)
        for i, zi in enumerate(z):
            p = 1.0 / (1.0 + exp(-zi)) if zi > -700 else 0.0          # expit
            pc = min(max(p, lo.EPS32), 1.0 - lo.EPS32)
            want = -log(pc) if yv else -log(1.0 - pc)
            assert abs(rows[i] - want) <= 1e-14 * max(1.0, abs(want))
            assert abs(dz[i] - 0.5 * (p - yv)) <= 1e-15           # unclipped p
            assert pred[i] == (1 if p > 0.5 else 0)
        assert rows.max() <= -log(lo.EPS32) * (1 + 1e-15)             # the clip caps the loss
    assert lo.EPS32 == 2.0 ** -23
    # against torch's own float64 binary cross-entropy where the clip is not active
    zz = np.linspace(-10, 10, 41)
    yy = (np.arange(41) % 2)
    want = torch.nn.functional.binary_cross_entropy_with_logits(
        torch.tensor(zz), torch.tensor(yy, dtype=torch.float64), reduction="none").numpy()
    np.testing.assert_allclose(lo.binary_head(zz, yy, 1.0)[0], want, rtol=1e-9)


@pytest.mark.parametrize("wd", [0.0, 0.03])
def test_adam_style0_is_torch_adam(wd):
    rng = np.random.RandomState(1)
    n = 257
    p = rng.randn(n)
    m, v = np.zeros(n), np.zeros(n)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=0.004, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    for t in range(1, 21):
        g = rng.randn(n) * 10.0 ** rng.randint(-4, 3, n)
        pt.grad = torch.tensor(g)
        opt.step()
        p, m, v, _ = lo.adam_step(p, m, v, g, style=0, lr=0.004, beta1=0.9, beta2=0.999, eps=1e-8, t=t, wd=wd)
        np.testing.assert_allclose(p, pt.detach().numpy(), rtol=1e-12, atol=1e-14)


def test_adam_masks_fedprox_and_l2_term():
    rng = np.random.RandomState(2)
    n = 50
    p, g, anchor = rng.randn(n), rng.randn(n), rng.randn(n)
    mask = np.zeros(n, dtype=np.uint8)
    mask[:7] = 1
    mask[20:31] = 1
    kw = dict(style=1, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, t=3)
    got = lo.adam_step(p, np.zeros(n), np.zeros(n), g, wd=0.1, wd_mask=mask, mu=0.2, anchor=anchor, l2_coef=0.5, **kw)
    g_eff = g + 0.1 * p * mask + 0.2 * (p - anchor)
    want = lo.adam_step(p, np.zeros(n), np.zeros(n), g_eff, **kw)
    for a, b in zip(got[:3], want[:3]):
        np.testing.assert_allclose(a, b, rtol=1e-14)
    np.testing.assert_allclose(got[3], 0.5 * np.sum(p[mask == 1] ** 2), rtol=1e-14)
    assert want[3] == 0.0


def test_adam_style1_is_sklearn_adam_optimizer():
    pytest.importorskip("sklearn")
    from sklearn.neural_network._stochastic_optimizers import AdamOptimizer
    rng = np.random.RandomState(3)
    params = [rng.randn(5, 7), rng.randn(7)]
    opt = AdamOptimizer([a.copy() for a in params], 0.004, 0.9, 0.999, 1e-8)
    sk = [a.copy() for a in params]
    opt.params = sk
    p = np.concatenate([a.ravel() for a in params])
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, 21):
        grads = [rng.randn(5, 7), rng.randn(7)]
        opt.update_params(sk, grads)
        p, m, v, _ = lo.adam_step(p, m, v, np.concatenate([a.ravel() for a in grads]), style=1, lr=0.004, beta1=0.9,
                                  beta2=0.999, eps=1e-8, t=t)
        np.testing.assert_allclose(p, np.concatenate([a.ravel() for a in sk]), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("tol,nic", [(1e-2, 2), (1e-4, 3)])
def test_epoch_end_rule_is_sklearns(tol, nic):
    sknn = pytest.importorskip("sklearn.neural_network")
    warnings.filterwarnings("ignore")
    rng = np.random.RandomState(4)
    n = 100
    # a loss sequence that improves, stalls within tol, recovers (reset), then stalls for good
    losses = np.concatenate([np.linspace(1.0, 0.5, 6), 0.5 - 1e-5 * np.arange(1, 3), [0.3],
                             0.3 + 1e-6 * rng.rand(12)])
    sk = sknn.MLPClassifier(tol=tol, n_iter_no_change=nic)
    sk.loss_curve_, sk.best_loss_, sk._no_improvement_count = [], np.inf, 0
    ee = lo.EpochEnd(n, tol, nic, max_iter=len(losses), tol_stop=1)
    stopped = None
    for it, loss in enumerate(losses):
        assert ee.update(loss * n) == 0.0
        sk.loss_curve_.append(loss * n / n)
        sk._update_no_improvement_count(False, None, None, None)
        assert ee.count == sk._no_improvement_count and ee.best == sk.best_loss_
        assert ee.curve == sk.loss_curve_ and ee.n_iter == it + 1
        if sk._no_improvement_count > nic:            # _fit_stochastic breaks here
            stopped = it + 1
            break
        assert ee.active == (0 if it + 1 == len(losses) else 1)
    assert stopped is not None and stopped < len(losses) and ee.active == 0
    assert ee.update(123.0) == 123.0 and ee.n_iter == stopped      # a stopped trial is left alone


def test_epoch_end_max_iter_and_no_tol_stop():
    ee = lo.EpochEnd(10, 1e-4, 1, max_iter=5, tol_stop=0)
    for it in range(5):
        assert ee.active == 1
        ee.update(10.0)
    assert ee.active == 0 and ee.n_iter == 5 and ee.count == 4 and len(ee.curve) == 5


def test_gather_and_confusion_models():
    rng = np.random.RandomState(5)
    X, y = rng.randn(20, 6), rng.randint(0, 3, 20)
    perms = np.stack([rng.permutation(20) for _ in range(3)])
    out, yb = lo.gather_rows(X, y, perms, 2, 4, 5, 4, 8)
    for i in range(5):
        np.testing.assert_array_equal(out[i, :4], X[perms[2, 4 + i], :4])
        assert yb[i] == y[perms[2, 4 + i]]
    assert (out[:, 4:] == 0).all()
    out, yb = lo.gather_rows(X, y, None, 0, 3, 2, 6, 6)
    np.testing.assert_array_equal(out, X[3:5])
    cm = lo.confusion([0, 1, 1, 2], [0, 1, 2, 2], 3)
    np.testing.assert_array_equal(cm, [[1, 0, 0], [0, 1, 0], [0, 1, 1]])


def test_bounds_reject_subtly_wrong_variants():
    """The op tests' data-driven bound (4x the transcription's error) is far below the effect of
    the mistakes it is there to catch: a bias correction one step off at t = 1000, a learning
    rate without sqrt(1 - beta2^t), a probability clip at the float64 epsilon."""
    rng = np.random.RandomState(7)
    n = 1025
    g = (10.0 ** rng.uniform(-8, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    p = rng.randn(n).astype(np.float32)
    m0 = (rng.randn(n) * np.abs(g)).astype(np.float32)
    v0 = (rng.rand(n) * g.astype(float) ** 2).astype(np.float32)
    kw = dict(lr=0.004, beta1=0.9, beta2=0.999, eps=1e-8)
    for style in (0, 1):
        ref = lo.adam_step(p, m0, v0, g, style=style, t=1000, **kw)[0]
        scale = np.abs(p) + np.abs(ref - p)
        tb = lo.bound(lo.nerr(lo.adam_step_f32(p, m0, v0, g, style=style, t=1000, **kw)[0], ref, scale))
        off_by_one = lo.adam_step_f32(p, m0, v0, g, style=style, t=999, **kw)[0]
        assert lo.nerr(off_by_one, ref, scale) > 10 * tb
    ref1 = lo.adam_step(p, m0, v0, g, style=1, t=5, **kw)[0]
    scale = np.abs(p) + np.abs(ref1 - p)
    tb = lo.bound(lo.nerr(lo.adam_step_f32(p, m0, v0, g, style=1, t=5, **kw)[0], ref1, scale))
    no_sqrt = p - np.float32(0.004 / (1 - 0.9 ** 5)) * lo.adam_step_f32(p, m0, v0, g, style=1, t=5, **kw)[1] / (
        np.sqrt(lo.adam_step_f32(p, m0, v0, g, style=1, t=5, **kw)[2]) + np.float32(1e-8))
    assert lo.nerr(no_sqrt, ref1, scale) > 10 * tb
    z, y = np.array([20.0, -20.0, 1.0], dtype=np.float32), np.array([0, 1, 1])
    rows = lo.binary_head(z, y, 1.0)[0]
    tb = lo.bound(lo.nerr(lo.binary_head_f32(z, y, 1.0)[0], rows, 1.0 + np.abs(rows)))
    wide_clip = lo.binary_head(z, y, 1.0, eps=np.finfo(np.float64).eps)[0]
    assert lo.nerr(wide_clip, rows, 1.0 + np.abs(rows)) > 0.1 > 10 * tb


def test_fp32_transcriptions_track_the_oracle():
    """The transcriptions are float32 roundings of the same formulas: a few ulp from the oracle."""
    rng = np.random.RandomState(6)
    z, y = rng.randn(64, 5) * 2, rng.randint(0, 5, 64)
    rows, dz, _ = lo.ce_head(z.astype(np.float32), y, 0.5)
    r32, d32 = lo.ce_head_f32(z, y, 0.5)
    assert 0 < lo.nerr(d32, dz, 0.5) < 8 * lo.EPS32
    assert lo.nerr(r32, rows, np.abs(z).max(axis=1) * 2 + 2) < 8 * lo.EPS32
    A, B = rng.randn(9, 40).astype(np.float32), rng.randn(40, 11).astype(np.float32)
    e = lo.nerr(lo.matmul_f32(A, B), A.astype(float) @ B.astype(float), np.abs(A) @ np.abs(B))
    assert 0 < e < 40 * lo.EPS32
    np.testing.assert_allclose(lo.sum_f32(A, 1), A.astype(float).sum(1), rtol=0, atol=1e-4)
    p, m, v, g = (rng.randn(100) for _ in range(4))
    v = v * v
    for style in (0, 1):
        kw = dict(style=style, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, t=5)
        f32 = [a.astype(np.float32) for a in (p, m, v, g)]
        ref = lo.adam_step(*f32, **kw)
        got = lo.adam_step_f32(*f32, **kw)
        for a, b in zip(got, ref[:3]):
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7)

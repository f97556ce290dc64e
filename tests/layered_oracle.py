"""Float64 models of the layered-path operations (mlp_ops.hip, the small kernels of gemm_mfma.hip
and the helpers of gemm_nt_bf16.hip), one plain numpy function per operation, as the kernels'
comments state them.  No GPU import: ``test_layered_oracle_cpu.py`` pins every model to an
independent implementation (torch autograd, ``torch.optim.Adam``, scikit-learn), and
``test_layered_ops.py`` compares the HIP kernels with the models.

The second half holds float32 TRANSCRIPTIONS of the same formulas in the kernels' operation
order.  They are not references: their distance from the float64 model on a test's own inputs is
the rounding error a correct fp32 implementation shows there, and the op tests allow a kernel
four times that (``bound``).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
F64 = np.float64
EPS32 = float(np.finfo(np.float32).eps)      # 2^-23: the binary head's probability clip


# ----------------------------------------------------------------------------- bf16
def bf16_bits(x) -> np.ndarray:
    """fp32 -> bf16 bit patterns (uint16), round to nearest, ties to even; NaN stays a (quiet) NaN."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, dtype=F32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_round(x) -> np.ndarray:
    """The bf16 rounding of fp32 values, as fp32."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(F32)


# ----------------------------------------------------------------------------- loss heads
def ce_head(z, y, scale):
    """Softmax cross-entropy head.  z [M][C], y [M] -> (row losses [M], dz = (p - onehot) * scale,
    first-maximum argmax [M]); the loss of a minibatch is the SUM of the row losses."""
    z = np.asarray(z, dtype=F64)
    y = np.asarray(y)
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    se = e.sum(axis=1, keepdims=True)
    rows = np.arange(z.shape[0])
    loss = mx[:, 0] + np.log(se[:, 0]) - z[rows, y]
    p = e / se
    p[rows, y] -= 1.0
    return loss, p * float(scale), np.argmax(z, axis=1)       # np.argmax: first maximum


def binary_head(z, y, scale, eps=EPS32):
    """sklearn binary head.  z [M] logits, y [M] in {0, 1}: logistic output p, log-loss of p clipped
    to [eps, 1 - eps] (the kernel clips at the fp32 epsilon), dz = (p - y) * scale with the
    UNCLIPPED p, prediction p > 0.5."""
    z = np.asarray(z, dtype=F64)
    y = np.asarray(y)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
    pc = np.clip(p, eps, 1.0 - eps)
    loss = np.where(y != 0, -np.log(pc), -np.log(1.0 - pc))
    return loss, (p - y.astype(F64)) * float(scale), (p > 0.5).astype(np.int64)


# ----------------------------------------------------------------------------- Adam
def adam_step(p, m, v, g, *, style, lr, beta1, beta2, eps, t, wd=0.0, wd_mask=None, mu=0.0, anchor=None,
              l2_coef=0.0):
    """One Adam step (1-based step t) -> (p, m, v, l2_term).
    style 0: torch.optim.Adam; style 1: sklearn AdamOptimizer.  The gradient first gains
    wd * p on the masked entries (all when wd_mask is None) and mu * (p - anchor) everywhere;
    l2_term = l2_coef * sum p^2 over the masked entries of the PRE-update weights."""
    p, m, v, g = (np.asarray(a, dtype=F64) for a in (p, m, v, g))
    mask = np.ones(p.shape, dtype=bool) if wd_mask is None else np.asarray(wd_mask).astype(bool)
    l2 = float(l2_coef) * float(np.sum(np.where(mask, p * p, 0.0)))
    g = g + np.where(mask, wd * p, 0.0)
    if mu != 0.0:
        g = g + mu * (p - np.asarray(anchor, dtype=F64))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** float(t), 1.0 - beta2 ** float(t)
    if style == 0:
        p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    else:
        p = p - (lr * np.sqrt(bc2) / bc1) * m / (np.sqrt(v) + eps)
    return p, m, v, l2


# ----------------------------------------------------------------------------- plumbing
def gather_rows(X, y, perms, epoch, off, M, F, ldo):
    """Minibatch assembly: rows perms[epoch][off : off + M] of X (identity when perms is None),
    first F features, zero padded to ldo -> (out [M][ldo], labels [M])."""
    X = np.asarray(X)
    src = np.arange(off, off + M) if perms is None else np.asarray(perms)[epoch, off:off + M]
    out = np.zeros((M, ldo), dtype=X.dtype)
    out[:, :F] = X[src, :F]
    return out, np.asarray(y)[src]


def confusion(pred, y, C):
    """cm[y][pred] counts."""
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (np.asarray(y), np.asarray(pred)), 1)
    return cm


class EpochEnd:
    """The end-of-epoch rule of one trial (sklearn _fit_stochastic + _update_no_improvement_count):
    loss = acc / n; append to the curve; count += 1 when loss > best - tol, else 0; best = min;
    stop when count > n_iter_no_change (if tol_stop) or at max_iter."""

    def __init__(self, n, tol, n_iter_no_change, max_iter, tol_stop, best=np.inf, count=0):
        self.n, self.tol, self.nic, self.max_iter, self.tol_stop = n, tol, n_iter_no_change, max_iter, tol_stop
        self.best, self.count, self.n_iter, self.active, self.curve = float(best), int(count), 0, 1, []

    def update(self, loss_acc):
        """Fold one epoch's accumulated loss in; returns the accumulator's new value."""
        if not self.active:
            return loss_acc
        loss = float(loss_acc) / float(self.n)
        if self.n_iter < self.max_iter:
            self.curve.append(loss)
        self.count = self.count + 1 if loss > self.best - self.tol else 0
        self.best = min(self.best, loss)
        self.n_iter += 1
        if (self.tol_stop and self.count > self.nic) or self.n_iter >= self.max_iter:
            self.active = 0
        return 0.0


# ----------------------------------------------------------------------------- error measure
def nerr(x, ref, scale) -> float:
    """max_i |x_i - ref_i| / scale_i: the error in units of each element's own magnitude
    (for a sum: the sum of its terms' magnitudes, so cancellation neither hides nor fakes an
    error).  An element with scale 0 must be exact."""
    d = np.abs(np.asarray(x, dtype=F64) - np.asarray(ref, dtype=F64))
    s = np.broadcast_to(np.asarray(scale, dtype=F64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0.0, 0.0, d / s)
    return float(np.max(q)) if q.size else 0.0


def bound(transcription_err: float) -> float:
    """What a kernel may differ from the float64 model by: four times the error of the float32
    transcription on the same inputs (fma contraction, expf / logf / sqrtf an ulp or two off
    numpy's, another fixed summation order)."""
    return 4.0 * float(transcription_err)


# ----------------------------------------------------------------------------- fp32 transcriptions
def ce_head_f32(z, y, scale):
    """xent_kernel mode 0 in float32, in its order: running max, se += expf(z - mx) over k,
    loss = mx + logf(se) - z[y], dz = (expf(z - mx) / se - onehot) * scale."""
    z = np.asarray(z, dtype=F32)
    y = np.asarray(y)
    scale = F32(scale)
    rows = np.arange(z.shape[0])
    mx = z.max(axis=1)
    e = np.exp(z - mx[:, None])
    se = np.zeros(z.shape[0], dtype=F32)
    for k in range(z.shape[1]):
        se = se + e[:, k]
    loss = (mx + np.log(se)) - z[rows, y]
    oh = np.zeros_like(z)
    oh[rows, y] = 1.0
    return loss.astype(F64), (e / se[:, None] - oh) * scale


def binary_head_f32(z, y, scale, eps=EPS32):
    """xent_kernel mode 1: p, the clip and dz in float32, the logarithm of the clipped p in double."""
    z = np.asarray(z, dtype=F32)
    y = np.asarray(y)
    with np.errstate(over="ignore"):
        p = F32(1.0) / (F32(1.0) + np.exp(-z))
    pc = np.minimum(np.maximum(p, F32(eps)), F32(1.0) - F32(eps)).astype(F64)
    loss = np.where(y != 0, -np.log(pc), -np.log(1.0 - pc))
    return loss, (p - y.astype(F32)) * F32(scale)


def adam_step_f32(p, m, v, g, *, style, lr, beta1, beta2, eps, t, wd=0.0, wd_mask=None, mu=0.0, anchor=None):
    """adam_kernel in float32: the two step coefficients in double then rounded, the element
    update in the kernel's order -> (p, m, v)."""
    p, m, v, g = (np.asarray(a, dtype=F32) for a in (p, m, v, g))
    mask = np.ones(p.shape, dtype=bool) if wd_mask is None else np.asarray(wd_mask).astype(bool)
    b1, b2, omb1, omb2 = F32(beta1), F32(beta2), F32(1.0 - beta1), F32(1.0 - beta2)
    if wd != 0.0:
        g = np.where(mask, g + F32(wd) * p, g)
    if mu != 0.0:
        g = g + F32(mu) * (p - np.asarray(anchor, dtype=F32))
    bc1, bc2 = 1.0 - beta1 ** float(t), 1.0 - beta2 ** float(t)
    if style == 0:
        c0, c1 = F32(lr / bc1), F32(np.sqrt(bc2))
        m = m + omb1 * (g - m)
        v = v * b2 + omb2 * g * g
        p = p + (-c0) * (m / (np.sqrt(v) / c1 + F32(eps)))
    else:
        c0 = F32(lr * np.sqrt(bc2) / bc1)
        m = b1 * m + omb1 * g
        v = b2 * v + omb2 * g * g
        p = p - c0 * m / (np.sqrt(v) + F32(eps))
    return p, m, v


def matmul_f32(A, B):
    """sum_k A[m][k] B[k][n] accumulated in float32 in k order (one rounding per product and per add)."""
    A, B = np.asarray(A, dtype=F32), np.asarray(B, dtype=F32)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=F32)
    for k in range(A.shape[1]):
        acc = acc + A[:, k, None] * B[None, k, :]
    return acc


def sum_f32(X, axis):
    """Sequential float32 sum along ``axis`` (numpy's own sum is pairwise)."""
    X = np.moveaxis(np.asarray(X, dtype=F32), axis, 0)
    acc = np.zeros(X.shape[1:], dtype=F32)
    for r in range(X.shape[0]):
        acc = acc + X[r]
    return acc

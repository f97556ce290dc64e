"""Host oracle of ONE train launch, per workgroup (CPU only; tests/test_train_stage.py holds the HIP
train kernels to it, tests/test_train_stage_oracle_cpu.py holds the oracle itself).

The train kernel of a shard ``(X, y)`` of n rows at R rows per workgroup writes one slab row per
workgroup b -- rows ``[bR, min((b + 1)R, n))`` of the shard:

* the loss slot: the sum of the block's rows' cross-entropies, divided by the SHARD's n;
* the gradient partial: the block's rows' contribution to the gradient of the shard's mean loss (the
  1/n of the shard, not of the block), ``[n_slabs, P]`` in dense parameter order.

Two models, both in float64:

``exact``
    every operation in float64, written out by hand (no autograd): what the fp32 kernels approximate.
``bf16``
    the bf16 kernels' arithmetic (``reference_oracle._bf16_forward`` / ``_split_bf16_reference_grad``,
    called per block with the shard's n as the divisor): split or plain forward; for the fp32 slab
    the delta of the mean loss rounded to bf16 (``scaled_delta``), for the fp16 slab the unscaled
    delta and unscaled sums (the Adam kernel applies the 1/n), which is what ``slab_partials()``
    returns for such an engine.

``StageRef.margin`` is the case's ReLU margin, ``min |pre-activation| / max |pre-activation|`` over all
hidden units and rows, on the model's own pre-activations.  A GPU case needs at least ``MIN_MARGIN``:
the kernels accumulate in fp32, whose error relative to the largest pre-activation is a few 1e-7, so
no ReLU mask of the device can differ from the oracle's and no row or element is ever excluded from a
comparison."""
from dataclasses import dataclass

import numpy as np
import torch

from .reference_oracle import _bf16_forward, _dense_layers, _split_bf16_reference_grad

MIN_MARGIN = 1e-5

# (rows, F, C, hidden, R): the smallest shards that reach each path of the train kernels
STAGE_CASES = [
    (5, 14, 2, (50, 200), 32),     # reference shape (specialised and generic body), one partial workgroup
    (33, 14, 2, (50, 200), 32),    # a second workgroup of one live row
    (95, 14, 2, (50, 200), 32),    # three workgroups, the last partial
    (33, 14, 2, (50, 200), 16),    # 16 rows per workgroup: always the generic body
    (33, 14, 3, (7,), 32),         # general CE epilogue, one hidden tile
    (95, 14, 5, (33, 17, 9), 16),  # three hidden layers
    (70, 14, 16, (40,), 32),       # FL_MAX_CLASSES
    (40, 1, 2, (16,), 16),         # F = 1
    (70, 17, 3, (16, 16), 32),     # second 16-chunk of features
    (70, 33, 2, (65,), 32),        # second 16-chunk of features, odd hidden tile
]
# bf16 only: 64 rows per workgroup on a model whose split layout fits LDS there
BF16_R64_CASE = (129, 14, 2, (7,), 64)
# the plain-bf16 training forward (an emulated client of several)
# (the 95-row shard's plain model has a ReLU margin of 6.2e-7: not used)
PLAIN_CASE = (33, 14, 2, (50, 200), 32)
# second local step: (rows, F, C, hidden, R)
LOCAL2_CASES = [(33, 14, 2, (50, 200), 32), (95, 14, 5, (33, 17, 9), 16)]


def case_id(case):
    rows, F, C, hidden, R = case
    return f"{rows}x{F}-{'-'.join(map(str, hidden))}-{C}@R{R}"


def block_slices(n, R):
    return [slice(b * R, min((b + 1) * R, n)) for b in range((n + R - 1) // R)]


def tensor_slices(dims):
    """[(name, slice)] of the dense parameter order: W0, b0, W1, b1, ..."""
    out, off = [], 0
    for l in range(len(dims) - 1):
        for name, k in ((f"W{l}", dims[l] * dims[l + 1]), (f"b{l}", dims[l + 1])):
            out.append((name, slice(off, off + k)))
            off += k
    return out


@dataclass
class StageRef:
    loss: np.ndarray    # [n_slabs] float64
    grad: np.ndarray    # [n_slabs, P] float64
    margin: float


def _margin(pre):
    a = torch.cat([p.abs().reshape(-1) for p in pre])
    return float(a.min() / a.max())


def _row_ce(z, y):
    yt = torch.tensor(np.asarray(y), dtype=torch.long)
    return torch.logsumexp(z, 1) - z[torch.arange(len(yt)), yt]


def _exact(flat, X, y, dims, R, n):
    layers = _dense_layers(flat, dims)
    L = len(layers)
    loss, grad, pre_all = [], [], []
    for s in block_slices(len(y), R):  # (block by block: a block's row is bitwise what its rows alone give)
        acts, pre = [torch.tensor(X[s], dtype=torch.float64)], []
        for l, (W, b) in enumerate(layers):
            z = acts[-1] @ W.T + b
            if l + 1 < L:
                pre.append(z)
                acts.append(torch.relu(z))
        yt = torch.tensor(y[s], dtype=torch.long)
        loss.append(float(_row_ce(z, y[s]).sum() / n))
        dz = torch.softmax(z, 1)
        dz[torch.arange(len(yt)), yt] -= 1.0
        dz /= n
        g = [None] * L
        for l in range(L - 1, -1, -1):
            g[l] = torch.cat([(dz.T @ acts[l]).reshape(-1), dz.sum(0)])
            if l:
                dz = (dz @ layers[l][0]) * (pre[l - 1] > 0)
        grad.append(torch.cat(g).numpy())
        pre_all += pre
    return StageRef(np.asarray(loss), np.stack(grad), _margin(pre_all))


def _bf16(flat, X, y, dims, R, n, plain, slab):
    pre, loss, grad = [], [], []
    for s in block_slices(len(y), R):
        z = _bf16_forward(flat, X[s], dims, plain, pre_out=pre)[2]
        loss.append(float(_row_ce(z, y[s]).sum() / n))
        if slab == "fp32":
            g = _split_bf16_reference_grad(flat, X[s], y[s], dims, scaled_delta=True, plain=plain, n_div=n)
        else:
            g = _split_bf16_reference_grad(flat, X[s], y[s], dims, scaled_delta=False, plain=plain, n_div=1)
        grad.append(g)
    return StageRef(np.asarray(loss), np.stack(grad), _margin(pre))


def stage_oracle(flat, X, y, dims, R, model="exact", plain=False, slab="fp32", n=None):
    """Loss slots and gradient partials of every slab row.  ``n``: the mean's divisor (default: the
    rows given; a block's rows alone with the shard's n reproduce that block's slab row).
    ``model="bf16"``: ``plain`` picks the forward, ``slab`` ("fp32" | "fp16") the slab's scaling."""
    X, y = np.asarray(X, np.float32), np.asarray(y)
    n = len(y) if n is None else int(n)
    if model == "exact":
        return _exact(flat, X, y, list(dims), R, n)
    if model != "bf16" or slab not in ("fp32", "fp16"):
        raise ValueError((model, slab))
    return _bf16(flat, X, y, list(dims), R, n, bool(plain), slab)


def fp32_tensor_error(g, ref):
    """The fp32 metric: max|g - ref| / max|ref| over one tensor of one slab row."""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(g - ref).max() / np.abs(ref).max())


def rel_l2(g, ref):
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(g - ref) / np.linalg.norm(ref))

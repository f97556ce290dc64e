"""Record-level DP-SGD (Abadi et al. 2016) on the project's ReLU MLP, in plain torch: the specification of
``fedmi/ops/csrc/fl_train_dpsgd.hip``.

Row ``r``'s weight gradient in layer ``l`` is the outer product ``dZ_{l+1}[r] (x) act_l[r]`` and its bias
gradient ``dZ_{l+1}[r]``, so the norm of its whole gradient needs no per-example gradient ("ghost clipping"):

    ||g_r||^2 = sum over layers l of (1 + ||act_l[r]||^2) * ||dZ_{l+1}[r]||^2

and the clipped sum ``sum_r min(1, C / ||g_r||) g_r / n`` is the ordinary weight gradient of the deltas
scaled row by row.  ``dZ_L = softmax - onehot`` of the UNscaled per-example loss; the ``1 / n`` of the mean
rides the row factor.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from ..models.mlp import param_layout


def ghost_clipped_grad(flat: torch.Tensor, dims: Sequence[int], X: torch.Tensor, y: torch.Tensor,
                       clip: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(norms [n], grad [P], loss)`` in ``flat``'s dtype: every row's pre-clip gradient norm, the dense
    (``named_parameters()`` order) sum of the rows' gradients each clipped to L2 norm ``clip`` and divided by
    ``n``, and the mean cross-entropy."""
    L = len(dims) - 1
    lay = param_layout(dims)
    W = [flat[off:off + shape[0] * shape[1]].view(shape) for _, shape, off in lay[0::2]]
    b = [flat[off:off + shape[0]] for _, shape, off in lay[1::2]]
    n = X.shape[0]
    acts = [X.to(flat.dtype)]
    for l in range(L):
        z = acts[l] @ W[l].T + b[l]
        acts.append(torch.relu(z) if l + 1 < L else z)
    logp = torch.log_softmax(acts[L], 1)
    loss = -logp[torch.arange(n), y].mean()
    dz = [None] * (L + 1)
    dz[L] = torch.exp(logp)
    dz[L][torch.arange(n), y] -= 1.0
    for l in range(L - 1, 0, -1):
        dz[l] = (dz[l + 1] @ W[l]) * (acts[l] > 0).to(flat.dtype)
    s = torch.zeros(n, dtype=flat.dtype, device=flat.device)
    for l in range(L):
        s = s + (1.0 + (acts[l] ** 2).sum(1)) * (dz[l + 1] ** 2).sum(1)
    norms = torch.sqrt(s)
    C = torch.tensor(float(clip), dtype=flat.dtype)
    f = torch.where(s > C * C, C / norms, torch.ones_like(norms)) / n
    grad = torch.empty_like(flat)
    for l in range(L):
        d = dz[l + 1] * f[:, None]
        (_, ws, wo), (_, bs, bo) = lay[2 * l], lay[2 * l + 1]
        grad[wo:wo + ws[0] * ws[1]] = (d.T @ acts[l]).reshape(-1)
        grad[bo:bo + bs[0]] = d.sum(0)
    return norms, grad, loss

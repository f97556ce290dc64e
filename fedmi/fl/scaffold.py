"""SCAFFOLD (Karimireddy et al. 2020), option I: control-variate drift correction of the local steps.

Client ``i`` keeps a control variate ``c_i``, every replica the server variate ``c``; both start at 0 and live in
dense parameter order.  In a live round in which client ``i`` is sampled:

* ``g0 = grad f_i(x)``: the full-batch gradient at the model ``x`` the round trains from (local step 0's);
* every local step's optimizer sees ``g + (c - c_i)``, with ``c`` and ``c_i`` as they were at the round's start
  (weight decay and the FedProx term are added after that, as without it);
* ``cnew_i = g0``, ``delta_i = cnew_i - c_i`` stay pending until the model is aggregated; then, with ``s`` the left
  fold from +0, in client order, of ``delta_j`` over the round's sampled clients, ``c <- c + s / N`` (``N`` = all
  clients, not the sampled count) and every sampled client commits ``c_i <- c_i + delta_i``.

The commit is the addition ``c`` takes, not a copy of ``cnew_i``: in floating point ``c_i + (g0 - c_i)`` is ``g0`` only
where the subtraction is exact, so a copy leaves ``c`` and the ``c_i`` one rounding apart after the first round even
where all clients hold the same shard.  Committed by the addition, ``c`` and ``c_i`` move by the same operations: on
equal shards with a power-of-two client count ``c == c_i`` bit for bit, the correction is exactly 0 and the round is
the plain round's.  ``c_i`` stays within one rounding of ``g0``; the error does not accumulate, every round's delta being
taken from ``g0`` anew.

Option I does not depend on the local optimizer (here Adam).  The model aggregate keeps its sample-size weights; a
global step size is ``server_opt="sgd"`` with ``server_momentum=0``.

:func:`scaffold_fold` is the rule for the torch engines (fp32) and, on float64 tensors, the oracle;
:func:`scaffold_grad_model` / :func:`scaffold_capture_model` / :func:`scaffold_fold_model` reproduce the two HIP
kernels (``fedmi/ops/csrc/fl_scaffold.hip``) bit for bit in numpy fp32.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

MAX_SCAFFOLD_CLIENTS = 64   # the width of the sampled-client mask (fl_common.h FL_SCAFFOLD_MAX_K)
_ROWS = 16                  # row partials per position of the capture kernel (FL_SCAFFOLD_ROWS)


def scaffold_enabled(cfg, world: Optional[int] = None) -> bool:
    """Validate ``cfg.scaffold`` against what it does not combine with; True when the correction is on.
    ``world``: the federation's size when the caller knows it -- with one client there is no drift to correct,
    so the feature is off and nothing is refused."""
    if not bool(getattr(cfg, "scaffold", False)) or (world is not None and int(world) <= 1):
        return False
    no = lambda why: ValueError(f"scaffold does not run with {why}")
    if cfg.dtype == "bf16":
        raise no("dtype='bf16': the fp16 gradient slab cannot carry the correction row c - c_i")
    if float(cfg.dpsgd_clip) > 0.0:
        raise no("record-level DP-SGD (dpsgd_clip > 0): the captured step-0 gradient is unclipped")
    if float(cfg.dp_clip) > 0.0:
        raise no("differential privacy (dp_clip > 0): the control variates leave the client un-noised")
    if bool(cfg.secagg):
        raise no("secagg: the control fold needs every client's delta, secure aggregation opens only a sum")
    if cfg.aggregator != "mean":
        raise no(f"aggregator={cfg.aggregator!r}: the control fold is a plain mean a robust rule does not protect")
    if cfg.screen != "none":
        raise no(f"screen={cfg.screen!r}: the control fold takes every sampled client, screened or not")
    if cfg.attack != "none":
        raise no(f"attack={cfg.attack!r}: the attack models rewrite model contributions, not control variates")
    if cfg.compress != "none":
        raise no(f"compress={cfg.compress!r}: the deltas would travel dense beside a compressed update")
    if world is not None and int(world) > MAX_SCAFFOLD_CLIENTS:
        raise no(f"more than {MAX_SCAFFOLD_CLIENTS} clients (the width of the sampled-client mask), got {int(world)}")
    return True


def scaffold_fold(c: torch.Tensor, deltas: Sequence[torch.Tensor], sampled: Sequence[bool], n_clients: int) -> torch.Tensor:
    """The new server variate in ``c``'s dtype: ``c + s / N``, ``s`` the left fold from +0 in client order of the
    sampled clients' ``deltas`` (an unsampled client's entry is never read)."""
    s = torch.zeros_like(c)
    for d, on in zip(deltas, sampled):
        if on:
            s = s + d.to(c.dtype)
    return c + s / torch.tensor(float(n_clients), dtype=c.dtype)


def scaffold_grad_model(rows: np.ndarray) -> np.ndarray:
    """fp32 column sums of the slab rows ``rows`` [n_blk, P] in the capture kernel's order: partial ``r`` of 16 adds
    rows r, r + 16, ... in ascending order from +0, then the partials are added in ``r`` order from +0."""
    rows = np.asarray(rows, np.float32)
    g = np.zeros(rows.shape[1], np.float32)
    for r in range(_ROWS):
        acc = np.zeros(rows.shape[1], np.float32)
        for k in range(r, rows.shape[0], _ROWS):
            acc = acc + rows[k]
        g = g + acc
    return g


def scaffold_capture_model(rows: np.ndarray, c: np.ndarray, ci: np.ndarray):
    """(cnew, delta, correction row) of the capture kernel, fp32 bit for bit."""
    c, ci = np.asarray(c, np.float32), np.asarray(ci, np.float32)
    g = scaffold_grad_model(rows)
    return g, g - ci, c - ci


def scaffold_fold_model(c: np.ndarray, deltas: np.ndarray, sampled: Sequence[bool], n_clients: int) -> np.ndarray:
    """The fold kernel's new ``c`` from the [K, P] stack ``deltas``, fp32 bit for bit."""
    c, deltas = np.asarray(c, np.float32), np.asarray(deltas, np.float32)
    s = np.zeros_like(c)
    for k, on in enumerate(sampled):
        if on:
            s = s + deltas[k]
    return c + s / np.float32(n_clients)

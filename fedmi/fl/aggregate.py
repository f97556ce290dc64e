"""Byzantine-robust aggregation rules: the coordinate-wise median and beta-trimmed mean of Yin et
al. 2018 ("Byzantine-Robust Distributed Learning: Towards Optimal Statistical Rates").

With ``K_r`` clients sampled in a round and ``v_k[c]`` client k's unscaled post-step local model
at coordinate c:

* ``t = (K_r - 1) // 2`` for the median (1 value kept for odd ``K_r``, the 2 middle ones for even),
  ``t = floor(beta * K_r)`` for the trimmed mean (never more than the median's), :func:`trim_count`;
* the ``K_r`` values of a coordinate are ordered by the total order "any NaN above +inf, otherwise
  by value; ties, -0 / +0 included, by client index";
* the ``t`` lowest and ``t`` highest are dropped, the kept ones summed in client order starting from
  0 with one rounding per addition, and the sum divided once by ``K_r - 2 t``.

The aggregate is unweighted: sample sizes are self-reported, and a weighted median is not what the
paper analyses.  :func:`robust_aggregate_torch` is that rule in the tensors' dtype: in fp32 a
bit-exact model of the HIP kernel (``fedmi/ops/csrc/fl_robust.hip``), in float64 the oracle's
arithmetic.
"""
from __future__ import annotations

import math
from typing import Sequence

import torch

AGGREGATORS = ("mean", "median", "trimmed_mean")
MAX_ROBUST_CLIENTS = 64   # width of the per-round sampled-client mask (fl_common.h FL_ROBUST_MAX_K)


def trim_count(kind: str, beta: float, k_r: int) -> int:
    """Values cut at EACH end of ``k_r`` >= 1 sampled clients; ``2 t < k_r`` always."""
    k_r = int(k_r)
    if k_r < 1:
        raise ValueError(f"trim_count: needs at least one sampled client, got {k_r}")
    med = (k_r - 1) // 2
    if kind == "median":
        return med
    if kind != "trimmed_mean":
        raise ValueError(f"trim_count: kind must be 'median' or 'trimmed_mean', got {kind!r}")
    beta = float(beta)
    if not (math.isfinite(beta) and 0.0 <= beta < 0.5):
        raise ValueError(f"trim_ratio must be a finite number in [0, 0.5), got {beta!r}")
    return min(int(math.floor(beta * float(k_r))), med)


class _AggLaunch:
    """The Python-launched aggregation kernels (``robust_aggregate``, ``secagg_mask``, ``secagg_open``) of
    one federation, over buffers that keep their addresses.  ``lead``: the engine whose dims, round
    state, ``rtab`` and config every launch uses (identical on all clients); ``src[par]`` / ``dst[par]``:
    the source and destination buffers of a round of output parity ``par``; :meth:`mask` masks the
    destinations in place -- what a process publishes is where it receives the aggregate -- as clients
    ``first_client ..`` with the clamp histories ``clamps``.  Owns the device pointer tables."""

    def __init__(self, lead, src, dst, clamps=(), first_client: int = 0):
        def table(ts):
            return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=lead.device)
        self._lead, self._bufs = lead, (src, dst, clamps)   # (the tables hold addresses: keep the buffers)
        self._k, self._n, self._first = len(src[0]), len(dst[0]), int(first_client)
        self._src = [table(s) for s in src]
        self._dst = self._src if dst is src else [table(s) for s in dst]
        self._clamp = table(clamps)

    def _round(self, par: int):
        e = self._lead
        return e.state[par].data_ptr(), e.rtab.data_ptr()

    def robust(self, par: int, stream: int) -> None:
        e = self._lead
        e.m.robust_aggregate(e.dims, e.robust, float(e.cfg.trim_ratio), self._src[par].data_ptr(), self._k,
                             self._dst[par].data_ptr(), self._n, *self._round(par), self._k * e.tail_stride,
                             int(e.cfg.max_rounds), stream)

    def mask(self, par: int, stream: int) -> None:
        e = self._lead
        e.m.secagg_mask(e.dims, int(e.cfg.secagg_bits), e.secagg_seed, self._dst[par].data_ptr(), self._n, self._first,
                        *self._round(par), self._clamp.data_ptr(), int(e.cfg.max_rounds), stream)

    def open(self, par: int, stream: int) -> None:
        e = self._lead
        e.m.secagg_open(e.dims, int(e.cfg.secagg_bits), self._src[par].data_ptr(), self._k, self._dst[par].data_ptr(),
                        self._n, *self._round(par), self._k * e.tail_stride, int(e.cfg.max_rounds), stream)


def _sort_keys(stack: torch.Tensor) -> torch.Tensor:
    """int64 keys whose order is the total order of the values: NaN above +inf, -0 == +0."""
    stack = stack.contiguous()
    if stack.dtype == torch.float32:
        bits, mag = stack.view(torch.int32).to(torch.int64), 0x7FFFFFFF
    else:
        bits, mag = stack.view(torch.int64), 0x7FFFFFFFFFFFFFFF
    key = torch.where(bits < 0, -(bits & mag), bits)   # sign-magnitude -> two's complement; -0 -> 0
    return torch.where(torch.isnan(stack), torch.full_like(key, mag), key)


def robust_aggregate_torch(stack: torch.Tensor, active_mask: Sequence[bool], kind: str, beta: float) -> torch.Tensor:
    """Coordinate-wise median / trimmed mean of the rows of ``stack`` [K, P] whose ``active_mask``
    entry is true, in ``stack``'s dtype (float32 or float64), by the rule of the module docstring."""
    if stack.dim() != 2 or stack.dtype not in (torch.float32, torch.float64):
        raise ValueError("robust_aggregate_torch: needs a [K, P] float32 or float64 tensor")
    K = int(stack.shape[0])
    act = [bool(a) for a in active_mask]
    if len(act) != K:
        raise ValueError(f"robust_aggregate_torch: {len(act)} mask entries for {K} clients")
    k_r = sum(act)
    t = trim_count(kind, beta, k_r)
    key = _sort_keys(stack)
    rank = torch.zeros_like(key)
    for i in range(K):
        if not act[i]:
            continue
        for j in range(K):
            if j != i and act[j]:
                before = (key[j] <= key[i]) if j < i else (key[j] < key[i])
                rank[i] += before.to(rank.dtype)
    acc = torch.zeros(stack.shape[1], dtype=stack.dtype, device=stack.device)
    for i in range(K):
        if act[i]:
            keep = (rank[i] >= t) & (rank[i] < k_r - t)
            acc = torch.where(keep, acc + stack[i], acc)
    return acc / torch.tensor(float(k_r - 2 * t), dtype=stack.dtype, device=stack.device)

"""Secure aggregation: pairwise-masked fixed-point FedAvg contributions -- the rule and its host model.

Bonawitz et al. 2017 ("Practical Secure Aggregation for Privacy-Preserving Machine Learning"): every
pair of a round's sampled clients shares a mask that one adds and the other subtracts, so each
contribution on the wire is uniformly distributed while the masks cancel in the sum.  With
``EngineConfig.secagg`` the parameter image a peer receives (the host gather, the k buffers of a
:class:`~fedmi.fl.simulate.ClientGroup`) carries these masked integers instead of the clear weighted
model; with differential privacy on, the distributed-noise guarantee then applies to what peers see.

This is a SIMULATION of the protocol's arithmetic, not of its key exchange: all pair masks derive
from ONE shared group seed, so whoever knows the seed can unmask.  Out of scope:

* Diffie-Hellman key agreement.
* Secret-sharing recovery of dropped clients.
* The malicious-server rounds.

Metric tails (confusion counts and loss) stay in the clear as floats: per-client metrics are part of
the product's console and history.

The rule (``fedmi/ops/csrc/fl_secagg.hip`` is bit-exact against the functions below), for a live
round ``r`` with sampled set ``P_r`` (the per-round table's mask), ``K_r = |P_r|``, ``F = secagg_bits``
and ``c_i[p]`` sampled client ``i``'s weighted fp32 contribution at dense parameter ``p`` (what the
Adam, DP or compression kernel left in the FedAvg buffer)::

    quantise   L = floor((2^31 - 1) / K_r)
               q_i[p] = clamp(round_half_even(c_i[p] * 2^F), -L, L)       +-inf -> +-L, NaN -> 0
               (every clamped or NaN coordinate is counted; |q| <= L, so the true sum cannot wrap)
    mask       y_i[p] = q_i[p] + sum_{j in P_r, j > i} m(i, j)[p] - sum_{j in P_r, j < i} m(j, i)[p]   mod 2^32
               m(a, b)[p] = word p % 4 of Philox4x32-10 at counter (p // 4, r, 64 a + b, SECAGG_STREAM)
                            under the key seed_key(secagg_seed)
    open       S[p] = sum_{i in P_r} y_i[p] mod 2^32;  aggregate = float(int32(S[p])) * 2^-F

``y_i`` is stored as its bit pattern at the parameter's image position; image padding keeps the bits
of +0 and opens to exact 0 whatever the sources hold.  The opened image does not depend on the seed,
and against the float64 sum ``ref`` of the fp32 contributions ``|opened - ref| <= K_r 2^-(F+1) +
2^-24 |ref|`` (K_r roundings to the grid, one int-to-float rounding) where nothing clamped.

An unsampled client and a round that is not live are not touched by the mask step (a round that is
not live opens as the fp32 left fold of the whole buffers, as the robust aggregators' does).  With
``K_r = 1`` there is no pair: the lone client's quantised value travels UNMASKED.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

from ..privacy.philox import DP_STREAM, philox4x32_10, seed_key

SECAGG_STREAM = 0x47414353   # fourth counter word of the pair masks ("SCAG"); the DP noise uses DP_STREAM
assert SECAGG_STREAM != DP_STREAM
SECAGG_MIN_BITS, SECAGG_MAX_BITS = 8, 30
MAX_SECAGG_CLIENTS = 64      # width of the sampled-client mask; the pair counter word is 64 a + b


def _bits(bits) -> int:
    if isinstance(bits, (bool, np.bool_)) or not isinstance(bits, (int, np.integer)) \
            or not SECAGG_MIN_BITS <= int(bits) <= SECAGG_MAX_BITS:
        raise ValueError(f"secagg_bits must be an integer in [{SECAGG_MIN_BITS}, {SECAGG_MAX_BITS}], got {bits!r}")
    return int(bits)


def secagg_id(cfg) -> int:
    """Validate the secure-aggregation fields of an ``EngineConfig``; 1 when it is on, else 0."""
    if not isinstance(cfg.secagg, (bool, np.bool_)):
        raise ValueError(f"secagg must be a bool, got {cfg.secagg!r}")
    _bits(cfg.secagg_bits)
    s = cfg.secagg_seed
    if s is not None and (isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer))
                          or not 0 <= int(s) < 2 ** 64):
        raise ValueError(f"secagg_seed must be None or an integer in [0, 2**64), got {s!r}")
    return int(bool(cfg.secagg))


def secagg_limit(kr: int) -> int:
    """``L = floor((2^31 - 1) / K_r)``: the largest |q| of one of K_r contributions."""
    return (2 ** 31 - 1) // int(kr)


def secagg_quantize(c, bits: int, kr: int) -> Tuple[np.ndarray, int]:
    """``(q, clamped)``: the fixed-point image of the fp32 contribution ``c`` (int32) and the number
    of clamped or NaN coordinates.  The scaling is a power of two, so in float64 it is exact."""
    bits, L = _bits(bits), secagg_limit(kr)
    x = np.asarray(c, np.float32).astype(np.float64) * 2.0 ** bits
    nan = np.isnan(x)
    r = np.rint(np.where(nan, 0.0, x))   # half to even
    over = np.abs(r) > L
    q = np.clip(r, -L, L).astype(np.int64).astype(np.int32)
    return q, int(nan.sum() + over.sum())


def pair_mask(a: int, b: int, r: int, n_params: int, seed: int) -> np.ndarray:
    """``m(a, b)`` of round ``r`` over dense parameters ``0 .. n_params - 1``: uint32."""
    nq = (int(n_params) + 3) // 4
    ctr = np.empty((nq, 4), np.uint64)
    ctr[:, 0] = np.arange(nq, dtype=np.uint64)
    ctr[:, 1] = int(r) & 0xFFFFFFFF
    ctr[:, 2] = 64 * int(a) + int(b)
    ctr[:, 3] = SECAGG_STREAM
    return philox4x32_10(ctr, seed_key(seed)).reshape(-1)[:int(n_params)]


def secagg_mask(q, i: int, sampled: Sequence[int], r: int, seed: int) -> np.ndarray:
    """``y_i``: sampled client ``i``'s quantised contribution ``q`` (int32, dense order) under the pair
    masks of round ``r``'s sampled set, as uint32 (mod 2^32)."""
    q = np.asarray(q)
    if q.dtype != np.int32:
        raise ValueError(f"secagg_mask takes the int32 output of secagg_quantize, got {q.dtype}")
    i, sampled = int(i), sorted(int(j) for j in sampled)
    if i not in sampled or sampled[0] < 0 or sampled[-1] >= MAX_SECAGG_CLIENTS:
        raise ValueError(f"client {i} is not in the sampled set {sampled} of clients 0 .. {MAX_SECAGG_CLIENTS - 1}")
    y = q.reshape(-1).view(np.uint32).copy()
    with np.errstate(over="ignore"):
        for j in sampled:
            if j > i:
                y += pair_mask(i, j, r, y.size, seed)
            elif j < i:
                y -= pair_mask(j, i, r, y.size, seed)
    return y


def secagg_open(ys, bits: int) -> np.ndarray:
    """The aggregate of the sampled clients' masked rows ``ys`` ([K_r, P] uint32): fp32."""
    bits = _bits(bits)
    ys = np.asarray(ys)
    if ys.dtype != np.uint32 or ys.ndim != 2:
        raise ValueError("secagg_open takes a [K_r, P] uint32 stack")
    with np.errstate(over="ignore"):
        S = ys.sum(axis=0, dtype=np.uint32)
    return S.view(np.int32).astype(np.float32) * np.float32(2.0 ** -bits)


def secagg_round(cs, sampled: Sequence[int], r: int, bits: int, seed: int):
    """The whole rule for one live round on the host: ``cs[i]`` the dense fp32 contribution of client
    ``i`` (rows of unsampled clients are ignored).  Returns ``(opened fp32 [P], masked rows {i: uint32
    [P]}, clamp counts {i: int})``."""
    sampled = sorted(int(j) for j in sampled)
    ys, counts = {}, {}
    for i in sampled:
        q, counts[i] = secagg_quantize(cs[i], bits, len(sampled))
        ys[i] = secagg_mask(q, i, sampled, r, seed)
    return secagg_open(np.stack([ys[i] for i in sampled]), bits), ys, counts

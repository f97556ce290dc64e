"""Host model (numpy) of the differential-privacy noise stream of the HIP round engine.

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"; Random123) with the
counter / key layout of ``fedmi/ops/csrc/fl_dp.hip``: dense parameter ``p``
(``named_parameters()`` order) draws lane ``p % 4`` of the block at counter
``(p // 4, round, rank, 0x46454450)`` under the key ``(seed & 0xffffffff, seed >> 32)``.  Each
32-bit output ``o`` maps to ``u = ((o >> 8) + 0.5) / 2**24`` evaluated in fp32 like the device's
``u01`` (exact below 0.5, rounded to 24 bits above), then Box-Muller in float64: the pair
``(u0, u1)`` gives lanes 0 and 1 (``sqrt(-2 ln u0)`` times ``cos`` / ``sin`` of ``2 pi u1``), the
pair ``(u2, u3)`` lanes 2 and 3.
"""
from __future__ import annotations

import numpy as np

DP_STREAM = 0x46454450
# Streams of the stochastic update compressors (fedmi/fl/compress.py; FL_QSGD_STREAM / FL_RANDK_STREAM of
# fedmi/ops/csrc/fl_common.h): same counter layout, the words used as they come (param_words)
QSGD_STREAM = 0x44475351
RANDK_STREAM = 0x4B444E52
# Stream of the Gaussian Byzantine client (fedmi/fl/attack.py; FL_ATTACK_STREAM of fl_common.h, "ATCK"): the DP
# layout with the bad client's index in the rank word, Box-Muller normals like the DP noise.  Distinct from the
# streams above and from the pair masks' (fedmi/fl/secagg.py SECAGG_STREAM = 0x47414353).
ATTACK_STREAM = 0x4B435441
assert len({DP_STREAM, QSGD_STREAM, RANDK_STREAM, ATTACK_STREAM, 0x47414353}) == 5
_M0 = np.uint64(0xD2511F53)
_M1 = np.uint64(0xCD9E8D57)
_W0 = 0x9E3779B9
_W1 = 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 of ``counter`` ([..., 4] uint32 words) under ``key`` (two uint32 words):
    the four output words per counter, uint32 ``[..., 4]``."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _MASK, n2, p0 & _MASK
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u01(o) -> np.ndarray:
    """The device's ``u01``: ``((o >> 8) + 0.5) * 2**-24`` in fp32 arithmetic, as float64."""
    x = (np.asarray(o, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return ((x + np.float32(0.5)) * np.float32(1.0 / 16777216.0)).astype(np.float64)


def box_muller(o: np.ndarray) -> np.ndarray:
    """Four standard normals per Philox block ``o`` ([..., 4] uint32), float64."""
    u = u01(o)
    out = np.empty(u.shape, np.float64)
    for a in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u[..., a]))
        ang = 2.0 * np.pi * u[..., a + 1]
        out[..., a] = rad * np.cos(ang)
        out[..., a + 1] = rad * np.sin(ang)
    return out


def seed_key(seed: int):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def param_words(n_params: int, round_index: int, rank: int, seed: int, stream: int) -> np.ndarray:
    """The 32-bit word of dense parameters ``0 .. n_params - 1`` for (round, rank) on ``stream``:
    parameter ``p`` takes word ``p % 4`` of the block at counter ``(p // 4, round, rank, stream)``
    under ``seed_key(seed)``; uint32."""
    n_params = int(n_params)
    nq = (n_params + 3) // 4
    ctr = np.empty((nq, 4), np.uint64)
    ctr[:, 0] = np.arange(nq, dtype=np.uint64)
    ctr[:, 1] = int(round_index) & 0xFFFFFFFF
    ctr[:, 2] = int(rank) & 0xFFFFFFFF
    ctr[:, 3] = int(stream) & 0xFFFFFFFF
    return philox4x32_10(ctr, seed_key(seed)).reshape(-1)[:n_params]


def dp_normals(n_params: int, round_index: int, rank: int, seed: int) -> np.ndarray:
    """Standard normals of dense parameters ``0 .. n_params - 1`` for (round, rank): float64."""
    n_params = int(n_params)
    nq = (n_params + 3) // 4
    ctr = np.empty((nq, 4), np.uint64)
    ctr[:, 0] = np.arange(nq, dtype=np.uint64)
    ctr[:, 1] = int(round_index) & 0xFFFFFFFF
    ctr[:, 2] = int(rank) & 0xFFFFFFFF
    ctr[:, 3] = DP_STREAM
    return box_muller(philox4x32_10(ctr, seed_key(seed))).reshape(-1)[:n_params]

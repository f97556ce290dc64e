"""Update compression with error feedback: the rule, a host model of the kernel, wire-size accounting.

A client's round update is compressed before it enters the FedAvg exchange (top-k sparsification with
memory, Stich et al. 2018; scaled sign with error feedback, Karimireddy et al. 2019; stochastic
quantisation, QSGD, Alistarh et al. 2017; random-k sparsification).  This is a
SIMULATION of a compressed uplink: the exchange still carries the dense fp32 image (a 45 KB image is
latency-bound, not bandwidth-bound, on xGMI); what changes is the information in it, and
:func:`uplink_bytes` reports what a real uplink would have carried.

The rule, per client, in a live round in which the client is sampled (FedAvg weight ``w != 0``), on
the P real parameters, every operation an fp32 round-to-nearest one (``fedmi/ops/csrc/fl_compress.hip``)::

    u  = (local - x) + e                   x = the image the round trained from, e = residual (0 at start)
    c  = C(u)
    e' = error_feedback ? (kept ? 0 : u - c) : 0
    contribution = w * (x + c)

* ``"topk"``: ``k = max(1, min(P, ceil(compress_ratio * P)))``; order by the unsigned integer image of
  ``|u|`` (``bits & 0x7fffffff``, so any NaN ranks above inf), larger first, ties by lower dense
  (``named_parameters()`` order) index; exactly k entries are kept with ``c = u``, the rest have
  ``c = 0`` and ``e' = u``.
* ``"sign"``: ``s = (sum |u|) / P`` summed in the kernel's fixed order (:func:`sign_scale`),
  ``c = copysign(s, u)``; nothing is kept, ``e' = u - c``.

The two random compressors draw, for dense parameter ``p`` of round ``r`` of client ``i``, word
``p % 4`` of Philox4x32-10 at counter ``(p // 4, r, i, STREAM)`` under ``seed_key(compress_seed)``
(``fedmi/privacy/philox.py`` ``param_words``; ``QSGD_STREAM`` / ``RANDK_STREAM``):

* ``"qsgd"`` (one bucket = the whole model, ``s = compress_levels``): ``norm = sqrt(sum u * u)`` summed in
  the sign compressor's fixed order (:func:`qsgd_norm`).  ``norm`` 0 or not finite: ``c = u``, ``e' = 0``
  (the round travels as it is).  Otherwise ``a = min((|u| / norm) * s, s)``, ``l = floor(a)``,
  ``level = l + ((word >> 8) < (a - l) * 2**24)`` and ``c = copysign((norm * level) / s, u)``: unbiased,
  ``E c = u``.  Nothing is kept, ``e' = u - c``.
* ``"randk"``: ``k`` as for top-k; order by ``key31 = word >> 1``, larger first, ties by lower dense
  index; exactly k entries are kept.  The indices follow from the shared seed alone, so only the k
  values travel.  The variant is COUPLED to ``error_feedback``: with it (the memory variant of Stich
  et al.) kept entries send ``c = u`` and ``e' = kept ? 0 : u``; without it kept entries send
  ``c = u * (P / k)`` (the unbiased variant, ``E c = u``) and ``e' = 0``.  A gain together with a
  memory would count the dropped mass twice.

An unsampled client and a round that is not live leave contribution and residual untouched.  Top-k and
sign are deterministic: every replica and every graph replay is bit-identical.  The random compressors
are deterministic given ``(compress_seed, round, client)``: the round word comes from the device state,
so a replayed graph draws fresh words each round, and a resumed run continues the stream.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

COMPRESSORS = ("none", "topk", "sign")
# stochastic compressors: their output depends on (compress_seed, round, client)
RANDOM_COMPRESSORS = ("qsgd", "randk")
ALL_COMPRESSORS = COMPRESSORS + RANDOM_COMPRESSORS
MAX_LEVELS = 32767
# threads of the kernel's workgroup: the fixed summation order of `s` follows them
_THREADS = 1024


def compress_id(cfg) -> int:
    """Validate the compression fields of an ``EngineConfig``; the compressor's index in
    ``ALL_COMPRESSORS`` (0 = off)."""
    if cfg.compress not in ALL_COMPRESSORS:
        raise ValueError(f"compress must be one of {ALL_COMPRESSORS}, got {cfg.compress!r}")
    try:
        ratio = float(cfg.compress_ratio)
    except (TypeError, ValueError):
        ratio = math.nan
    if not (math.isfinite(ratio) and 0.0 < ratio <= 1.0):
        raise ValueError(f"compress_ratio must be a finite number in (0, 1], got {cfg.compress_ratio!r}")
    if not isinstance(cfg.error_feedback, (bool, np.bool_)):
        raise ValueError(f"error_feedback must be a bool, got {cfg.error_feedback!r}")
    levels = getattr(cfg, "compress_levels", 127)
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (int, np.integer)) or not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f"compress_levels must be an integer in [1, {MAX_LEVELS}], got {levels!r}")
    seed = getattr(cfg, "compress_seed", None)
    if seed is not None and (isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer))
                             or not 0 <= int(seed) < 2 ** 64):
        raise ValueError(f"compress_seed must be None or an integer in [0, 2**64), got {seed!r}")
    kind = ALL_COMPRESSORS.index(cfg.compress)
    if kind and float(cfg.dp_clip) > 0.0:
        raise ValueError(f"compress={cfg.compress!r} does not combine with differential privacy (dp_clip > 0): "
                         "both rewrite the contribution, and the noise calibration assumes the clipped update")
    return kind


def topk_count(ratio: float, P: int) -> int:
    """Entries top-k keeps of P parameters: ``max(1, min(P, ceil(ratio * P)))``."""
    return max(1, min(int(P), int(math.ceil(float(ratio) * int(P)))))


def compress_k(cfg, P: int) -> int:
    """Entries a config's compressor transmits of P parameters (sign, qsgd and dense: all P)."""
    return topk_count(cfg.compress_ratio, P) if cfg.compress in ("topk", "randk") else int(P)


def qsgd_code_bits(levels: int) -> int:
    """Width of QSGD's fixed-width sign-and-level code: ``ceil(log2(2 s + 1))`` bits."""
    return (2 * int(levels)).bit_length()   # 2 s + 1 codes: the smallest b with 2**b >= 2 s + 1


def uplink_bytes(kind: str, k: int, P: int, levels: int = 127) -> int:
    """Bytes a real uplink would carry per client and round: top-k ``8 k`` (an fp32 value and an int32
    index per kept entry), sign ``4 + ceil(P / 8)`` (the fp32 scale and one bit per coordinate), qsgd
    ``4 + ceil(P * ceil(log2(2 s + 1)) / 8)`` (the fp32 norm and a fixed-width sign-and-level code per
    coordinate; no Elias coding), randk ``4 k`` (the values only: the indices follow from the shared
    seed), dense ``4 P``."""
    if kind not in ALL_COMPRESSORS:
        raise ValueError(f"compress must be one of {ALL_COMPRESSORS}, got {kind!r}")
    if kind == "topk":
        return 8 * int(k)
    if kind == "sign":
        return 4 + (int(P) + 7) // 8
    if kind == "qsgd":
        return 4 + (int(P) * qsgd_code_bits(levels) + 7) // 8
    if kind == "randk":
        return 4 * int(k)
    return 4 * int(P)


def _vec(t) -> torch.Tensor:
    """A flat CPU vector in fp32 (the kernel's arithmetic), or in float64 where the caller passes
    float64 (the same rule without fp32 roundings: derivations, telescoping checks)."""
    t = torch.as_tensor(t)
    dt = torch.float64 if t.dtype == torch.float64 else torch.float32
    return t.detach().to(device="cpu", dtype=dt).reshape(-1).contiguous()


def _keys(u: torch.Tensor) -> np.ndarray:
    """Unsigned integer image of |u| (sign bit cleared): orders magnitudes, any NaN above inf."""
    if u.dtype == torch.float64:
        return (u.numpy().view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)).astype(np.int64)
    return (u.numpy().view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)


def ordered_sum(a: np.ndarray):
    """The sum of the vector ``a`` (fp32 or float64, non-negative terms or NaN) in the kernel's order:
    thread t of 1024 adds its entries t, t + 1024, ... in turn, an xor tree (offsets 32, 16, ... 1) sums
    each 64-lane wave, the 16 wave sums are added in wave order."""
    a = np.ascontiguousarray(a).reshape(-1)
    P, ft = a.shape[0], a.dtype.type
    per = (P + _THREADS - 1) // _THREADS
    pad = np.zeros(per * _THREADS, ft)
    pad[:P] = a
    acc = np.zeros(_THREADS, ft)
    with np.errstate(invalid="ignore", over="ignore"):
        for row in pad.reshape(per, _THREADS):   # (adding the padding's +0 changes no bit: the terms are >= +0)
            acc = acc + row
        lanes = acc.reshape(_THREADS // 64, 64)
        idx = np.arange(64)
        off = 32
        while off:
            lanes = lanes + lanes[:, idx ^ off]
            off >>= 1
        ss = ft(0.0)
        for wsum in lanes[:, 0]:
            ss = ft(ss + wsum)
    return ss


def sign_scale(u):
    """``(sum |u|) / P`` in the kernel's order (:func:`ordered_sum`), one division by ``float(P)``."""
    a = np.abs(_vec(u).numpy())
    ft = a.dtype.type
    return ft(ordered_sum(a) / ft(a.shape[0]))


def qsgd_norm(u):
    """``sqrt(sum u * u)`` in the kernel's order (:func:`ordered_sum`): every product rounded once,
    one square root."""
    a = _vec(u).numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        return a.dtype.type(np.sqrt(ordered_sum(a * a)))


def topk_mask(u, k: int) -> torch.Tensor:
    """Boolean mask of the k entries top-k keeps (magnitude key, larger first; ties: lower index)."""
    return _largest_mask(_keys(_vec(u)), k)


def _largest_mask(key: np.ndarray, k: int) -> torch.Tensor:
    order = np.argsort(-key, kind="stable")
    kept = np.zeros(key.shape[0], bool)
    kept[order[:int(k)]] = True
    return torch.as_tensor(kept)


def compress_words(kind: str, P: int, seed: int, round: int, client: int) -> np.ndarray:
    """The 32-bit Philox word of every dense parameter for a random compressor (uint32 ``[P]``)."""
    from ..privacy.philox import QSGD_STREAM, RANDK_STREAM, param_words
    if kind not in RANDOM_COMPRESSORS:
        raise ValueError(f"compress_words: kind must be one of {RANDOM_COMPRESSORS}, got {kind!r}")
    return param_words(P, round, client, seed, QSGD_STREAM if kind == "qsgd" else RANDK_STREAM)


def randk_keys(P: int, seed: int, round: int, client: int) -> np.ndarray:
    """``key31 = word >> 1`` of every dense parameter (int64 ``[P]``): rand-k keeps the k largest."""
    return (compress_words("randk", P, seed, round, client) >> np.uint32(1)).astype(np.int64)


def randk_mask(P: int, k: int, seed: int, round: int, client: int) -> torch.Tensor:
    """Boolean mask of the k entries rand-k keeps (``key31``, larger first; ties: lower index)."""
    return _largest_mask(randk_keys(P, seed, round, client), k)


def qsgd_levels(u, levels: int, norm, words: np.ndarray) -> np.ndarray:
    """The integer level in ``[0, s]`` of every entry of ``u`` (finite, ``norm`` finite and > 0), in
    ``u``'s float type."""
    a = _vec(u).numpy()
    ft = a.dtype.type
    s = ft(int(levels))
    lv = np.minimum((np.abs(a) / ft(norm)) * s, s)
    low = np.floor(lv)
    frac = lv - low                                              # exact
    up = (words >> np.uint32(8)).astype(ft) < frac * ft(2.0 ** 24)
    return low + up.astype(ft)


def compress_torch(u, kind: str, k: int = 0, error_feedback: bool = True,
                   s: Optional[float] = None, *, levels: int = 127, seed: int = 0, round: int = 0,
                   client: int = 0, norm: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """``(c, e', stat)`` of the vector ``u`` (fp32, or float64 kept as float64): the compressed update,
    the new residual and the round's statistic (top-k: the magnitude of the k-th kept entry; sign: the
    scale ``s``; qsgd: the norm; randk: ``key31`` of the k-th kept entry times ``2**-31``, the selection's
    quantile).  In fp32 a bit-exact model of the kernel given the same ``u`` and, for sign / qsgd, the same
    ``s`` / ``norm`` (``None``: the host model of the kernel's sum, :func:`sign_scale` / :func:`qsgd_norm`).
    The random kinds draw the words of ``(seed, round, client)``."""
    u = _vec(u)
    P = u.numel()
    if kind == "topk":
        if not 1 <= int(k) <= P:
            raise ValueError(f"k must be in 1 .. {P}, got {k!r}")
        kept = topk_mask(u, k)
        zero = torch.zeros_like(u)
        c = torch.where(kept, u, zero)
        e = torch.where(kept, zero, u)
        fin = u[kept][~torch.isnan(u[kept])]   # (NaN ranks first: the k-th kept entry is the smallest finite one)
        stat = float(fin.abs().min()) if fin.numel() else math.nan
    elif kind == "sign":
        sc = sign_scale(u) if s is None else u.numpy().dtype.type(s)
        c = torch.copysign(torch.full_like(u, float(sc)), u)
        e = u - c
        stat = float(sc)
    elif kind == "qsgd":
        if not 1 <= int(levels) <= MAX_LEVELS:
            raise ValueError(f"levels must be in 1 .. {MAX_LEVELS}, got {levels!r}")
        ft = u.numpy().dtype.type
        nv = qsgd_norm(u) if norm is None else ft(norm)
        if not (np.isfinite(nv) and nv != 0):
            c, e = u.clone(), torch.zeros_like(u)
        else:
            lv = qsgd_levels(u, levels, nv, compress_words("qsgd", P, seed, round, client))
            mag = torch.as_tensor((nv * lv) / ft(int(levels)))
            c = torch.copysign(mag, u)
            e = u - c
        stat = float(nv)
    elif kind == "randk":
        if not 1 <= int(k) <= P:
            raise ValueError(f"k must be in 1 .. {P}, got {k!r}")
        key = randk_keys(P, seed, round, client)
        kept = _largest_mask(key, k)
        zero = torch.zeros_like(u)
        if error_feedback:
            c = torch.where(kept, u, zero)
        else:   # the unbiased variant: one gain, (float)P / (float)k in u's type
            ft = u.numpy().dtype.type
            c = torch.where(kept, u * float(ft(ft(P) / ft(int(k)))), zero)
        e = torch.where(kept, zero, u)
        stat = float(np.float32(key[kept.numpy()].min()) * np.float32(2.0 ** -31))
    else:
        raise ValueError(f"compress_torch: kind must be one of {ALL_COMPRESSORS[1:]}, got {kind!r}")
    if not error_feedback:
        e = torch.zeros_like(u)
    return c, e, stat


def compress_round(local, x, e, w: float, kind: str, k: int = 0, error_feedback: bool = True,
                   s: Optional[float] = None, *, levels: int = 127, seed: int = 0, round: int = 0,
                   client: int = 0, norm: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """The whole rule for one sampled client of a live round: ``(contribution, e', stat)`` from its
    local model, the image ``x`` the round trained from, its residual ``e`` and FedAvg weight ``w``
    (dense vectors; fp32 unless ``local`` is float64)."""
    local = _vec(local)
    x, e = _vec(x).to(local.dtype), _vec(e).to(local.dtype)
    u = (local - x) + e
    c, e_new, stat = compress_torch(u, kind, k, error_feedback, s, levels=levels, seed=seed, round=round,
                                    client=client, norm=norm)
    return torch.tensor(float(w), dtype=local.dtype) * (x + c), e_new, stat

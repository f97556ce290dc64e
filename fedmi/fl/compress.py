"""Update compression with error feedback: the rule, a host model of the kernel, wire-size accounting.

A client's round update is compressed before it enters the FedAvg exchange (top-k sparsification with
memory, Stich et al. 2018; scaled sign with error feedback, Karimireddy et al. 2019).  This is a
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

An unsampled client and a round that is not live leave contribution and residual untouched.  Both
compressors are deterministic: every replica and every graph replay is bit-identical.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

COMPRESSORS = ("none", "topk", "sign")
# threads of the kernel's workgroup: the fixed summation order of `s` follows them
_THREADS = 1024


def compress_id(cfg) -> int:
    """Validate the compression fields of an ``EngineConfig``; the compressor's index in
    ``COMPRESSORS`` (0 = off)."""
    if cfg.compress not in COMPRESSORS:
        raise ValueError(f"compress must be one of {COMPRESSORS}, got {cfg.compress!r}")
    try:
        ratio = float(cfg.compress_ratio)
    except (TypeError, ValueError):
        ratio = math.nan
    if not (math.isfinite(ratio) and 0.0 < ratio <= 1.0):
        raise ValueError(f"compress_ratio must be a finite number in (0, 1], got {cfg.compress_ratio!r}")
    if not isinstance(cfg.error_feedback, (bool, np.bool_)):
        raise ValueError(f"error_feedback must be a bool, got {cfg.error_feedback!r}")
    kind = COMPRESSORS.index(cfg.compress)
    if kind and float(cfg.dp_clip) > 0.0:
        raise ValueError(f"compress={cfg.compress!r} does not combine with differential privacy (dp_clip > 0): "
                         "both rewrite the contribution, and the noise calibration assumes the clipped update")
    return kind


def topk_count(ratio: float, P: int) -> int:
    """Entries top-k keeps of P parameters: ``max(1, min(P, ceil(ratio * P)))``."""
    return max(1, min(int(P), int(math.ceil(float(ratio) * int(P)))))


def compress_k(cfg, P: int) -> int:
    """Entries a config's compressor transmits of P parameters (sign and dense: all P)."""
    return topk_count(cfg.compress_ratio, P) if cfg.compress == "topk" else int(P)


def uplink_bytes(kind: str, k: int, P: int) -> int:
    """Bytes a real uplink would carry per client and round: top-k ``8 k`` (an fp32 value and an int32
    index per kept entry), sign ``4 + ceil(P / 8)`` (the fp32 scale and one bit per coordinate), dense
    ``4 P``."""
    if kind not in COMPRESSORS:
        raise ValueError(f"compress must be one of {COMPRESSORS}, got {kind!r}")
    if kind == "topk":
        return 8 * int(k)
    if kind == "sign":
        return 4 + (int(P) + 7) // 8
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


def sign_scale(u):
    """``(sum |u|) / P`` in the kernel's order: thread t of 1024 adds its entries t, t + 1024, ... in
    turn, an xor tree (offsets 32, 16, ... 1) sums each 64-lane wave, the 16 wave sums are added in wave
    order, one division by ``float(P)``."""
    a = np.abs(_vec(u).numpy())
    P, ft = a.shape[0], a.dtype.type
    per = (P + _THREADS - 1) // _THREADS
    pad = np.zeros(per * _THREADS, ft)
    pad[:P] = a
    acc = np.zeros(_THREADS, ft)
    for row in pad.reshape(per, _THREADS):   # (adding the padding's +0 changes no bit: |u| >= +0)
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
    return ft(ss / ft(P))


def topk_mask(u, k: int) -> torch.Tensor:
    """Boolean mask of the k entries top-k keeps (magnitude key, larger first; ties: lower index)."""
    key = _keys(_vec(u))
    order = np.argsort(-key, kind="stable")
    kept = np.zeros(key.shape[0], bool)
    kept[order[:int(k)]] = True
    return torch.as_tensor(kept)


def compress_torch(u, kind: str, k: int = 0, error_feedback: bool = True,
                   s: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """``(c, e', stat)`` of the vector ``u`` (fp32, or float64 kept as float64): the compressed update,
    the new residual and the round's statistic (top-k: the magnitude of the k-th kept entry; sign: the scale ``s``).  In fp32 a
    bit-exact model of the kernel given the same ``u`` and, for sign, the same ``s`` (``s=None``: the
    host model of the kernel's sum, :func:`sign_scale`)."""
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
    else:
        raise ValueError(f"compress_torch: kind must be 'topk' or 'sign', got {kind!r}")
    if not error_feedback:
        e = torch.zeros_like(u)
    return c, e, stat


def compress_round(local, x, e, w: float, kind: str, k: int = 0, error_feedback: bool = True,
                   s: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """The whole rule for one sampled client of a live round: ``(contribution, e', stat)`` from its
    local model, the image ``x`` the round trained from, its residual ``e`` and FedAvg weight ``w``
    (dense vectors; fp32 unless ``local`` is float64)."""
    local = _vec(local)
    x, e = _vec(x).to(local.dtype), _vec(e).to(local.dtype)
    u = (local - x) + e
    c, e_new, stat = compress_torch(u, kind, k, error_feedback, s)
    return torch.tensor(float(w), dtype=local.dtype) * (x + c), e_new, stat

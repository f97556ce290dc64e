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

The low-rank compressor is the only one that uses the parameters' matrix structure
(``fedmi/ops/csrc/fl_lowrank.hip``; PowerSGD, Vogels et al. 2019):

* ``"powersgd"`` (``r = compress_rank``, 1 .. 8) works layer by layer.  Biases travel raw (``c = u``,
  ``e' = 0``), and so does a weight matrix with ``r (N + K) >= N K`` (the factors would cost as much as the
  matrix; a compressed layer therefore has ``r < min(N, K)``).  A compressed layer's block of ``u`` is the
  row-major ``M [N][K]`` (N out, K in) and ``Q [K][r]`` its state; one warm-started power iteration:
  ``P = M Q``; the columns of ``P`` orthonormalised by modified Gram-Schmidt in column order (column j:
  for i < j in turn ``d = <P_i, P_j>``, ``P_j = P_j - d P_i``; then ``ss = <P_j, P_j>``, ``P_j = P_j /
  sqrt(ss)``, one division per element, or the zero column where ``ss == 0``); ``Q' = M^T P``;
  ``c = P Q'^T``; ``Q <- Q'``; ``e' = u - c``.  If one of the r values ``ss`` is not finite the whole
  layer travels raw this round and keeps its ``Q``.  Order: the dot products of ``M Q`` (over k), ``M^T P``
  (over n) and ``P Q'^T`` (over j) run in ascending contraction index from ``+0``, a product and a sum
  per term; a Gram-Schmidt dot over N is summed as one 64-lane wave does, lane t adding the products of
  entries t, t + 64, ... in turn from ``+0``, then the xor tree 32 .. 1 (:func:`wave_dot`).  The order
  depends on the layer's shape and r alone.  ``Q_0``: ``numpy.random.default_rng(compress_seed)
  .standard_normal((K, r))`` per compressed layer in layer order, cast to fp32 (``None``: a private
  64-bit draw); there is no device RNG, and ``Q`` is state (``compress_q``).  The statistic is
  ``sqrt(sum (u - c)^2) / sqrt(sum u^2)`` over all P entries, both sums in :func:`ordered_sum`'s order
  (0 where ``u = 0`` or the client is not sampled).  A real uplink carries ``r (N + K)`` floats per
  compressed layer and every raw entry; no indices.

The block-scaled quantiser is the only rule that is local: a block's code depends on its own 32 values
(``fedmi/ops/csrc/fl_mx.hip``; OCP Microscaling Formats "MX" v1.0, Rouhani et al. 2023):

* ``"mx"`` (``compress_format`` in ``e4m3`` / ``e5m2`` / ``e2m1``, ``compress_rounding`` in ``nearest`` /
  ``stochastic``).  A block is 32 consecutive dense parameters; the last one is partial.  ``A`` = the largest
  ``bits(u) & 0x7fffffff`` of the block, ``E = A >> 23``.  ``E == 255`` (an inf or NaN in the block): the block
  travels raw, ``c = u``, ``e' = 0`` (qsgd's escape, per block).  ``E < 32`` (block maximum below ``2**-95``):
  ``c = copysign(0, u)``, ``e' = u - c``; the cut-off keeps every scale and every dequantised value a normal
  fp32.  Otherwise ``e = E - 127 - emax`` with ``emax`` = 8 / 15 / 2, the MX scale ``2**(floor(log2 max) -
  emax)``; ``t = |u| * 2**-e`` exactly; the element grid is the format's non-negative finite values (e4m3:
  bias 7, subnormals, maximum 448, no inf; e5m2: bias 15, subnormals, maximum 57344; e2m1: 0, 0.5, 1, 1.5,
  2, 3, 4, 6); ``t`` at or above the maximum saturates to it (the band up to ``2**(emax + 1)`` is reachable in
  every block).  ``"nearest"``: the nearest grid value, ties to the even element code.  ``"stochastic"``: with
  ``l <= t < h`` the neighbouring grid values and ``frac = (t - l) / (h - l)``, ``q = h if (word >> 8) < frac
  * 2**24 else l`` (``t`` on the grid or saturated: ``q = t``), ``word`` as for the random compressors on
  ``MX_STREAM``.  ``c = copysign(q * 2**e, u)``, exact; ``e' = u - c``.  The statistic is the largest block
  scale ``2**e`` of the round's quantised blocks (0: none, or the client is not sampled).  A real uplink
  carries one E8M0 scale byte per block and ``bits`` = 8 / 8 / 4 per element: ``ceil(P / 32) + ceil(P * bits /
  8)`` bytes; blocks that travel raw are not counted.  :func:`mx_quantize` states the rule from the formats'
  value tables.

An unsampled client and a round that is not live leave contribution and residual (and powersgd's ``Q``)
untouched.  Top-k, sign, powersgd and mx with nearest rounding are deterministic: every replica and every graph replay is bit-identical.  The random compressors
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
# low-rank factorisation: the compressor carries a state Q per compressed layer beside the residual
LOWRANK_COMPRESSORS = ("powersgd",)
COMPRESSOR_KINDS = ALL_COMPRESSORS + LOWRANK_COMPRESSORS   # compress_id's index: the kernels' FL_COMPRESS_*
# block floating point: 32 consecutive parameters share one power-of-two scale (OCP MX)
BLOCK_COMPRESSORS = ("mx",)
COMPRESSOR_NAMES = COMPRESSOR_KINDS + BLOCK_COMPRESSORS   # ... and with "mx" = FL_COMPRESS_MX = 6 behind them
MX_FORMATS = ("e4m3", "e5m2", "e2m1")                     # the kernel's FL_MX_* index
MX_ROUNDINGS = ("nearest", "stochastic")
MX_BLOCK = 32
MAX_LEVELS = 32767
MAX_RANK = 8
# threads of the kernel's workgroup: the fixed summation order of `s` follows them
_THREADS = 1024


def compress_id(cfg) -> int:
    """Validate the compression fields of an ``EngineConfig``; the compressor's index in
    ``COMPRESSOR_NAMES`` (0 = off)."""
    if cfg.compress not in COMPRESSOR_NAMES:
        raise ValueError(f"compress must be one of {COMPRESSOR_NAMES}, got {cfg.compress!r}")
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
    rank = getattr(cfg, "compress_rank", 4)
    if isinstance(rank, (bool, np.bool_)) or not isinstance(rank, (int, np.integer)) or not 1 <= int(rank) <= MAX_RANK:
        raise ValueError(f"compress_rank must be an integer in [1, {MAX_RANK}], got {rank!r}")
    fmt, rounding = getattr(cfg, "compress_format", "e4m3"), getattr(cfg, "compress_rounding", "nearest")
    if not isinstance(fmt, str) or fmt not in MX_FORMATS:
        raise ValueError(f"compress_format must be one of {MX_FORMATS}, got {fmt!r}")
    if not isinstance(rounding, str) or rounding not in MX_ROUNDINGS:
        raise ValueError(f"compress_rounding must be one of {MX_ROUNDINGS}, got {rounding!r}")
    kind = COMPRESSOR_NAMES.index(cfg.compress)
    if kind and float(cfg.dp_clip) > 0.0:
        raise ValueError(f"compress={cfg.compress!r} does not combine with differential privacy (dp_clip > 0): "
                         "both rewrite the contribution, and the noise calibration assumes the clipped update")
    return kind


def topk_count(ratio: float, P: int) -> int:
    """Entries top-k keeps of P parameters: ``max(1, min(P, ceil(ratio * P)))``."""
    return max(1, min(int(P), int(math.ceil(float(ratio) * int(P)))))


def compress_k(cfg, P: int, dims=None) -> int:
    """Entries a config's compressor transmits of P parameters (sign, qsgd and dense: all P; powersgd:
    the factors' entries and every raw entry of the model ``dims``)."""
    if cfg.compress in LOWRANK_COMPRESSORS:
        if dims is None:
            raise ValueError("compress_k: compress='powersgd' needs the model's dims")
        return lowrank_layers(dims, int(cfg.compress_rank))["entries"]
    return topk_count(cfg.compress_ratio, P) if cfg.compress in ("topk", "randk") else int(P)


def qsgd_code_bits(levels: int) -> int:
    """Width of QSGD's fixed-width sign-and-level code: ``ceil(log2(2 s + 1))`` bits."""
    return (2 * int(levels)).bit_length()   # 2 s + 1 codes: the smallest b with 2**b >= 2 s + 1


def mx_uplink_bytes(P: int, fmt: str) -> int:
    """Bytes of an MX uplink: one E8M0 scale per block of 32 and 8 / 8 / 4 bits per element."""
    return (int(P) + MX_BLOCK - 1) // MX_BLOCK + (int(P) * (4 if MX_FORMATS.index(fmt) == 2 else 8) + 7) // 8


def uplink_bytes(kind: str, k: int, P: int, levels: int = 127, fmt: str = "e4m3") -> int:
    """Bytes a real uplink would carry per client and round: top-k ``8 k`` (an fp32 value and an int32
    index per kept entry), sign ``4 + ceil(P / 8)`` (the fp32 scale and one bit per coordinate), qsgd
    ``4 + ceil(P * ceil(log2(2 s + 1)) / 8)`` (the fp32 norm and a fixed-width sign-and-level code per
    coordinate; no Elias coding), randk ``4 k`` (the values only: the indices follow from the shared
    seed), powersgd ``4 k`` (``k`` = :func:`compress_k`: factors and raw entries), mx
    :func:`mx_uplink_bytes` of ``fmt`` (raw blocks are not counted), dense ``4 P``."""
    if kind not in COMPRESSOR_NAMES:
        raise ValueError(f"compress must be one of {COMPRESSOR_NAMES}, got {kind!r}")
    if kind in BLOCK_COMPRESSORS:
        return mx_uplink_bytes(P, fmt)
    if kind == "topk":
        return 8 * int(k)
    if kind == "sign":
        return 4 + (int(P) + 7) // 8
    if kind == "qsgd":
        return 4 + (int(P) * qsgd_code_bits(levels) + 7) // 8
    if kind == "randk" or kind in LOWRANK_COMPRESSORS:
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
    from ..privacy.philox import MX_STREAM, QSGD_STREAM, RANDK_STREAM, param_words
    streams = {"qsgd": QSGD_STREAM, "randk": RANDK_STREAM, "mx": MX_STREAM}
    if kind not in streams:
        raise ValueError(f"compress_words: kind must be one of {tuple(streams)}, got {kind!r}")
    return param_words(P, round, client, seed, streams[kind])


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
                   client: int = 0, norm: Optional[float] = None, fmt: str = "e4m3",
                   rounding: str = "nearest") -> Tuple[torch.Tensor, torch.Tensor, float]:
    """``(c, e', stat)`` of the vector ``u`` (fp32, or float64 kept as float64): the compressed update,
    the new residual and the round's statistic (top-k: the magnitude of the k-th kept entry; sign: the
    scale ``s``; qsgd: the norm; randk: ``key31`` of the k-th kept entry times ``2**-31``, the selection's
    quantile; mx: the largest block scale).  In fp32 a bit-exact model of the kernel given the same ``u`` and, for sign / qsgd, the same
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
    elif kind == "mx":
        words = compress_words("mx", P, seed, round, client) if rounding == "stochastic" else None
        c, raw, stat = mx_quantize(u, fmt, rounding, words)
        with np.errstate(invalid="ignore"):
            e = torch.where(raw, torch.zeros_like(u), u - c)
    else:
        raise ValueError(f"compress_torch: kind must be one of {ALL_COMPRESSORS[1:] + BLOCK_COMPRESSORS}, got {kind!r}")
    if not error_feedback:
        e = torch.zeros_like(u)
    return c, e, stat


def compress_round(local, x, e, w: float, kind: str, k: int = 0, error_feedback: bool = True,
                   s: Optional[float] = None, *, levels: int = 127, seed: int = 0, round: int = 0,
                   client: int = 0, norm: Optional[float] = None, fmt: str = "e4m3",
                   rounding: str = "nearest") -> Tuple[torch.Tensor, torch.Tensor, float]:
    """The whole rule for one sampled client of a live round: ``(contribution, e', stat)`` from its
    local model, the image ``x`` the round trained from, its residual ``e`` and FedAvg weight ``w``
    (dense vectors; fp32 unless ``local`` is float64)."""
    local = _vec(local)
    x, e = _vec(x).to(local.dtype), _vec(e).to(local.dtype)
    u = (local - x) + e
    c, e_new, stat = compress_torch(u, kind, k, error_feedback, s, levels=levels, seed=seed, round=round,
                                    client=client, norm=norm, fmt=fmt, rounding=rounding)
    return torch.tensor(float(w), dtype=local.dtype) * (x + c), e_new, stat


# ---- block-scaled FP8 / FP4 elements (OCP MX): the rule fl_mx.hip is held to ----
_MX_SPEC = {"e4m3": (7, 3, 8, 0x7E), "e5m2": (15, 2, 15, 0x7B), "e2m1": (1, 1, 2, 0x7)}   # bias, mantissa bits, emax, top code


def mx_grid(fmt: str) -> np.ndarray:
    """The non-negative finite values of an element format in code order (float64; index = element code)."""
    bias, m, _, top = _MX_SPEC[fmt]
    vals = []
    for code in range(top + 1):
        ex, man = code >> m, code & ((1 << m) - 1)
        vals.append(man * 2.0 ** (1 - bias - m) if ex == 0 else (1.0 + man * 2.0 ** -m) * 2.0 ** (ex - bias))
    return np.asarray(vals, np.float64)


def mx_quantize(u, fmt: str = "e4m3", rounding: str = "nearest", words: Optional[np.ndarray] = None):
    """``(c, raw, stat)`` of the vector ``u`` under the MX rule of the module docstring, block by block in
    float64 from :func:`mx_grid`: ``c`` in ``u``'s float type, ``raw`` = the entries of blocks that travel as
    they are, ``stat`` = the largest block scale (0: no block was quantised).  ``words``: the uint32 word of
    every entry (``"stochastic"``)."""
    if fmt not in MX_FORMATS or rounding not in MX_ROUNDINGS:
        raise ValueError(f"mx_quantize: fmt must be one of {MX_FORMATS} and rounding one of {MX_ROUNDINGS}")
    u = _vec(u)
    a = u.numpy().astype(np.float64)
    grid, emax = mx_grid(fmt), _MX_SPEC[fmt][2]
    if rounding == "stochastic":
        if words is None or len(words) != a.shape[0]:
            raise ValueError("mx_quantize: stochastic rounding needs one word per entry")
        w24 = (np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float64)
    c, raw, best = a.copy(), np.zeros(a.shape[0], bool), None
    for b in range(0, a.shape[0], MX_BLOCK):
        blk = a[b:b + MX_BLOCK]
        if not np.all(np.isfinite(blk)):
            raw[b:b + MX_BLOCK] = True
            continue
        top = np.abs(blk).max()
        if top < 2.0 ** -95:
            c[b:b + MX_BLOCK] = np.copysign(0.0, blk)
            continue
        e = math.frexp(top)[1] - 1 - emax                   # floor(log2 max) - emax
        t = np.minimum(np.ldexp(np.abs(blk), -e), grid[-1])   # exact; the band above the maximum saturates
        hi = np.minimum(np.searchsorted(grid, t, side="right"), len(grid) - 1)
        lo = np.searchsorted(grid, t, side="right") - 1      # grid[lo] <= t, and t < grid[hi] unless saturated
        l, h = grid[lo], grid[hi]
        if rounding == "nearest":
            mid = 0.5 * (l + h)
            up = (t > mid) | ((t == mid) & (lo % 2 == 1))    # a tie goes to the even code
        else:
            frac = (t - l) / np.where(h > l, h - l, 1.0)     # exact: a 25-bit difference over a power of two
            up = w24[b:b + MX_BLOCK] < frac * 2.0 ** 24
        c[b:b + MX_BLOCK] = np.copysign(np.ldexp(np.where(up, h, l), e), blk)
        best = e if best is None else max(best, e)
    stat = 0.0 if best is None else 2.0 ** best
    return torch.as_tensor(c.astype(u.numpy().dtype)), torch.as_tensor(raw), float(stat)


# ---- low-rank factors (PowerSGD): the host model of fl_lowrank.hip ----
def lowrank_layers(dims, r: int) -> dict:
    """Which layers of the model ``dims`` rank ``r`` compresses: ``layers`` = one dict per Linear layer
    (``N``, ``K``, ``compressed``, dense offsets ``w_off`` / ``b_off``, ``q_off`` = offset of its
    ``Q [K][r]`` in the state vector), ``q_len`` = the state's length, ``entries`` = floats a real uplink
    carries (``r (N + K)`` per compressed layer and every raw entry)."""
    r = int(r)
    if not 1 <= r <= MAX_RANK:
        raise ValueError(f"compress_rank must be an integer in [1, {MAX_RANK}], got {r!r}")
    layers, off, q_off, entries = [], 0, 0, 0
    for K, N in zip(dims[:-1], dims[1:]):
        K, N = int(K), int(N)
        comp = r * (N + K) < N * K
        layers.append(dict(N=N, K=K, compressed=comp, w_off=off, b_off=off + N * K, q_off=q_off))
        off += N * K + N
        q_off += r * K if comp else 0
        entries += (r * (N + K) if comp else N * K) + N
    return dict(layers=layers, q_len=q_off, entries=entries, P=off)


def lowrank_q0(dims, r: int, seed: Optional[int]) -> np.ndarray:
    """``Q_0`` of every compressed layer, concatenated in layer order (fp32 ``[q_len]``): standard normals
    of ``numpy.random.default_rng(seed)``, one ``(K, r)`` draw per compressed layer; ``None``: a private
    64-bit seed."""
    import os
    g = np.random.default_rng(int.from_bytes(os.urandom(8), "little") if seed is None else int(seed))
    parts = [g.standard_normal((ly["K"], int(r))).astype(np.float32).reshape(-1)
             for ly in lowrank_layers(dims, r)["layers"] if ly["compressed"]]
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def wave_dot(a: np.ndarray, b: np.ndarray):
    """``<a, b>`` as one 64-lane wave of the kernel sums it: lane t adds the products of entries t,
    t + 64, ... in turn from ``+0``, then the xor tree (offsets 32, 16, ... 1).  (A lane's sum is never
    ``-0``, so the ``+0`` products of the padding change no bit.)"""
    ft = a.dtype.type
    prod = a * b
    pad = np.zeros(-(-prod.shape[0] // 64) * 64, ft)
    pad[:prod.shape[0]] = prod
    lanes = np.zeros(64, ft)
    for row in pad.reshape(-1, 64):
        lanes = lanes + row
    idx, off = np.arange(64), 32
    while off:
        lanes = lanes + lanes[idx ^ off]
        off >>= 1
    return lanes[0]


def _lowrank_layer(M: np.ndarray, Q: np.ndarray):
    """One power iteration on ``M [N][K]`` from ``Q [K][r]``: ``(c, Q', finite)``; every operation one
    rounding in ``M``'s float type, the orders of the module docstring."""
    ft = M.dtype.type
    N, K = M.shape
    r = Q.shape[1]
    P = np.zeros((N, r), ft)
    for k in range(K):
        P = P + M[:, k:k + 1] * Q[k:k + 1, :]
    finite = True
    for j in range(r):
        for i in range(j):
            P[:, j] = P[:, j] - wave_dot(P[:, i], P[:, j]) * P[:, i]
        ss = wave_dot(P[:, j], P[:, j])
        finite = finite and bool(np.isfinite(ss))
        P[:, j] = ft(0.0) if ss == 0 else P[:, j] / np.sqrt(ss)
    Qn = np.zeros((K, r), ft)
    for n in range(N):
        Qn = Qn + M[n, :, None] * P[n:n + 1, :]
    c = np.zeros((N, K), ft)
    for j in range(r):
        c = c + P[:, j:j + 1] * Qn[None, :, j]
    return c, Qn, finite


def lowrank_torch(u, q, dims, r: int, error_feedback: bool = True):
    """``(c, e', q', stat)`` of the dense vector ``u`` and the state ``q`` (:func:`lowrank_layers` order)
    for the model ``dims`` at rank ``r``.  In fp32 a bit-exact model of the kernel; float64 inputs run the
    same rule in float64."""
    u = _vec(u)
    a = u.numpy()
    ft = a.dtype.type
    qv = np.ascontiguousarray(torch.as_tensor(q).detach().cpu().numpy().reshape(-1), dtype=a.dtype)
    plan = lowrank_layers(dims, r)
    if a.shape[0] != plan["P"] or qv.shape[0] != plan["q_len"]:
        raise ValueError(f"lowrank_torch: u has {a.shape[0]} entries and q {qv.shape[0]}, the model "
                         f"{plan['P']} and {plan['q_len']}")
    c, e, qn = a.copy(), np.zeros_like(a), qv.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for ly in plan["layers"]:
            if not ly["compressed"]:
                continue
            N, K, wo, qo = ly["N"], ly["K"], ly["w_off"], ly["q_off"]
            cl, ql, finite = _lowrank_layer(a[wo:wo + N * K].reshape(N, K), qv[qo:qo + K * int(r)].reshape(K, int(r)))
            if finite:   # else: the layer travels raw and keeps its Q
                c[wo:wo + N * K] = cl.reshape(-1)
                e[wo:wo + N * K] = a[wo:wo + N * K] - c[wo:wo + N * K]
                qn[qo:qo + K * int(r)] = ql.reshape(-1)
        d = a - c
        den = np.sqrt(ordered_sum(a * a))
        stat = ft(0.0) if den == 0 else ft(np.sqrt(ordered_sum(d * d)) / den)
    if not error_feedback:
        e = np.zeros_like(a)
    return torch.as_tensor(c), torch.as_tensor(e), torch.as_tensor(qn), float(stat)

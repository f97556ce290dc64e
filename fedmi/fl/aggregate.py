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

Multi-Krum screening (Blanchard et al. 2017, "Machine Learning with Adversaries: Byzantine Tolerant
Gradient Descent"; ``EngineConfig.screen``) runs in front of any of the three rules and judges whole
models, where the rules above judge every coordinate on its own.  With ``f`` Byzantine clients
assumed and ``m`` clients to keep, per round:

* ``d(i, j)`` = the sum over the real parameters of ``(v_i - v_j)^2`` for sampled ``i != j``, a sum
  that is not ``< +inf`` (NaN, inf, overflow) counting as ``+inf``; ``d(i, i) = 0``;
* ``K_r < 2 f + 3`` keeps every sampled client; otherwise ``score(i)`` = the sum, in client order, of
  the ``K_r - f - 2`` smallest ``d(i, j)`` (ties by client index);
* the ``min(m, K_r - f)`` clients of smallest score are kept (ties to the lower client index), and the
  coordinate rule runs over them: ``K_r`` becomes the number kept.  ``aggregator="mean"`` is then the
  UNWEIGHTED mean of the kept clients (the trimmed mean with ``beta = 0``) -- the paper's multi-Krum;
  ``m = 1`` is Krum.

:func:`pair_distances_model` is the bit-exact fp32 model of the distance kernel
(``fedmi/ops/csrc/fl_screen.hip``) over parameter images, :func:`screen_select` the selection rule on
a distance matrix (the select kernel's model, and what the torch engines run).  The torch engines
compute their distances with :func:`pair_distances_torch`, fp32 in torch's own summation order: their
kept set can differ from the HIP engines' only where two scores lie within fp32 summation error of
each other.

The geometric median (``aggregator="geomed"``; Pillutla, Kakade, Harchaoui 2022, "Robust Aggregation for
Federated Learning", RFA) sits between the two: a whole-vector rule that needs no ``f``, with breakdown
point 1/2, every client pulling with at most unit force.  It iterates, so it is no ``AGGREGATORS``
entry (those are one-launch rules) but the ``ITERATIVE_AGGREGATORS`` one, id 3 in ``ALL_AGGREGATORS``.
With ``T = geomed_iters`` and ``nu = float32(geomed_nu)``, over the sampled (and, behind a screen, kept)
clients ``S``:

* ``z_0`` = the coordinate-wise median of ``S``, exactly the rule above;
* ``T`` times: ``d_i = sum (v_i - z_t)^2`` over the real parameters; the clients with ``d_i < +inf`` are
  included (NaN, inf and overflow exclude a client for that iteration -- selected out, never multiplied
  by 0); ``b_i = 1 / max(nu, sqrt(d_i))``; ``z_{t+1} = (sum b_i v_i) / (sum b_i)``, both sums in client
  order from ``+0``, one division; nobody included: ``z_{t+1} = z_t``.

:func:`geomed_model` is the bit-exact fp32 model of the launches (``fedmi/ops/csrc/fl_geomed.hip``) over
parameter images, with the distances added in the kernel's one order (:func:`geomed_block_sums`);
:func:`geomed_torch` is the rule in the tensor's dtype with torch's own summation order: what the torch
engines run in fp32, and the float64 oracle in float64.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from .attack import ATTACKS

AGGREGATORS = ("mean", "median", "trimmed_mean")
# rules that iterate over whole models (several launches, scratch of their own); ids follow AGGREGATORS'
ITERATIVE_AGGREGATORS = ("geomed",)
ALL_AGGREGATORS = AGGREGATORS + ITERATIVE_AGGREGATORS
MAX_ROBUST_CLIENTS = 64   # width of the per-round sampled-client mask (fl_common.h FL_ROBUST_MAX_K)
SCREENS = ("none", "multi_krum")
_SCREEN_THREADS = 256     # workgroup of the distance kernel (fl_screen.hip FL_SCREEN_THREADS)
GEOMED_MAX_ITERS = 32     # fl_common.h FL_GEOMED_MAX_ITERS
GEOMED_BLOCK = 256        # floats of the image per block of a distance sum (fl_common.h FL_GEOMED_THREADS)
GEOMED_SLOT = 192         # floats of one iteration's record in the scratch (fl_common.h FL_GEOMED_SLOT)


def geomed_scratch_floats(pimg: int, iters: int) -> int:
    """Floats of scratch the geomed launches need for an image of ``pimg`` floats (fl_common.h
    fl_geomed_scratch_floats): two sets of 64 distance partials per block, then ``iters`` records."""
    return 2 * ((int(pimg) + GEOMED_BLOCK - 1) // GEOMED_BLOCK) * MAX_ROBUST_CLIENTS + int(iters) * GEOMED_SLOT


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
    """The Python-launched aggregation kernels (``robust_aggregate``, ``secagg_mask``, ``secagg_open``) and the
    attack stage in front of them (``attack_apply``, ``fedmi/fl/attack.py``) of one federation, over buffers
    that keep their addresses.  ``lead``: the engine whose dims, round
    state, ``rtab`` and config every launch uses (identical on all clients); ``src[par]`` / ``dst[par]``:
    the source and destination buffers of a round of output parity ``par``; :meth:`mask` masks the
    destinations in place -- what a process publishes is where it receives the aggregate -- as clients
    ``first_client ..`` with the clamp histories ``clamps``.  Owns the device pointer tables."""

    def __init__(self, lead, src, dst, clamps=(), first_client: int = 0):
        """With a screen (``lead.screen``) the launcher also owns the K x K distance scratch and the
        kept-mask word of each parity; the kept-mask history is the lead engine's ``screen_hist``."""
        def table(ts):
            return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=lead.device)
        self._lead, self._bufs = lead, (src, dst, clamps)   # (the tables hold addresses: keep the buffers)
        self._k, self._n, self._first = len(src[0]), len(dst[0]), int(first_client)
        self._src = [table(s) for s in src]
        self._dst = self._src if dst is src else [table(s) for s in dst]
        self._clamp = table(clamps)
        self._dist = self._keep = self._geomed = None
        if ALL_AGGREGATORS[getattr(lead, "robust", 0)] == "geomed":
            # distance partials and the iterations' records (weights, distances, combined mask) of the geomed launches
            self._geomed = torch.zeros(geomed_scratch_floats(lead.Pimg, int(lead.cfg.geomed_iters)),
                                       dtype=torch.float32, device=lead.device)
        if getattr(lead, "screen", 0):
            self._dist = torch.zeros(self._k * self._k, dtype=torch.float32, device=lead.device)
            self._keep = torch.zeros(2, dtype=torch.int64, device=lead.device)
        self._wtab = None
        if getattr(lead, "attack_stage", False):
            # the attack stage's table of the k buffers' FedAvg weights per round (unweighted mode: none, all 1)
            wtab = lead.attack_weights()
            if wtab is not None:
                self._wtab = torch.as_tensor(wtab, device=lead.device).contiguous()
            self._bad = mask_bits(k in lead.attack_par["clients"] for k in range(self._k))   # a constant of the federation

    def _round(self, par: int):
        e = self._lead
        return e.state[par].data_ptr(), e.rtab.data_ptr()

    def robust(self, par: int, stream: int) -> None:
        """The aggregate launch; with a screen the distance and select launches run in front of it and
        the rule takes the kept clients."""
        e = self._lead
        keep = ()   # (no screen: the call is the one it was before screening existed, argument for argument)
        if self._keep is not None:
            word = self._keep.data_ptr() + 8 * par
            keep = (word,)
            e.m.screen_dist(e.dims, self._src[par].data_ptr(), self._k, self._dist.data_ptr(), *self._round(par),
                            int(e.cfg.max_rounds), stream)
            e.m.screen_select(self._dist.data_ptr(), self._k, int(e.cfg.screen_byzantine), int(e.cfg.screen_keep or 0),
                              word, e.screen_hist.data_ptr(), *self._round(par), int(e.cfg.max_rounds), stream)
        if self._geomed is not None:
            # the geometric median: geomed_iters + 1 launches (fl_geomed.hip) in the place of the one
            e.m.geomed_aggregate(e.dims, int(e.cfg.geomed_iters), float(e.cfg.geomed_nu), self._src[par].data_ptr(),
                                 self._k, self._dst[par].data_ptr(), self._n, *self._round(par),
                                 self._k * e.tail_stride, int(e.cfg.max_rounds), self._geomed.data_ptr(), stream, *keep)
            return
        e.m.robust_aggregate(e.dims, e.robust, float(e.robust_beta), self._src[par].data_ptr(), self._k,
                             self._dst[par].data_ptr(), self._n, *self._round(par), self._k * e.tail_stride,
                             int(e.cfg.max_rounds), stream, *keep)

    def attack(self, par: int, stream: int) -> None:
        """The attack stage (fl_attack.hip): one launch rewrites the bad sampled clients' buffers among the
        sources in place; ``x`` is the lead engine's round-input image, the other parity's buffer."""
        e = self._lead
        a = e.attack_par
        e.m.attack_apply(e.dims, ATTACKS.index(a["kind"]), a["scale"], a["z"], int(e.cfg.attack_seed),
                         self._src[par].data_ptr(), self._k, e.params[par ^ 1].data_ptr(),
                         0 if self._wtab is None else self._wtab.data_ptr(), self._bad,
                         *self._round(par), int(e.cfg.max_rounds), stream)

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


def _check_geomed(who: str, K: int, active: Sequence[bool], iters: int, nu: float):
    act = [bool(a) for a in active]
    if len(act) != K:
        raise ValueError(f"{who}: {len(act)} mask entries for {K} clients")
    if not any(act):
        raise ValueError(f"{who}: needs at least one sampled client")
    if not 1 <= int(iters) <= GEOMED_MAX_ITERS:
        raise ValueError(f"{who}: iters must be in [1, {GEOMED_MAX_ITERS}], got {iters!r}")
    nu32 = np.float32(nu)   # the kernels' smoothing constant is (float)geomed_nu
    if not (np.isfinite(nu32) and nu32 > 0):
        raise ValueError(f"{who}: nu must be finite and > 0 in fp32, got {nu!r}")
    return act, nu32


def geomed_torch(stack: torch.Tensor, active: Sequence[bool], iters: int, nu: float,
                 trace: Optional[list] = None) -> torch.Tensor:
    """The smoothed-Weiszfeld geometric median (Pillutla et al. 2022, RFA) of the rows of ``stack`` [K, P]
    whose ``active`` entry is true, in ``stack``'s dtype (float32: what the torch engines run; float64:
    the oracle): from the coordinate-wise median, ``iters`` times ``d_i = sum (v_i - z)^2`` in torch's own
    summation order, the clients with ``d_i < +inf`` combined with weights ``1 / max(nu, sqrt(d_i))``
    (added in client order, divided once by their sum); nobody at a finite distance: ``z`` stays.
    ``trace``: a list that receives each iteration's included clients."""
    if stack.dim() != 2 or stack.dtype not in (torch.float32, torch.float64):
        raise ValueError("geomed_torch: needs a [K, P] float32 or float64 tensor")
    act, nu32 = _check_geomed("geomed_torch", int(stack.shape[0]), active, iters, nu)
    S = [i for i, a in enumerate(act) if a]
    z = robust_aggregate_torch(stack, act, "median", 0.0)
    floor = torch.tensor(float(nu32), dtype=stack.dtype, device=stack.device)
    for _ in range(int(iters)):
        d = ((stack[S] - z[None]) ** 2).sum(1)
        incl = [i for i, ok in zip(S, (d < math.inf).tolist()) if ok]
        if trace is not None:
            trace.append(incl)
        if not incl:
            continue   # (z stays, and so does every later iteration's distance)
        b = 1.0 / torch.maximum(floor, torch.sqrt(d))
        acc = torch.zeros_like(z)
        tot = torch.zeros((), dtype=stack.dtype, device=stack.device)
        for j, i in enumerate(S):
            if i in incl:   # selected, never multiplied by 0: an excluded row may hold NaN
                acc = acc + b[j] * stack[i]
                tot = tot + b[j]
        z = acc / tot
    return z


def geomed_block_sums(sq: np.ndarray) -> np.ndarray:
    """The distance sums of ``fl_geomed_kernel`` for the per-position terms ``sq`` [K, n] (fp32, ``+0`` where
    the position is image padding): blocks of 256 consecutive positions (the last one filled with ``+0``),
    each added by the xor tree (offsets 32, 16, ... 1) over its four runs of 64 and the four sums in order
    from ``+0``; the block sums folded in block order from ``+0``.  One rounding per addition."""
    sq = np.ascontiguousarray(sq, np.float32)
    K, n = sq.shape
    nb = (n + GEOMED_BLOCK - 1) // GEOMED_BLOCK
    pad = np.zeros((K, nb * GEOMED_BLOCK), np.float32)
    pad[:, :n] = sq
    lanes = pad.reshape(K, nb, GEOMED_BLOCK // 64, 64)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        off = 32
        while off:
            lanes = lanes + lanes[..., idx ^ off]
            off >>= 1
        blk = np.zeros((K, nb), np.float32)
        for w in range(GEOMED_BLOCK // 64):
            blk = blk + lanes[:, :, w, 0]
        d = np.zeros(K, np.float32)
        for w in range(nb):
            d = d + blk[:, w]
    return d


def geomed_model(stack, active: Sequence[bool], real, iters: int, nu: float, trace: Optional[list] = None,
                 records: Optional[list] = None) -> np.ndarray:
    """What the ``fl_geomed`` launches write for the parameter images ``stack`` [K, Pimg] (fp32), bit for
    bit: the image of the geometric median of the ``active`` clients, padding (``real`` [Pimg] false)
    exact 0.  The rule is :func:`geomed_torch`'s with every operation one fp32 rounding, the median by
    ``robust_aggregate_torch`` and the distances added in the kernel's order (:func:`geomed_block_sums`;
    padding adds ``+0`` whatever it holds).  ``trace`` receives each iteration's included clients,
    ``records`` each iteration's scratch record as the kernel leaves it: ``d`` [K] the distances it measured
    (``+inf`` for a sum that is not ``< +inf``, 0 for a client that is not active), ``b`` [K] and ``mask`` the
    weights and clients it combined (an iteration with nobody included repeats the last combine: its
    record carries that one's; ``mask`` 0: the median was kept)."""
    a = np.ascontiguousarray(np.asarray(stack, np.float32))
    real = np.asarray(real, bool).reshape(-1)
    K, n = a.shape
    if real.shape[0] != n:
        raise ValueError("geomed_model: needs [K, Pimg] images and Pimg flags")
    act, nu32 = _check_geomed("geomed_model", K, active, iters, nu)
    S = [i for i in range(K) if act[i]]
    z = robust_aggregate_torch(torch.from_numpy(a), act, "median", 0.0).numpy()
    eff_b, eff_mask = np.zeros(K, np.float32), 0
    inf = np.float32(np.inf)
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            df = a[S] - z[None]
            dS = geomed_block_sums(np.where(real[None], df * df, np.float32(0.0)))
            d = np.zeros(K, np.float32)
            d[S] = np.where(dS < inf, dS, inf)
            incl = [i for i in S if d[i] < inf]
            if trace is not None:
                trace.append(incl)
            if incl:
                eff_b = np.zeros(K, np.float32)
                eff_b[incl] = np.float32(1.0) / np.maximum(nu32, np.sqrt(d[incl]))
                eff_mask = mask_bits([i in incl for i in range(K)])
                acc = np.zeros(n, np.float32)
                tot = np.float32(0.0)
                for i in incl:
                    acc = acc + eff_b[i] * a[i]
                    tot = np.float32(tot + eff_b[i])
                z = acc / tot
            if records is not None:
                records.append({"d": d, "b": eff_b.copy(), "mask": eff_mask})
    return np.where(real, z, np.float32(0.0)).astype(np.float32)


def _key32(x: np.ndarray) -> np.ndarray:
    """The sortable uint32 image of fp32 values (fl_robust_select.h robust_key): NaN above +inf, -0 == +0."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    k = np.where(u == np.uint32(0x80000000), np.uint32(0x80000000), k)
    return np.where((u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFE), k).astype(np.uint32)


def pair_distances_model(stack, active: Sequence[bool], real) -> np.ndarray:
    """The K x K fp32 matrix ``fl_screen_dist_kernel`` writes for the parameter images ``stack``
    [K, Pimg] (Pimg a multiple of 4), bit for bit: thread t of 256 owns the float4s t, t + 256, ... in
    increasing order and adds, lane by lane, ``(a - b) * (a - b)`` -- one rounding per operation, ``+0``
    for a position that is image padding (``real`` [Pimg] false) -- into its accumulator; an xor tree
    (offsets 32, 16, ... 1) sums each 64-lane wave, the four wave sums are added in wave order; a sum
    that is not ``< +inf`` becomes ``+inf``; the diagonal is 0.  Rows and columns of clients that are
    not ``active`` are left 0 (the kernel leaves them unspecified)."""
    a = np.ascontiguousarray(np.asarray(stack, np.float32))
    real = np.asarray(real, bool).reshape(-1)
    K, n = a.shape
    if n % 4 or real.shape[0] != n:
        raise ValueError("pair_distances_model: needs [K, Pimg] images, Pimg a multiple of 4, and Pimg flags")
    act = [bool(x) for x in active]
    if len(act) != K:
        raise ValueError(f"pair_distances_model: {len(act)} mask entries for {K} clients")
    T = _SCREEN_THREADS
    per = (n // 4 + T - 1) // T
    pad = np.zeros((K, per * T * 4), np.float32)
    pad[:, :n] = a
    keep = np.zeros(per * T * 4, bool)
    keep[:n] = real
    keep = keep.reshape(per, T, 4)
    out = np.zeros((K, K), np.float32)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for i in range(K):
            js = [j for j in range(i + 1, K) if act[i] and act[j]]
            if not js:
                continue
            df = pad[js] - pad[i][None]          # (a - b and b - a square to the same float)
            sq = np.where(keep[None], (df * df).reshape(len(js), per, T, 4), np.float32(0.0))
            acc = np.zeros((len(js), T), np.float32)
            for q in range(per):
                for e in range(4):
                    acc = acc + sq[:, q, :, e]
            lanes = acc.reshape(len(js), T // 64, 64)
            off = 32
            while off:
                lanes = lanes + lanes[:, :, idx ^ off]
                off >>= 1
            ss = np.zeros(len(js), np.float32)
            for w in range(T // 64):
                ss = ss + lanes[:, w, 0]
            ss = np.where(ss < np.float32(np.inf), ss, np.float32(np.inf)).astype(np.float32)
            out[i, js] = ss
            out[js, i] = ss
    return out


def pair_distances_torch(stack: torch.Tensor, active: Sequence[bool]) -> np.ndarray:
    """Squared distances between the rows of ``stack`` [K, P] in fp32, torch's own summation order (the
    torch engines' distances; canonicalised like the kernel's: not ``< +inf`` is ``+inf``, zero diagonal)."""
    a = stack.to(torch.float32)
    d = ((a[:, None, :] - a[None, :, :]) ** 2).sum(-1)
    d = torch.where(d < math.inf, d, torch.full_like(d, math.inf))
    d.fill_diagonal_(0.0)
    act = torch.as_tensor([bool(x) for x in active])
    return torch.where(act[:, None] & act[None, :], d, torch.zeros_like(d)).numpy()


def screen_keep_count(k_r: int, f: int, m: Optional[int]) -> int:
    """Clients a round of ``k_r`` sampled clients keeps: all of them when ``k_r < 2 f + 3`` (the rule
    is undefined there), else ``min(m, k_r - f)``, ``m = None`` meaning ``k_r - f``."""
    k_r, f = int(k_r), int(f)
    if k_r < 2 * f + 3:
        return k_r
    return k_r - f if not m else min(int(m), k_r - f)


def screen_select(dist, active: Sequence[bool], f: int, m: Optional[int] = None) -> list:
    """The multi-Krum kept mask (a list of K bools) from the K x K fp32 distance matrix ``dist``, by the
    rule of the module docstring -- pure rule code, the model of ``fl_screen_select_kernel``: rows and
    columns of clients that are not ``active`` are ignored whatever they hold; scores are added in fp32
    in client order; scores and distances compare on the sortable key, ties to the lower index."""
    d = np.ascontiguousarray(np.asarray(dist, np.float32))
    act = [bool(x) for x in active]
    K = len(act)
    if d.shape != (K, K):
        raise ValueError(f"screen_select: a {d.shape} matrix for {K} clients")
    f = int(f)
    if f < 0 or (m is not None and int(m) < 1):
        raise ValueError(f"screen_select: needs f >= 0 and m >= 1, got f={f}, m={m}")
    S = [i for i in range(K) if act[i]]
    k_r = len(S)
    if k_r < 2 * f + 3:
        return act
    nb, want = k_r - f - 2, screen_keep_count(k_r, f, m)
    key = _key32(d)
    scores = {}
    with np.errstate(all="ignore"):
        for i in S:
            others = [j for j in S if j != i]
            near = sorted(others, key=lambda j: (int(key[i, j]), j))[:nb]
            s = np.float32(0.0)
            for j in sorted(near):
                s = np.float32(s + d[i, j])
            scores[i] = s
    skey = {i: int(_key32(np.array([scores[i]], np.float32))[0]) for i in S}
    kept = set(sorted(S, key=lambda i: (skey[i], i))[:want])
    return [i in kept for i in range(K)]


def mask_bits(mask: Sequence[bool]) -> int:
    """A client mask as the integer the kernels hold (bit k = client k)."""
    return sum(1 << k for k, on in enumerate(mask) if on)

"""Client contribution scores: coalition tables, Shapley / leave-one-out values and the host models of the
coalition kernels (``fedmi/ops/csrc/fl_coalition.hip``).

The players of a round are its sampled clients ``S_r``.  A coalition ``T`` (a 64-bit mask, bit i = client i) is
scored by the FedAvg model it would have produced alone: with ``v_i`` client i's contribution buffer (already
scaled by its FedAvg weight ``w_i``), ``T' = T & S_r`` and ``x`` the image the round trained from,

    num = left fold from +0, in client order, over i in T' of v_i        den = the same fold of w_i
    model = num / den  (one fp32 division);  T' empty: x, selected;  image padding: exact 0

and by that model's utility on the held-out rows: ``u_loss = -(loss_sum / n)`` and ``u_acc = correct / n``.
No server-optimizer step is applied to a coalition model.  The scores are host math in float64 from the
utilities: exact Shapley values over all ``2^K`` masks (K <= 8), the permutation-sampling estimate (K > 8;
Ghorbani & Zou 2019, Song et al. 2019, Wang et al. 2020), or leave-one-out.  An unsampled client is a null
player and scores 0.  Pure numpy: no torch, no device.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

MODES = ("none", "loo", "shapley")
MAX_CONTRIBUTION_CLIENTS = 64   # the width of the sampled-client mask (fl_common.h FL_COALITION_MAX_K)
MAX_COALITIONS = 4096           # fl_common.h FL_COALITION_MAX_M
EXACT_MAX_K = 8                 # "shapley": all 2^K masks up to here, permutations above


def contribution_id(cfg, world: Optional[int] = None) -> int:
    """Validate the contribution fields against what they do not combine with; the mode's index in ``MODES``
    (0 = off).  ``world``: the federation's size when the caller knows it -- one client has nobody to compare
    with, so the feature is off and nothing is refused."""
    mode = getattr(cfg, "contribution", "none")
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"contribution must be one of {MODES}, got {mode!r}")
    m, every = getattr(cfg, "contribution_perms", 0), getattr(cfg, "contribution_every", 1)
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) < 0:
        raise ValueError(f"contribution_perms must be an integer >= 0, got {m!r}")
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or int(every) < 1:
        raise ValueError(f"contribution_every must be an integer >= 1, got {every!r}")
    if mode == "none" or (world is not None and int(world) <= 1):
        return 0
    no = lambda why: ValueError(f"contribution={mode!r} does not run with {why}")
    if bool(cfg.secagg):
        raise no("secagg: a coalition needs the individual contributions, secure aggregation opens only their sum")
    if float(cfg.dp_clip) > 0.0:
        raise no("differential privacy (dp_clip > 0): the contributions carry noise calibrated to the full sum")
    if cfg.compress != "none":
        raise no(f"compress={cfg.compress!r}: a coalition of compressed updates is not the FedAvg of its members")
    if cfg.aggregator != "mean":
        raise no(f"aggregator={cfg.aggregator!r}: the buffers are unscaled local models under another rule")
    if cfg.screen != "none":
        raise no(f"screen={cfg.screen!r}: the buffers are unscaled local models under another rule")
    if world is not None:
        if int(world) > MAX_CONTRIBUTION_CLIENTS:
            raise no(f"more than {MAX_CONTRIBUTION_CLIENTS} clients (the width of the sampled-client mask), "
                     f"got {int(world)}")
        coalition_count(mode, int(world), int(m))
    return MODES.index(mode)


def coalition_count(mode: str, K: int, perms: int = 0) -> int:
    """M, the coalitions of the mode's table for K clients."""
    if mode == "loo":
        M = K + 1
    elif mode != "shapley":
        raise ValueError(f"contribution must be 'loo' or 'shapley' here, got {mode!r}")
    elif K <= EXACT_MAX_K:
        M = 1 << K
    else:
        if int(perms) < 1:
            raise ValueError(f"contribution='shapley' with more than {EXACT_MAX_K} clients samples permutations: "
                             f"contribution_perms must be > 0, got {perms!r}")
        M = 1 + int(perms) * K
    if M > MAX_COALITIONS:
        raise ValueError(f"contribution={mode!r}: {M} coalitions, at most {MAX_COALITIONS} "
                         "(fewer contribution_perms)")
    return M


def coalition_perms(K: int, perms: int, seed: int = 0) -> np.ndarray:
    """``[perms, K]`` permutations of the clients, drawn once from ``numpy.random.default_rng(seed)``."""
    rng = np.random.default_rng(int(seed))
    return np.stack([rng.permutation(K) for _ in range(int(perms))]).astype(np.int64)


def coalition_masks(mode: str, K: int, perms: int = 0, seed: int = 0) -> np.ndarray:
    """The static table ``masks[M]`` (uint64): ``"loo"`` the full mask, then the full mask without client i;
    ``"shapley"`` with K <= 8 every mask at its own index; with K > 8 the empty mask followed by every
    permutation's K prefixes (prefix j of permutation p at ``1 + p K + j``)."""
    M = coalition_count(mode, K, perms)
    full = (1 << K) - 1
    if mode == "loo":
        tab = [full] + [full & ~(1 << i) for i in range(K)]
    elif K <= EXACT_MAX_K:
        tab = list(range(M))
    else:
        tab = [0]
        for p in coalition_perms(K, perms, seed):
            acc = 0
            for i in p:
                acc |= 1 << int(i)
                tab.append(acc)
    return np.array(tab, dtype=np.uint64)


def coalition_slices(M: int, n_blocks: int) -> int:
    """Row slices per coalition of the scoring launch (fl_common.h fl_coalition_slices): a function of the
    shapes alone, so the loss sum's order is the same on every machine."""
    return min(int(n_blocks), max(1, 256 // int(M)))


def _players(players, K: int) -> list:
    """Sorted client indices from an index list or a mask."""
    if isinstance(players, (int, np.integer)):
        return [i for i in range(K) if (int(players) >> i) & 1]
    return sorted(int(i) for i in players)


def shapley_exact(util_by_mask, players, K: Optional[int] = None) -> np.ndarray:
    """Exact Shapley values (float64 ``[K]``) of ``players`` (indices or a mask) under ``util_by_mask[mask]``
    (an array of ``2^K`` entries or any mapping): ``phi_i = sum over T within players \\ i of
    |T|! (n - |T| - 1)! / n! (u(T + i) - u(T))``.  Clients outside ``players`` score 0."""
    if K is None:
        K = int(math.log2(len(util_by_mask)))
    pl = _players(players, K)
    n, phi = len(pl), np.zeros(K, np.float64)
    wt = [math.factorial(t) * math.factorial(n - t - 1) / math.factorial(n) for t in range(n)]
    for sub in range(1 << n):
        T = sum(1 << pl[j] for j in range(n) if (sub >> j) & 1)
        size = bin(sub).count("1")
        uT = float(util_by_mask[T])
        for j in range(n):
            if not (sub >> j) & 1:
                phi[pl[j]] += wt[size] * (float(util_by_mask[T | (1 << pl[j])]) - uT)
    return phi


def shapley_permutations(util, perms, players) -> np.ndarray:
    """Permutation estimate (float64 ``[K]``): the mean over ``perms`` ``[m, K]`` of each player's marginal
    along the permutation restricted to ``players``.  ``util``: the ``1 + m K`` utilities of the prefix table
    (``coalition_masks``) as scored -- the utility at prefix j is that of the prefix's sampled members, so the
    marginal of an unsampled client is exactly 0 and is not counted."""
    perms = np.asarray(perms)
    m, K = perms.shape
    pl, util = set(_players(players, K)), np.asarray(util, np.float64)
    phi = np.zeros(K, np.float64)
    for p in range(m):
        prev = util[0]
        for j in range(K):
            i, cur = int(perms[p, j]), util[1 + p * K + j]
            if i in pl:
                phi[i] += cur - prev
                prev = cur
    return phi / m


def leave_one_out(util, players, K: Optional[int] = None) -> np.ndarray:
    """Leave-one-out scores (float64 ``[K]``) from the ``K + 1`` utilities of the ``"loo"`` table:
    ``u(S) - u(S \\ i)`` for the players, 0 for the others."""
    util = np.asarray(util, np.float64)
    K = len(util) - 1 if K is None else K
    phi = np.zeros(K, np.float64)
    for i in _players(players, K):
        phi[i] = util[0] - util[1 + i]
    return phi


def contribution_scores(mode: str, util, K: int, players, perms=None) -> np.ndarray:
    """The mode's scores from one round's utilities in table order."""
    if mode == "loo":
        return leave_one_out(util, players, K)
    if K <= EXACT_MAX_K:
        return shapley_exact(np.asarray(util, np.float64), players, K)
    return shapley_permutations(util, perms, players)


def contribution_history(mode: str, K: int, perms, loss_sum, correct, n_rows: int, sampled):
    """``contribution`` and ``contribution_acc``, float64 ``[rounds, K]``, from the rounds' coalition rows:
    ``u_loss = -(loss_sum / n)`` and ``u_acc = correct / n`` in float64, the round's players from ``sampled[r]``
    (a mask).  A round that was not scored (NaN loss sums) is a NaN row."""
    loss_sum, correct = np.asarray(loss_sum), np.asarray(correct)
    out = np.full((2, len(loss_sum), K), np.nan, np.float64)
    for r in range(len(loss_sum)):
        if correct[r, 0] < 0:
            continue
        utils = (-(loss_sum[r].astype(np.float64) / float(n_rows)), correct[r].astype(np.float64) / float(n_rows))
        for q, u in enumerate(utils):
            out[q, r] = contribution_scores(mode, u, K, int(sampled[r]), perms)
    return out[0], out[1]


# ---- host models of the kernels ----
def coalition_images_model(v, w, x, real, masks, sampled: int) -> np.ndarray:
    """``[M, Pimg]`` fp32 coalition images, bit for bit what ``fl_coalition_build_kernel`` stores: per mask the
    select-fold of ``v`` ``[K, Pimg]`` and of the weights ``w`` ``[K]`` over ``mask & sampled`` in client order
    from +0, one division; an empty coalition is ``x``; positions outside ``real`` are exact 0."""
    v, w, x = np.asarray(v, np.float32), np.asarray(w, np.float32), np.asarray(x, np.float32)
    out = np.zeros((len(masks), v.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for j, mk in enumerate(masks):
            eff = int(mk) & int(sampled)
            if eff == 0:
                out[j] = x
            else:
                num, den = np.zeros(v.shape[1], np.float32), np.float32(0.0)
                for i in range(v.shape[0]):
                    if (eff >> i) & 1:
                        num, den = num + v[i], np.float32(den + w[i])
                out[j] = num / den
    out[:, ~np.asarray(real, bool)] = 0.0
    return out


def logits_f64(flat, dims: Sequence[int], X) -> np.ndarray:
    """Float64 forward of the dense parameters ``flat`` (``named_parameters()`` order) on rows ``X``."""
    a, off = np.asarray(X, np.float64), 0
    flat = np.asarray(flat, np.float64)
    for l in range(len(dims) - 1):
        K, N = dims[l], dims[l + 1]
        W, b = flat[off:off + N * K].reshape(N, K), flat[off + N * K:off + N * K + N]
        off += N * K + N
        a = a @ W.T + b
        if l + 2 < len(dims):
            a = np.maximum(a, 0.0)
    return a


def utility_f64(z, y):
    """``(loss_sum, correct)`` of float64 logits ``z`` ``[n, C]``: the sum of the rows' softmax cross-entropies
    with the maximum subtracted, and the rows whose first-maximum argmax is the label."""
    z, y = np.asarray(z, np.float64), np.asarray(y)
    zm = z.max(1)
    loss = zm + np.log(np.exp(z - zm[:, None]).sum(1)) - z[np.arange(len(y)), y]
    return float(loss.sum()), int((z.argmax(1) == y).sum())

"""Byzantine attack models: what a client that is alive and malicious publishes instead of its update.

The defences of ``fedmi/fl/aggregate.py`` (coordinate-wise median, trimmed mean, multi-Krum, geometric
median) were published against specific attackers; this module is the specification of four of them as a
stage of the round, plus a data-poisoning one:

* ``sign_flip``  -- the client's own update reversed and scaled by ``s``;
* ``gauss``      -- its own model plus ``sigma`` times a standard normal per parameter;
* ``alie``       -- "A Little Is Enough" (Baruch, Baruch, Goldberg 2019): every coordinate ``z`` honest standard
  deviations below the honest mean, small enough to pass the median, the trimmed mean and Krum;
* ``ipm``        -- inner-product manipulation (Xie, Koyejo, Gupta 2020): ``-eps`` times the honest mean update,
  which turns the aggregate's inner product with the true update negative under the mean (large ``eps``) and
  breaks Krum and the median with a small one;
* ``label_flip`` -- no stage: a Byzantine client's shard labels become ``C - 1 - y`` when the shards are built.

The stage runs once per round, after the local steps and after any DP or compression kernel (a Byzantine
client obeys neither), before the screen, the robust rule, the secure-aggregation mask and the sum: where
``ClientGroup(tamper=...)`` is called (``tamper`` runs first if both are given).  It runs in a live round only.

With ``S_r`` the round's sampled clients, ``B_r = S_r & attack_clients``, ``H_r = S_r - attack_clients``,
``w_j`` client j's FedAvg weight in its buffer (1 in unweighted / robust mode, ``n_j / N_r`` under the weighted
mean), ``x`` the image the round trained from and ``m_j[p] = div(c_j[p], w_j)`` the model behind contribution
``c_j`` at real parameter ``p`` (division by 1.0 is exact), every ``k`` in ``B_r`` gets
``c_k[p] = mul(w_k, a_k[p])``::

    sign_flip   a_k = sub(x, mul(s, sub(m_k, x)))
    gauss       a_k = add(m_k, mul(sigma, n_k[p]))
    alie        mu  = div(sum_{j in H_r} m_j, float(|H_r|))                    sums from +0 in client order
                var = |H_r| >= 2 ? div(sum_{j in H_r} mul(d_j, d_j), float(|H_r| - 1)) : 0,  d_j = sub(m_j, mu)
                a_k = sub(mu, mul(z, sqrt(var)))                               the same vector for every bad client
    ipm         a_k = sub(x, mul(eps, sub(mu, x)))                             mu as above

Every operation is one round-to-nearest fp32 operation and nothing is contracted into a fused multiply-add:
:func:`attack_model` is the numpy model of the kernels (``fedmi/ops/csrc/fl_attack.hip``) over parameter
images, bit for bit.  The one exception is the normal of ``gauss``: dense parameter ``p`` takes lane ``p % 4``
of the Box-Muller pairs of Philox4x32-10 at counter ``(p // 4, round, k, ATTACK_STREAM)`` under
``seed_key(attack_seed)``, evaluated on the device as ``fl_dp.hip`` evaluates the DP noise (``u01``,
full-precision ``logf`` / ``sincosf``); the model rounds the float64 normal of ``fedmi/privacy/philox.py`` to
fp32.  Image padding, the metric tails, honest and unsampled clients' buffers are never written; nothing is
written when the round is not live, when ``B_r`` is empty and, for ``alie`` / ``ipm``, when ``H_r`` is empty.

:func:`attack_torch` is the same rule over dense contribution rows in the tensors' dtype: what the torch
engines run, and in float64 the oracle.
"""
from __future__ import annotations

import math
from statistics import NormalDist
from typing import Optional, Sequence

import numpy as np
import torch

from ..privacy.philox import ATTACK_STREAM, box_muller, philox4x32_10, seed_key

ATTACKS = ("none", "sign_flip", "gauss", "alie", "ipm", "label_flip")
# kinds with a stage of their own in the round (the kernels' kind argument is the index in ATTACKS)
DEVICE_ATTACKS = ("sign_flip", "gauss", "alie", "ipm")
COLLUDING_ATTACKS = ("alie", "ipm")    # one vector from the honest clients' statistics for every bad client
MAX_ATTACK_CLIENTS = 64                # width of the per-round sampled-client mask (fl_common.h FL_ATTACK_MAX_K)


def alie_z(n: int, f: int) -> float:
    """ALIE's default ``z`` for ``n`` clients of which ``f`` are Byzantine (Baruch et al. 2019, section 3):
    ``Phi^-1((n - f - s) / (n - f))`` with ``s = n // 2 + 1 - f`` the honest clients the attackers need on
    their side of the median."""
    n, f = int(n), int(f)
    s = n // 2 + 1 - f
    ratio = (n - f - s) / (n - f) if n > f else math.nan
    if not 0.0 < ratio < 1.0:
        raise ValueError(f"attack_z: the default z = Phi^-1((n - f - s) / (n - f)) is undefined for n = {n}, f = {f} "
                         f"(the ratio {ratio!r} is not inside (0, 1)); give an explicit attack_z")
    return NormalDist().inv_cdf(ratio)


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def attack_clients(cfg) -> tuple:
    """``cfg.attack_clients`` as a tuple of ints (validated by :func:`attack_id`)."""
    return tuple(int(k) for k in cfg.attack_clients)


def attack_id(cfg, world: Optional[int] = None) -> int:
    """Validate the attack fields; the attack's index in ``ATTACKS`` (0 = off).  ``world``: the federation's
    size when the caller knows it -- the client indices are checked against it, and one client switches the
    attack off, so nothing about the clients is refused there; None (the entry point, before the communicator
    exists) checks what can be checked without it."""
    if not isinstance(cfg.attack, str) or cfg.attack not in ATTACKS:
        raise ValueError(f"attack must be one of {ATTACKS}, got {cfg.attack!r}")
    try:
        with np.errstate(all="ignore"):
            s = float(np.float32(cfg.attack_scale)) if not isinstance(cfg.attack_scale, bool) else math.nan
    except (TypeError, ValueError):
        s = math.nan
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"attack_scale must be a finite number > 0 (in fp32), got {cfg.attack_scale!r}")
    if cfg.attack_z is not None:
        try:
            with np.errstate(all="ignore"):
                z = float(np.float32(cfg.attack_z)) if not isinstance(cfg.attack_z, bool) else math.nan
        except (TypeError, ValueError):
            z = math.nan
        if not math.isfinite(z):
            raise ValueError(f"attack_z must be None or a finite number (in fp32), got {cfg.attack_z!r}")
    if not _is_int(cfg.attack_seed) or not 0 <= int(cfg.attack_seed) < 2 ** 64:
        raise ValueError(f"attack_seed must be an integer in [0, 2**64), got {cfg.attack_seed!r}")
    try:
        bad = list(cfg.attack_clients)
    except TypeError:
        bad = None
    if bad is None or isinstance(cfg.attack_clients, (str, bytes)) or not all(_is_int(k) and int(k) >= 0 for k in bad):
        raise ValueError(f"attack_clients must be a sequence of client indices >= 0, got {cfg.attack_clients!r}")
    if len(set(int(k) for k in bad)) != len(bad):
        raise ValueError(f"attack_clients must be distinct, got {cfg.attack_clients!r}")
    kind = ATTACKS.index(cfg.attack)
    if not kind or (world is not None and int(world) <= 1):
        return 0
    if not bad:
        raise ValueError(f"attack_clients must name at least one client for attack={cfg.attack!r}")
    if world is not None:
        world = int(world)
        if max(int(k) for k in bad) >= world:
            raise ValueError(f"attack_clients must lie in [0, {world}) (the federation's clients), "
                             f"got {cfg.attack_clients!r}")
        if len(bad) >= world:
            raise ValueError(f"attack_clients must leave at least one client honest, got {len(bad)} of {world}")
        if cfg.attack == "alie" and cfg.attack_z is None:
            alie_z(world, len(bad))   # (raises, naming attack_z, where the default is undefined)
    return kind


def attack_params(cfg, world: int) -> dict:
    """What ``layout()["attack"]`` reports and the launches take: the kind, the bad clients, the fp32 scale and
    ALIE's ``z`` (the configured one, or the default computed once from ``world`` and the bad count)."""
    bad = attack_clients(cfg)
    if cfg.attack_z is not None:
        z = float(np.float32(cfg.attack_z))
    elif cfg.attack == "alie":
        z = float(np.float32(alie_z(world, len(bad))))
    else:
        z = 0.0
    return {"kind": cfg.attack, "clients": list(bad), "scale": float(np.float32(cfg.attack_scale)), "z": z}


def flip_labels(y, n_classes: int):
    """``label_flip``: the labels ``C - 1 - y`` of a Byzantine client's shard."""
    return (int(n_classes) - 1) - (y if isinstance(y, torch.Tensor) else np.asarray(y))


def _mask(sel, K: int, who: str) -> list:
    """K bools from K bools or from a collection of client indices."""
    sel = list(sel)
    if len(sel) == K and all(isinstance(b, (bool, np.bool_)) for b in sel):
        return [bool(b) for b in sel]
    if not all(_is_int(k) and 0 <= int(k) < K for k in sel):
        raise ValueError(f"{who}: needs {K} flags or client indices in [0, {K}), got {sel!r}")
    return [k in set(int(i) for i in sel) for k in range(K)]


def attack_normals(n_params: int, round_index: int, client: int, seed: int) -> np.ndarray:
    """Standard normals of dense parameters ``0 .. n_params - 1`` of bad client ``client`` in a round, float64
    (``dp_normals`` on ``ATTACK_STREAM``)."""
    n_params = int(n_params)
    nq = (n_params + 3) // 4
    ctr = np.empty((nq, 4), np.uint64)
    ctr[:, 0] = np.arange(nq, dtype=np.uint64)
    ctr[:, 1] = int(round_index) & 0xFFFFFFFF
    ctr[:, 2] = int(client) & 0xFFFFFFFF
    ctr[:, 3] = ATTACK_STREAM
    return box_muller(philox4x32_10(ctr, seed_key(seed))).reshape(-1)[:n_params]


def attack_model(stack, x, active: Sequence, bad: Sequence, kind: str, scale: float, z: float, real,
                 weights=None, seed: int = 0, round: int = 0, live: bool = True, dims=None) -> np.ndarray:
    """What the ``fl_attack`` launch leaves in the K buffers ``stack`` [K, >= Pimg] (fp32: the padded parameter
    image first, whatever follows -- the metric tails -- untouched), bit for bit except gauss's normal: a copy
    with the rows of the bad sampled clients rewritten at the real parameters (``real`` [Pimg] true) by the rule
    of the module docstring.  ``x`` [Pimg]: the image the round trained from; ``active`` / ``bad``: K flags, or
    client indices; ``weights`` [K]: the clients' fp32 FedAvg weights (None: all 1); ``scale`` / ``z`` are taken
    in fp32; ``live`` false: the round is past a stop, nothing is written.  ``gauss`` needs ``dims`` (the dense
    order of the normals) and draws ``(seed, round, client)``."""
    if kind not in DEVICE_ATTACKS:
        raise ValueError(f"attack_model: kind must be one of {DEVICE_ATTACKS}, got {kind!r}")
    out = np.array(np.asarray(stack, np.float32), copy=True, order="C")
    real = np.asarray(real, bool).reshape(-1)
    xv = np.ascontiguousarray(np.asarray(x, np.float32)).reshape(-1)
    K, n = out.shape[0], real.shape[0]
    if out.ndim != 2 or out.shape[1] < n or xv.shape[0] != n:
        raise ValueError("attack_model: needs [K, >= Pimg] buffers, a [Pimg] image x and Pimg flags")
    act, bd = _mask(active, K, "attack_model"), _mask(bad, K, "attack_model")
    w = np.ones(K, np.float32) if weights is None else np.ascontiguousarray(np.asarray(weights, np.float32))
    if w.shape != (K,):
        raise ValueError(f"attack_model: {w.shape} weights for {K} clients")
    B = [k for k in range(K) if act[k] and bd[k]]
    H = [k for k in range(K) if act[k] and not bd[k]]
    if not live or not B or (kind in COLLUDING_ATTACKS and not H):
        return out
    s32, z32 = np.float32(scale), np.float32(z)
    img = out[:, :n]

    def model_of(j):
        return img[j] if weights is None else img[j] / w[j]

    with np.errstate(all="ignore"):
        if kind in COLLUDING_ATTACKS:
            acc = np.zeros(n, np.float32)
            for j in H:
                acc = acc + model_of(j)
            mu = acc / np.float32(len(H))
            if kind == "alie":
                var = np.zeros(n, np.float32)
                if len(H) >= 2:
                    for j in H:
                        d = model_of(j) - mu
                        var = var + d * d
                    var = var / np.float32(len(H) - 1)
                a = mu - z32 * np.sqrt(var)
            else:
                a = xv - s32 * (mu - xv)
            for k in B:
                img[k] = np.where(real, a if weights is None else w[k] * a, img[k])
            return out
        if kind == "gauss":
            from ..models.mlp import dense_to_image, param_count
            if dims is None:
                raise ValueError("attack_model: kind='gauss' needs dims (the dense order of the normals)")
            P = param_count(list(dims))
            # image position -> dense parameter (padding: -1)
            pos = np.asarray(dense_to_image(np.arange(1, P + 1, dtype=np.float64), list(dims))).astype(np.int64) - 1
        for k in B:
            m = model_of(k)
            if kind == "sign_flip":
                a = xv - s32 * (m - xv)
            else:
                nz = np.zeros(n, np.float32)
                nz[pos >= 0] = attack_normals(P, round, k, seed)[pos[pos >= 0]].astype(np.float32)
                a = m + s32 * nz
            img[k] = np.where(real, a if weights is None else w[k] * a, img[k])
    return out


def attack_torch(rows: Sequence[torch.Tensor], x: torch.Tensor, active: Sequence, bad: Sequence, kind: str,
                 scale: float, z: float, n: int, weights=None, seed: int = 0, round: int = 0) -> None:
    """The rule over the K contribution rows ``rows`` (the ``n`` dense parameters first, in place, whatever
    follows untouched) in the rows' dtype -- fp32: what the torch engines run; float64: the oracle.  ``x`` [n]:
    the model the round trained from; ``weights``: the K FedAvg weights the rows carry (None: all 1); ``scale``
    and ``z`` are the fp32 values."""
    if kind not in DEVICE_ATTACKS:
        raise ValueError(f"attack_torch: kind must be one of {DEVICE_ATTACKS}, got {kind!r}")
    K, n = len(rows), int(n)
    act, bd = _mask(active, K, "attack_torch"), _mask(bad, K, "attack_torch")
    B = [k for k in range(K) if act[k] and bd[k]]
    H = [k for k in range(K) if act[k] and not bd[k]]
    if not B or (kind in COLLUDING_ATTACKS and not H):
        return
    dt = rows[0].dtype
    xv = x[:n].to(dt)
    s, zz = float(np.float32(scale)), float(np.float32(z))
    wt = None if weights is None else [torch.tensor(float(v), dtype=dt) for v in weights]

    def model_of(j):
        return rows[j][:n] if wt is None else rows[j][:n] / wt[j]

    if kind in COLLUDING_ATTACKS:
        acc = torch.zeros(n, dtype=dt)
        for j in H:
            acc = acc + model_of(j)
        mu = acc / float(len(H))
        if kind == "alie":
            var = torch.zeros(n, dtype=dt)
            if len(H) >= 2:
                for j in H:
                    d = model_of(j) - mu
                    var = var + d * d
                var = var / float(len(H) - 1)
            # (numpy's square root: correctly rounded, as the kernel's; torch's vectorised one is not everywhere)
            a = mu - zz * torch.as_tensor(np.sqrt(var.cpu().numpy())).to(var.device)
        else:
            a = xv - s * (mu - xv)
        for k in B:
            rows[k][:n] = a if wt is None else wt[k] * a
        return
    for k in B:
        m = model_of(k)
        if kind == "sign_flip":
            a = xv - s * (m - xv)
        else:
            a = m + s * torch.as_tensor(attack_normals(n, round, k, seed)).to(dt)
        rows[k][:n] = a if wt is None else wt[k] * a

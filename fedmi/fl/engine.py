"""Round engines: one federated client's local train -> local eval -> FedAvg loop.

Two implementations with one interface and identical semantics:

* :class:`HipRoundEngine` -- the MI355X path.  Shard, flat parameters, Adam state, gradient
  slab, round state and metric history are device-resident; each round is three fused
  gfx950 kernels plus one RCCL all-reduce issued from C++ (``fedmi/ops/csrc``), optionally
  replayed as a captured HIP graph.  Early stopping is evaluated on the device.
* :class:`TorchRoundEngine` -- eager torch ops (``nn.Linear``, ``CrossEntropyLoss``,
  ``torch.optim.Adam`` + ``StepLR``), i.e. the reference's own numerics
  (``FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py:30-120``).  Used on CPU (the
  gloo plumbing config) and as the oracle the HIP kernels are tested against.

Round semantics (reference-compat): ``local_steps`` full-batch Adam steps
(reference: 1), StepLR stepped once per round, Adam moments never reset, local metrics of
the post-step model on the local *training* shard, global metrics = mean over clients of
local metrics (``metric_mode='mean'``, Q3) or pooled confusion (``'pooled'``, Q4),
weights averaged with weights n_i / N (C:110-116), early stop with patience/atol on the
4-metric vector (C:181-192).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field, asdict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ..models.mlp import (MLPModel, dense_to_image, flat_to_dict, image_layout, image_to_dense,
                          param_count)
from .aggregate import (AGGREGATORS, ALL_AGGREGATORS, GEOMED_MAX_ITERS, MAX_ROBUST_CLIENTS, SCREENS, _AggLaunch,
                        geomed_torch, mask_bits, pair_distances_torch, robust_aggregate_torch, screen_select)
from .attack import (ATTACKS, DEVICE_ATTACKS, MAX_ATTACK_CLIENTS, attack_clients, attack_id, attack_params,
                     attack_torch)
from .compress import COMPRESSORS, RANDOM_COMPRESSORS, compress_id, compress_k, compress_torch, uplink_bytes
from .early_stop import EarlyStopper
from .metrics import METRIC_NAMES, confusion_matrix, metrics_from_confusion, metric_vector
from .secagg import (MAX_SECAGG_CLIENTS, SECAGG_STREAM, secagg_id, secagg_mask, secagg_open,
                     secagg_quantize)


# bf16 shards of at most this many rows default to 16 rows per workgroup (EngineConfig.rows_per_block = 0):
# measured on MI355X (profiles/round_emulate_r4_shards.log), R = 16 wins at 1000 and 2000 rows,
# R = 32 at 4000 and 8000.
SMALL_SHARD_ROWS = 2000
# Local steps per round the native engine takes: a round's launches are planned into a fixed array
# (fedmi/ops/csrc/fl_round_plan.h FL_PLAN_MAX_LOCAL_STEPS).  The torch engine has no limit.
MAX_LOCAL_STEPS = 61


@dataclass
class EngineConfig:
    hidden: Sequence[int] = (50, 200)
    lr: float = 0.004
    betas: Sequence[float] = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.0
    step_size: int = 30
    gamma: float = 0.5
    local_steps: int = 1            # full-batch Adam steps per round (HIP engine: at most MAX_LOCAL_STEPS = 61)
    prox_mu: float = 0.0
    early_stop: bool = True
    patience: int = 10
    tolerance: float = 1e-4
    rtol: float = 1e-5
    max_rounds: int = 300
    metric_mode: str = "mean"       # 'mean' (C:169) | 'pooled' (S:130)
    rows_per_block: int = 0         # R rows per workgroup of the fused kernels (16 | 32 | 64 (bf16); 0 = auto:
                                    # 16 for bf16 shards of <= SMALL_SHARD_ROWS rows, else 32 if it fits LDS, else 16;
                                    # -1 = the largest that fits, 64 first (bf16))
    graph_rounds: int = 16          # rounds per captured HIP graph (0 = eager launches)
    seed: int = 0
    # partial participation (client sampling): each round max(1, round(participation * world))
    # clients, drawn by numpy's default Generator seeded with (seed, round) so every rank
    # draws the same set, train and are averaged (weights n_i / sum of the sampled n_i); the
    # others skip the local step and take the new global model.  The LR schedule follows the
    # round index for everyone, Adam's bias correction each client's own step count; global
    # metrics and loss are the sampled clients'.  Both engines (HIP: a per-round device table).
    participation: float = 1.0
    debug: bool = False             # eager, synchronised phases + non-finite checks every round
    dtype: str = "fp32"             # MFMA operand type of the fused kernels: 'fp32' | 'bf16'
    # one client: score round r's post-step model inside round r+1's train kernel (its forward
    # pass IS that evaluation, FedAvg of one client being the identity) instead of a separate
    # eval kernel; metrics, history and early stop are unchanged (fl_common.h FL_EVAL_FUSED)
    fused_eval: bool = True
    # world > 1 with the one-shot xGMI all-reduce: evaluate the post-step local model and
    # all-reduce in ONE kernel, the weights' all-reduce overlapping the evaluation
    # (fedmi/ops/csrc/peer_device.h); False = separate eval and all-reduce kernels
    eval_fedavg: bool = True
    # world > 1, bf16: score round r's post-step local model inside round r+1's train kernel --
    # no evaluation kernel in the round; the counts are exchanged inside round r+1's Adam
    # kernel (one-shot xGMI) or ride round r+1's all-reduce (RCCL; with early stopping a round
    # run past the stop is discarded bit-exactly, fl_common.h FLState::late); the
    # last round of every run() evaluates itself (fl_common.h FL_EVAL_LAGGED).  Metrics,
    # history, early-stop round and weights are identical to classic rounds.
    lagged_eval: bool = True
    # bf16 fused kernels: storage of the per-workgroup gradient partials reduced by the Adam
    # kernel -- 'fp16' (half the slab traffic; partial SUMS of the unscaled gradient, 1/n applied
    # after the fp32 reduction, saturating at +-65504), 'fp32', or 'auto' = fp16 when every
    # |feature| <= FP16_SLAB_MAX_ABS_X (standardised data: a partial over R <= 64 rows stays far
    # inside fp16's range), else fp32.  The fp32 kernels always use an fp32 slab.
    grad_slab: str = "auto"
    # bf16 kernels, several clients: run the TRAINING forward pass in plain bf16 (a_hi.W_hi) instead
    # of split-bf16 -- no round is scored from it there (lagged rounds score in registers, classic
    # rounds in the eval kernel, both split-bf16); None = auto (on for world > 1 / emulated
    # clients with register scoring), False = the split forward everywhere, True = on where it is
    # valid (never for one fused client, whose evaluation IS the training forward).  The engine's
    # layout()["plain_fwd"] reports what runs; bench records and checkpoints carry it.
    plain_fwd: Optional[bool] = None
    # Client-level differential privacy (DP-FedAvg with distributed noise; fedmi/privacy): every
    # sampled client clips its round update D = local - (the image the round trained from) to
    # ||D||_2 <= dp_clip and adds N(0, sigma_r^2 I), sigma_r = dp_noise * dp_clip * max_j w_j(r) /
    # sqrt(K_r), to its FedAvg contribution w_i (x + c D) BEFORE the exchange, so the all-reduced sum
    # carries noise of dp_noise times its sensitivity to one client and no rank sees an un-noised
    # peer update.  dp_clip = 0: off (nothing of a round changes).  dp_noise needs dp_clip > 0;
    # dp_noise = 0 is clipping only.  dp_seed: None = a private 64-bit seed per rank from
    # os.urandom (kept in the portable state, so a resume continues the stream), an int =
    # reproducible runs.  The local model, Adam moments, local metrics are untouched; rounds are
    # classic (no fused / lagged evaluation); history()["update_norm"] holds the pre-clip norms.
    dp_clip: float = 0.0
    dp_noise: float = 0.0
    dp_seed: Optional[int] = None
    # Server optimizer (Hsu et al. 2019, FedAvgM; Reddi et al. 2021, FedAdagrad / FedAdam / FedYogi):
    # with x the image a round trained from and a its aggregated image (after the all-reduce, so
    # after DP clip + noise), d = a - x is a pseudo-gradient and the next global image is
    #   "sgd":     m = b1 m + d;            x + lr m
    #   "adagrad": m = b1 m + (1 - b1) d;   v = v + d^2;                          x + lr m / (sqrt(v) + tau)
    #   "adam":    same m;                  v = b2 v + (1 - b2) d^2;              same step
    #   "yogi":    same m;                  v = v - (1 - b2) d^2 sign(v - d^2);   same step
    # with b1 = server_momentum, b2 = server_beta2, lr = server_lr, tau = server_tau; m starts at 0, v
    # at tau^2, no bias correction.  Every rank computes the same step on the same all-reduced image
    # (no extra communication), so every client must start from the same model (FederatedMLPLearning
    # and ClientGroup seed it so).  "none": off (nothing of a round changes).  The local models, client
    # Adam moments, local metrics and the early-stop rule are untouched; rounds are classic.
    server_opt: str = "none"
    server_lr: float = 1.0
    server_momentum: float = 0.9
    server_beta2: float = 0.99
    server_tau: float = 1e-3
    # Aggregation rule (fedmi/fl/aggregate.py): "mean" = the sample-weighted FedAvg above (nothing of a
    # round changes); "median" / "trimmed_mean" = the coordinate-wise median / beta-trimmed mean of the
    # round's sampled clients' UNWEIGHTED local models (Yin et al. 2018), robust against clients that
    # are alive and wrong (NaN, sign flips, scaling).  trim_ratio = beta, the fraction cut at EACH end
    # (t = floor(beta K_r) of K_r sampled clients; "trimmed_mean" only).  Metric tails, history and
    # the early-stop rule are unchanged; a server optimizer steps from the robust aggregate; rounds are
    # classic.  Not with dp_clip > 0 (the noise calibration assumes a weighted sum), trial batches or
    # WideClient; at most 64 clients.
    # "geomed" = the geometric median of the sampled clients' unweighted local models (Pillutla et al.
    # 2022, RFA): a whole-vector rule that needs no Byzantine count, breakdown point 1/2, every client
    # pulling with at most unit force.  geomed_iters smoothed Weiszfeld iterations from the coordinate-wise
    # median, weights 1 / max(geomed_nu, distance); geomed_iters + 1 launches per round (fl_geomed.hip).
    # Composes as the median does; on a multi-rank HipRoundEngine over the host gather only
    # (gather_plane="xgmi" is refused: the one-shot select kernel cannot iterate).
    aggregator: str = "mean"
    trim_ratio: float = 0.1
    geomed_iters: int = 3
    geomed_nu: float = 1e-6
    # Update compression with error feedback (fedmi/fl/compress.py): every sampled client compresses
    # u = (local - x) + e (x: the image the round trained from, e: its residual) before the exchange and
    # contributes w (x + C(u)); what C drops stays in e (error_feedback=False: it is discarded).  "topk"
    # keeps the k = max(1, min(P, ceil(compress_ratio P))) entries of largest |u| (Stich et al. 2018),
    # "sign" sends copysign(mean |u|, u) (Karimireddy et al. 2019); both are deterministic.  A SIMULATION
    # of the uplink: the exchange still carries the dense fp32 image, layout()["compress"] /
    # compress.uplink_bytes report what a real uplink would carry.  "none": off (nothing of a round
    # changes).  The local model, Adam moments, FedProx anchor and local metrics are untouched; rounds
    # are classic; history()["compress_stat"] holds the k-th kept magnitude (top-k) / the scale (sign).
    # Two stochastic compressors draw Philox words of (compress_seed, round, client): "qsgd" quantises
    # |u| / ||u||_2 to compress_levels = s levels with stochastic rounding (Alistarh et al. 2017, one
    # bucket; unbiased; compress_stat = the norm), "randk" keeps k random entries (k as for top-k; the
    # indices follow from the seed, so only the values travel; with error_feedback the memory variant,
    # without it the kept entries are scaled by P / k, the unbiased variant; compress_stat = the
    # selection's quantile).  compress_seed: None = a private 64-bit draw per client (kept in the portable
    # state, so a resume continues the stream), an int in [0, 2**64) = reproducible runs.
    # Not with dp_clip > 0, trial batches (comm_buffers), fed_sweep or WideClient.
    compress: str = "none"
    compress_ratio: float = 0.1
    error_feedback: bool = True
    compress_levels: int = 127
    compress_seed: Optional[int] = None
    # Secure aggregation (fedmi/fl/secagg.py; Bonawitz et al. 2017): every sampled client quantises its
    # weighted contribution to fixed point with secagg_bits fractional bits and adds / subtracts one
    # Philox mask per pair of the round's sampled clients (mod 2^32) before the exchange; the masks
    # cancel in the sum, so a peer sees uniform words and only the sum opens.  A SIMULATION of the
    # protocol's arithmetic: all pair masks derive from one shared group seed (secagg_seed; None = one
    # draw per group / rank 0's draw), there is no key agreement, dropout recovery or malicious-server
    # round.  The opened image does not depend on the seed (config only, never state).  Metric tails stay
    # clear floats.  False: off (nothing of a round changes); one client: the identity.  Composes with
    # dp_clip / dp_noise, compress, server_opt, participation, prox_mu, local_steps, early_stop, both
    # dtypes; rounds are classic and aggregated over the host gather; history()["secagg_clamped"] counts
    # this client's clamped / NaN coordinates.  Not with a robust aggregator, more than 64 clients, trial
    # batches (comm_buffers), fed_sweep or WideClient.
    secagg: bool = False
    secagg_bits: int = 24
    secagg_seed: Optional[int] = None
    # Data plane of a robust aggregator / secure aggregation on a multi-rank HipRoundEngine: "host" = every
    # rank's buffer gathered over the host plane, the rule launched from Python (aggregation 'host-gather');
    # "xgmi" = the one-shot xGMI peer kernel selects / opens instead of summing (peer_allreduce.hip
    # peer_select_kernel; aggregation 'xgmi-select'): the native engine aggregates, so rounds are traced and
    # graph-captured like any peer engine's.  At most 8 ranks; if the peer set-up fails on every rank they
    # warn and continue on the host gather.  A run-time choice, not state: results are bitwise equal on both
    # planes.  Ignored by every other engine kind (one client, the weighted mean, ClientGroup, torch).
    gather_plane: str = "host"
    # Client screening in front of the aggregator (fedmi/fl/aggregate.py): "multi_krum" (Blanchard et al.
    # 2017) keeps, per round, the screen_keep sampled clients whose WHOLE models lie closest to their
    # K_r - screen_byzantine - 2 nearest neighbours (squared distance), and the aggregator runs over the
    # kept clients only.  screen_byzantine = f, the Byzantine clients assumed: every round needs
    # K_r >= 2 f + 3 sampled clients.  screen_keep = m in [1, min_r K_r - f]; None = K_r - f; 1 = Krum.
    # Screening turns the unweighted (robust) mode on: with aggregator="mean" the kept clients' models
    # are averaged UNWEIGHTED (the paper's multi-Krum; sample sizes are self-reported), "median" /
    # "trimmed_mean" run over the kept set with K_r replaced by the number kept.  Metric tails, history
    # and the early-stop rule see every sampled client: rejecting a model does not drop its metrics.
    # history()["screen_kept"] holds each round's kept mask (bit k = client k).  "none": off (nothing of a
    # round changes); one client: off.  Not with secagg, dp_clip > 0, gather_plane="xgmi", more than 64
    # clients, trial batches (comm_buffers), fed_sweep or WideClient.
    screen: str = "none"
    screen_byzantine: int = 0
    screen_keep: Optional[int] = None
    # Byzantine attack model (fedmi/fl/attack.py, the specification): the clients / ranks attack_clients are
    # Byzantine and publish, every round they are sampled in, "sign_flip": their own update reversed and scaled
    # by attack_scale; "gauss": their model plus attack_scale * N(0, I) (Philox words of (attack_seed, round,
    # client)); "alie": the honest sampled clients' mean minus attack_z of their standard deviations in every
    # coordinate (Baruch et al. 2019; attack_z None = the paper's z for world clients, computed once); "ipm":
    # the round's input image minus attack_scale times the honest mean update (Xie et al. 2020).  One launch per
    # round (fl_attack.hip) after the local steps and any DP / compression kernel, before the screen, the
    # robust rule, the secure-aggregation mask and the sum -- where ClientGroup(tamper=...) is called.
    # "label_flip": no launch; a Byzantine client trains on the labels C - 1 - y (ClientGroup and
    # FederatedMLPLearning flip them when the shards are built).  "none": off (nothing of a round changes); one
    # client: off.  The launched kinds need the individual contributions: ClientGroup (every rule), or a
    # multi-rank engine on the host gather (a robust rule or a screen, gather_plane="host"); they make every
    # client start from one common model, as server_opt does.  Not with more than 64 clients, trial batches
    # (comm_buffers), fed_sweep or WideClient.  attack_seed is config, not state.
    attack: str = "none"
    attack_clients: Sequence[int] = ()
    attack_scale: float = 1.0
    attack_z: Optional[float] = None
    attack_seed: int = 0

    def to_dict(self) -> dict:
        d = asdict(self)
        d["hidden"] = list(self.hidden)
        d["betas"] = list(self.betas)
        if self.attack == "none":
            # (off: a checkpoint's config record is what it was before the attack fields existed)
            for k in ("attack", "attack_clients", "attack_scale", "attack_z", "attack_seed"):
                del d[k]
        else:
            d["attack_clients"] = [int(k) for k in self.attack_clients]
        return d


def _metric_mode_id(mode: str) -> int:
    if mode not in ("mean", "pooled"):
        raise ValueError(f"metric_mode must be 'mean' or 'pooled', got {mode!r}")
    return 0 if mode == "mean" else 1


# grad_slab='auto': the largest |feature| for which the bf16 kernels use fp16 gradient partials
FP16_SLAB_MAX_ABS_X = 64.0


def _dtype_id(dtype: str) -> int:
    if dtype not in ("fp32", "bf16"):
        raise ValueError(f"dtype must be 'fp32' or 'bf16', got {dtype!r}")
    return 0 if dtype == "fp32" else 1


def dp_enabled(cfg: EngineConfig) -> bool:
    """Validate the DP fields; True when differential privacy is on (``dp_clip > 0``)."""
    S, z = float(cfg.dp_clip), float(cfg.dp_noise)
    if not (math.isfinite(S) and S >= 0.0):
        raise ValueError(f"dp_clip must be a finite number >= 0, got {cfg.dp_clip!r}")
    if not (math.isfinite(z) and z >= 0.0):
        raise ValueError(f"dp_noise must be a finite number >= 0, got {cfg.dp_noise!r}")
    if z > 0.0 and S == 0.0:
        raise ValueError("dp_noise > 0 needs dp_clip > 0 (the noise is scaled by the clipping bound)")
    if cfg.dp_seed is not None and not (0 <= int(cfg.dp_seed) < 2 ** 64):
        raise ValueError(f"dp_seed must be None or an integer in [0, 2**64), got {cfg.dp_seed!r}")
    return S > 0.0


SERVER_OPTS = ("none", "sgd", "adagrad", "adam", "yogi")


def server_opt_id(cfg: EngineConfig) -> int:
    """Validate the server-optimizer fields; the optimizer's index in ``SERVER_OPTS`` (0 = off)."""
    if cfg.server_opt not in SERVER_OPTS:
        raise ValueError(f"server_opt must be one of {SERVER_OPTS}, got {cfg.server_opt!r}")
    lr, b1, b2, tau = (float(cfg.server_lr), float(cfg.server_momentum), float(cfg.server_beta2),
                       float(cfg.server_tau))
    if not (math.isfinite(lr) and lr > 0.0):
        raise ValueError(f"server_lr must be a finite number > 0, got {cfg.server_lr!r}")
    if not 0.0 <= b1 < 1.0:
        raise ValueError(f"server_momentum must be in [0, 1), got {cfg.server_momentum!r}")
    if not 0.0 <= b2 < 1.0:
        raise ValueError(f"server_beta2 must be in [0, 1), got {cfg.server_beta2!r}")
    kind = SERVER_OPTS.index(cfg.server_opt)
    if kind >= 2 and not (math.isfinite(tau) and tau > 0.0):
        raise ValueError(f"server_tau must be a finite number > 0 for server_opt={cfg.server_opt!r}, "
                         f"got {cfg.server_tau!r}")
    return kind


def aggregator_id(cfg: EngineConfig, world: Optional[int] = None) -> int:
    """Validate the aggregation fields; the rule's index in ``ALL_AGGREGATORS`` (0 = the weighted mean).
    ``world``: the federation's size when the caller knows it -- the aggregate of one client is the
    identity, so no combination is refused there."""
    if not isinstance(cfg.aggregator, str) or cfg.aggregator not in ALL_AGGREGATORS:
        raise ValueError(f"aggregator must be one of {ALL_AGGREGATORS}, got {cfg.aggregator!r}")
    T = cfg.geomed_iters
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or not 1 <= int(T) <= GEOMED_MAX_ITERS:
        raise ValueError(f"geomed_iters must be an integer in [1, {GEOMED_MAX_ITERS}], got {T!r}")
    try:
        nu = float(np.float32(cfg.geomed_nu)) if not isinstance(cfg.geomed_nu, bool) else math.nan
    except (TypeError, ValueError):
        nu = math.nan
    if not (math.isfinite(nu) and nu > 0.0):
        raise ValueError(f"geomed_nu must be a finite number > 0 (in fp32), got {cfg.geomed_nu!r}")
    try:
        beta = float(cfg.trim_ratio)
    except (TypeError, ValueError):
        beta = math.nan
    if not (math.isfinite(beta) and 0.0 <= beta < 0.5):
        raise ValueError(f"trim_ratio must be a finite number in [0, 0.5), got {cfg.trim_ratio!r}")
    kind = ALL_AGGREGATORS.index(cfg.aggregator)
    if kind and float(cfg.dp_clip) > 0.0:
        raise ValueError(f"aggregator={cfg.aggregator!r} does not combine with differential privacy (dp_clip > 0): "
                         "the noise calibration assumes a weighted sum")
    if cfg.aggregator == "geomed" and cfg.gather_plane == "xgmi" and (world is None or int(world) > 1):
        raise ValueError("aggregator='geomed' does not run on gather_plane='xgmi': the one-shot select kernel "
                         "cannot iterate; use gather_plane='host'")
    return kind


def screen_id(cfg: EngineConfig, world: Optional[int] = None) -> int:
    """Validate the screening fields and what a screen does not combine with; the screen's index in
    ``SCREENS`` (0 = off).  ``world``: the federation's size when the caller knows it -- one client
    switches the screen off, so nothing is refused there; None (the entry point, before the
    communicator exists) checks the combinations as for several clients.  The per-round bounds
    (``K_r >= 2 f + 3``, ``screen_keep <= K_r - f``) need the sampled counts: the engines check them."""
    if not isinstance(cfg.screen, str) or cfg.screen not in SCREENS:
        raise ValueError(f"screen must be one of {SCREENS}, got {cfg.screen!r}")
    f, m = cfg.screen_byzantine, cfg.screen_keep
    if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or int(f) < 0:
        raise ValueError(f"screen_byzantine must be an integer >= 0, got {f!r}")
    if m is not None and (isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) < 1):
        raise ValueError(f"screen_keep must be None or an integer >= 1, got {m!r}")
    kind = SCREENS.index(cfg.screen)
    if not kind or (world is not None and int(world) <= 1):
        return 0
    if bool(cfg.secagg):
        raise ValueError(f"screen={cfg.screen!r} does not combine with secagg: screening needs the individual "
                         "models, secure aggregation opens only their sum")
    if float(cfg.dp_clip) > 0.0:
        raise ValueError(f"screen={cfg.screen!r} does not combine with differential privacy (dp_clip > 0): "
                         "the noise calibration assumes a weighted sum")
    if cfg.gather_plane == "xgmi":
        raise ValueError(f"screen={cfg.screen!r} does not run on gather_plane='xgmi': the one-shot select kernel "
                         "never holds the stack of client models the pairwise distances need; use gather_plane='host'")
    return kind


def attack_stage(cfg: EngineConfig, world: Optional[int] = None) -> bool:
    """Validate the attack fields (``attack_id``); True when the attack is a stage of the round (a launch over
    the clients' contributions: every kind but ``"label_flip"``)."""
    return ATTACKS[attack_id(cfg, world)] in DEVICE_ATTACKS


def common_init(cfg: EngineConfig) -> bool:
    """Every client starts from one model: a server optimizer and the attack stage both read the image a round
    trained from, which must be the same on every replica from round 0 on."""
    return cfg.server_opt != "none" or cfg.attack in DEVICE_ATTACKS


GATHER_PLANES = ("host", "xgmi")


def gather_plane_id(cfg: EngineConfig) -> int:
    """Validate ``gather_plane``; the plane's index in ``GATHER_PLANES`` (0 = the host gather)."""
    if not isinstance(cfg.gather_plane, str) or cfg.gather_plane not in GATHER_PLANES:
        raise ValueError(f"gather_plane must be one of {GATHER_PLANES}, got {cfg.gather_plane!r}")
    return GATHER_PLANES.index(cfg.gather_plane)


def server_step(kind: int, cfg: EngineConfig, x: torch.Tensor, a: torch.Tensor, m: torch.Tensor,
                v: Optional[torch.Tensor]) -> torch.Tensor:
    """One server-optimizer step in the tensors' dtype: updates ``m`` (and ``v``) in place and
    returns the new global parameters.  The operation order is fl_server.hip's (which fuses
    ``b1 m + .``, ``v + d^2``, ``b2 v + .`` and ``x + lr .`` into single roundings)."""
    dt = x.dtype
    sc = lambda s: torch.tensor(float(s), dtype=torch.float32).to(dt)   # the kernel's fp32 scalars
    lr, b1, b2, tau = sc(cfg.server_lr), sc(cfg.server_momentum), sc(cfg.server_beta2), sc(cfg.server_tau)
    omb1 = sc(1.0 - float(cfg.server_momentum))
    omb2 = sc(1.0 - float(cfg.server_beta2))
    d = a - x
    if kind == 1:
        m.mul_(b1).add_(d)
        return x + lr * m
    m.mul_(b1).add_(omb1 * d)
    d2 = d * d
    if kind == 2:
        v.add_(d2)
    elif kind == 3:
        v.mul_(b2).add_(omb2 * d2)
    else:
        v.sub_(omb2 * d2 * torch.sign(v - d2))
    return x + lr * (m / (v.sqrt() + tau))


# Held-out rows an engine scores per round (fedmi/ops/csrc/fl_common.h FL_HELDOUT_MAX_ROWS).
HELDOUT_MAX_ROWS = 1 << 24


def heldout_metrics(history: dict) -> np.ndarray:
    """``[rounds_run, 4]`` accuracy / precision / recall / F1 (``metrics_from_confusion``) of the global
    model on the held-out set, round by round, from ``history()["heldout_cm"]``."""
    if "heldout_cm" not in history:
        raise KeyError("history has no held-out rows: call set_heldout(X, y) before the rounds")
    cm = np.asarray(history["heldout_cm"])
    if len(cm) == 0:
        return np.zeros((0, 4))
    return np.stack([metric_vector(metrics_from_confusion(c)) for c in cm])


def _softmax_ce_rows(z: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Per-row softmax cross-entropy lse(z) - z[y] in the logits' dtype."""
    return torch.logsumexp(z, 1) - z.gather(1, y.view(-1, 1)).squeeze(1)


class _History:
    # held-out scoring (set_heldout): per round the global model's confusion counts and fp32 loss SUM on
    # the n held-out rows, and the round with the smallest sum (-1: none yet); None: off
    ho_cm = None
    ho_loss = None
    ho_best_round = -1
    ho_n = 0

    def enable_heldout(self, n_classes: int, n_rows: int) -> None:
        if self.ho_cm is None:
            mr = len(self.loss)
            self.ho_cm = np.zeros((mr, n_classes, n_classes), dtype=np.int64)
            self.ho_loss = np.zeros(mr, dtype=np.float32)
        self.ho_n = int(n_rows)

    def __init__(self, max_rounds: int, world: int, dp: bool = False, compress: bool = False,
                 secagg: bool = False, screen: bool = False):
        # screening engines: the round's kept-client mask, bit k = client k (0: the round did not run)
        self.screen = np.zeros(max_rounds, dtype=np.uint64) if screen else None
        # secure aggregation: this client's clamped / NaN coordinates per round (0: not sampled)
        self.clamped = np.zeros(max_rounds, dtype=np.int64) if secagg else None
        # DP engines: this client's pre-clip update norm per round (0: not sampled)
        self.norm = np.zeros(max_rounds, dtype=np.float32) if dp else None
        # compressing engines: the round's statistic (top-k: k-th kept magnitude; sign: scale; qsgd: norm; rand-k: the selection's quantile; 0: not sampled)
        self.cstat = np.zeros(max_rounds, dtype=np.float32) if compress else None
        self.glob = np.zeros((max_rounds, 4))
        self.rank = np.zeros((max_rounds, world, 4))
        self.loss = np.zeros(max_rounds, dtype=np.float32)
        self.rounds_run = 0
        self.stop_round = -1       # round index at which training stopped early (-1: never)
        self.stop_trigger = -1     # round whose metrics triggered the stop

    def as_dict(self) -> dict:
        n = self.rounds_run
        out = {
            "rounds_run": n,
            "stop_round": self.stop_round,
            "stop_trigger": self.stop_trigger,
            "global": self.glob[:n].copy(),
            "per_rank": self.rank[:n].copy(),
            "loss": self.loss[:n].copy(),
        }
        if self.norm is not None:
            out["update_norm"] = self.norm[:n].copy()
        if self.cstat is not None:
            out["compress_stat"] = self.cstat[:n].copy()
        if self.clamped is not None:
            out["secagg_clamped"] = self.clamped[:n].copy()
        if self.screen is not None:
            out["screen_kept"] = self.screen[:n].copy()
        if self.ho_cm is not None:
            out["heldout_cm"] = self.ho_cm[:n].copy()
            out["heldout_loss_sum"] = self.ho_loss[:n].copy()
            out["heldout_loss"] = self.ho_loss[:n].astype(np.float64) / float(max(self.ho_n, 1))
            out["heldout_best_round"] = int(self.ho_best_round)
        return out

    def global_metrics_dict(self) -> Dict[str, List[float]]:
        """Same structure as the reference's returned ``global_metrics`` (C:124)."""
        n = self.rounds_run
        return {k: [float(x) for x in self.glob[:n, i]] for i, k in enumerate(METRIC_NAMES)}


class RoundEngineBase:
    def __init__(self, X: np.ndarray, y: np.ndarray, n_classes: int, cfg: EngineConfig, comm,
                 init_flat: np.ndarray, n_total: Optional[int] = None, client_sizes=None):
        self.cfg = cfg
        self.dp = dp_enabled(cfg)
        self.server = server_opt_id(cfg)   # index in SERVER_OPTS; 0 = plain FedAvg
        self.compress = compress_id(cfg)   # index in ALL_COMPRESSORS; 0 = dense contributions
        # the stochastic kinds carry one more piece of state: the client's seed (config, or a private draw)
        self.compress_random = cfg.compress in RANDOM_COMPRESSORS
        if self.compress_random:
            self.compress_seed = (int.from_bytes(os.urandom(8), "little") if cfg.compress_seed is None
                                  else int(cfg.compress_seed))
        gather_plane_id(cfg)               # validated by every engine; only a multi-rank HIP engine reads it
        self.comm = comm
        self.world = comm.size if comm is not None else 1
        self.rank = comm.rank if comm is not None else 0
        # index in ALL_AGGREGATORS, 0 = the weighted mean; the aggregate of one client is the identity
        kind = aggregator_id(cfg, self.world)
        self.robust = kind if self.world > 1 else 0
        if self.robust and self.world > MAX_ROBUST_CLIENTS:
            raise ValueError(f"aggregator={cfg.aggregator!r} takes at most {MAX_ROBUST_CLIENTS} clients "
                             f"(the width of the sampled-client mask), got {self.world}")
        # index in SCREENS, 0 = no screening; one client: off.  A screen turns the unweighted mode on
        # whatever the aggregator: "mean" over the kept clients is the trimmed-mean kind with beta = 0
        self.screen = screen_id(cfg, self.world)
        self.robust_beta = float(cfg.trim_ratio)
        if self.screen:
            if self.world > MAX_ROBUST_CLIENTS:
                raise ValueError(f"screen={cfg.screen!r} takes at most {MAX_ROBUST_CLIENTS} clients "
                                 f"(the width of the sampled-client mask), got {self.world}")
            if not self.robust:
                self.robust, self.robust_beta = AGGREGATORS.index("trimmed_mean"), 0.0
            f = int(cfg.screen_byzantine)
            k_min = self.sampled_count()   # every round samples that many: no round needs a look
            if k_min < 2 * f + 3:
                raise ValueError(f"screen={cfg.screen!r} with screen_byzantine={f} needs at least 2 f + 3 = {2 * f + 3} "
                                 f"sampled clients in every round, a round has {k_min}")
            if cfg.screen_keep is not None and not 1 <= int(cfg.screen_keep) <= k_min - f:
                raise ValueError(f"screen_keep must be in [1, {k_min - f}] (the fewest sampled clients of a round "
                                 f"minus screen_byzantine), got {cfg.screen_keep!r}")
        # secure aggregation: 1 = masked fixed-point contributions; one client is the identity
        on = secagg_id(cfg)
        if on and kind:
            raise ValueError(f"secagg does not combine with aggregator={cfg.aggregator!r}: the robust rules need the "
                             "individual models, secure aggregation opens only their sum")
        self.secagg = on if self.world > 1 else 0
        if self.secagg and self.world > MAX_SECAGG_CLIENTS:
            raise ValueError(f"secagg takes at most {MAX_SECAGG_CLIENTS} clients (the width of the sampled-client "
                             f"mask), got {self.world}")
        # Byzantine attack model: index in ATTACKS, 0 = off; one client: off.  attack_stage: the attack is a
        # stage over the clients' contributions (every kind but "label_flip", which poisons the shard instead)
        self.attack = attack_id(cfg, self.world)
        self.attack_stage = ATTACKS[self.attack] in DEVICE_ATTACKS
        if self.attack:
            if self.world > MAX_ATTACK_CLIENTS:
                raise ValueError(f"attack={cfg.attack!r} takes at most {MAX_ATTACK_CLIENTS} clients "
                                 f"(the width of the sampled-client mask), got {self.world}")
            self.attack_par = attack_params(cfg, self.world)
            self.attack_bad = attack_clients(cfg)
        if self.attack_stage and not getattr(comm, "in_process", False):
            # a rank of its own: the stage needs every client's contribution on this rank -- the host gather
            if self.secagg:
                raise ValueError(f"attack={cfg.attack!r} does not run with multi-rank secagg: a rank only ever holds "
                                 "its peers' masked contributions; use ClientGroup")
            if not self.robust:
                raise ValueError(f"attack={cfg.attack!r} does not run on a multi-rank engine with the plain mean: the "
                                 "weighted all-reduce never holds the individual contributions; use a robust rule, "
                                 "a screen, or ClientGroup")
        if self.attack_stage and client_sizes is not None:
            self._client_sizes = [int(n) for n in client_sizes]
        self.n_local = int(len(X))
        if self.n_local == 0:
            raise ValueError("client shard is empty (reference SURVEY Q12 would deadlock)")
        self.dims = [int(X.shape[1]), *[int(h) for h in cfg.hidden], int(n_classes)]
        self.n_classes = int(n_classes)
        self.P = param_count(self.dims)
        if n_total is None:
            n_total = self._allreduce_scalar(float(self.n_local))
        self.n_total = int(n_total)
        # robust aggregators are unweighted: the contribution image IS the local model (x 1.0f is exact)
        self.agg_scale = 1.0 if self.robust else float(self.n_local) / float(self.n_total)
        self.tail_stride = self.n_classes * self.n_classes + 1
        self.hist = _History(cfg.max_rounds, self.world, dp=self.dp, compress=bool(self.compress),
                             secagg=bool(self.secagg), screen=bool(self.screen))
        self.compress_k = compress_k(cfg, self.P)   # entries a contribution transmits (sign, dense: P)
        self.heldout = False     # set_heldout: the global model is scored on a held-out set every round
        self.keep_best = False   # ... and the model of the round with the smallest held-out loss is kept
        assert init_flat.shape == (self.P,)
        if self.dp:
            if self.world > 1 and client_sizes is None:
                if not hasattr(comm, "allgather"):
                    raise ValueError("differential privacy needs client_sizes (the noise scale follows max_j n_j / N)")
                client_sizes = comm.allgather(self.n_local)
            self._client_sizes = None if client_sizes is None else [int(n) for n in client_sizes]
            self.dp_seed = (int.from_bytes(os.urandom(8), "little") if cfg.dp_seed is None
                            else int(cfg.dp_seed))
            self.dp_sigma = self._dp_sigma_table(client_sizes)
        if self.secagg:
            if float(cfg.participation) < 1.0 and client_sizes is None:
                if not hasattr(comm, "allgather"):
                    raise ValueError("secagg with client sampling needs client_sizes (the contribution is weighted "
                                     "by n_i / the sampled clients' total before it is masked)")
                client_sizes = comm.allgather(self.n_local)
            if client_sizes is not None:
                self._client_sizes = [int(n) for n in client_sizes]
            # the group's mask seed: configured, or rank 0's draw over the control plane (ClientGroup
            # draws one for its clients).  Config only, never state: no result depends on it.
            if cfg.secagg_seed is not None:
                self.secagg_seed = int(cfg.secagg_seed)
            elif hasattr(comm, "bcast"):
                self.secagg_seed = int(comm.bcast(int.from_bytes(os.urandom(8), "little"), 0))
            else:
                raise ValueError("secagg_seed=None needs a communicator that can broadcast rank 0's draw; "
                                 "name one seed for the group (ClientGroup draws it itself)")

    def fedavg_weight(self, r: int) -> float:
        """This client's FedAvg weight in round ``r`` as the per-round device table holds it: n_i / N, with
        client sampling n_i / (the sampled clients' total), 0 when it is not sampled."""
        part = self.participants(r)
        if self.rank not in part:
            return 0.0
        if len(part) == self.world:
            return float(self.n_local) / float(self.n_total)
        return float(self.n_local) / float(sum(int(self._client_sizes[k]) for k in part))

    def attack_weights(self) -> Optional[np.ndarray]:
        """The [max_rounds, world] fp32 table of every client's FedAvg weight in its buffer, as the clients'
        per-round device tables hold them (0: not sampled), for the attack stage; None in unweighted (robust)
        mode, where every weight is 1."""
        if self.robust:
            return None
        sizes = getattr(self, "_client_sizes", None)
        if sizes is None:
            raise ValueError(f"attack={self.cfg.attack!r} under the weighted mean needs client_sizes (the contributions "
                             "carry the weights n_j / N)")
        mr = max(1, int(self.cfg.max_rounds))
        tab = np.zeros((mr, self.world), np.float32)
        for r in range(mr):
            part = [int(k) for k in self.participants(r)]
            denom = float(self.n_total) if len(part) == self.world else float(sum(int(sizes[k]) for k in part))
            for k in part:
                tab[r, k] = float(sizes[k]) / denom
        return tab

    def _dp_sigma_table(self, client_sizes) -> np.ndarray:
        """Per-round noise std of ONE client's share, sigma_r = z * S * max_{j in P_r} w_j(r) / sqrt(K_r),
        with the round's FedAvg weights as ``_round_tables`` builds them; computed in double, rounded
        to fp32 once (both engines use these fp32 values)."""
        cfg = self.cfg
        mr = max(1, int(cfg.max_rounds))
        z, S = float(cfg.dp_noise), float(cfg.dp_clip)
        sigma = np.zeros(mr, np.float32)
        for r in range(mr):
            part = self.participants(r)
            if self.world == 1:
                wmax = float(self.n_local) / float(self.n_total)
            else:
                denom = float(self.n_total) if len(part) == self.world else \
                    float(sum(int(client_sizes[k]) for k in part))
                wmax = max(int(client_sizes[k]) for k in part) / denom
            sigma[r] = z * S * wmax / math.sqrt(len(part))
        return sigma

    def participants(self, r: int) -> np.ndarray:
        """Ranks that train and are averaged in round r (all of them unless sampling): the same
        seeded draw on every rank, so no broadcast is needed."""
        frac = float(self.cfg.participation)
        if frac >= 1.0 or self.world == 1:
            return np.arange(self.world)
        k = self.sampled_count()
        rng = np.random.default_rng([int(self.cfg.seed), int(r)])
        return np.sort(rng.choice(self.world, size=k, replace=False))

    def sampled_count(self) -> int:
        """Clients sampled in every round (:meth:`participants` draws that many each time)."""
        frac = float(self.cfg.participation)
        return self.world if frac >= 1.0 or self.world == 1 else max(1, int(round(frac * self.world)))

    def own_steps(self, rounds: int) -> int:
        """Adam steps this client took in rounds [0, rounds) (it only steps when sampled)."""
        if float(self.cfg.participation) >= 1.0 or self.world == 1:
            return rounds * int(self.cfg.local_steps)
        return sum(int(self.rank in self.participants(r)) for r in range(rounds)) * int(self.cfg.local_steps)

    def set_early_stop(self, patience: int, tolerance: float) -> None:
        """Early-stop parameters of ``train_and_evaluate(termination_patience, tolerance)``
        (C:122); only before the first round."""
        if getattr(self, "rounds_issued", 0):
            raise RuntimeError("early-stop parameters must be set before the first round")
        self.cfg.patience = int(patience)
        self.cfg.tolerance = float(tolerance)
        self._apply_early_stop()

    def _apply_early_stop(self) -> None:
        raise NotImplementedError

    # -- held-out scoring of the global model, inference --
    def set_heldout(self, X, y, keep_best: bool = False) -> None:
        """Score the round's GLOBAL (aggregated, post-server-step) model on the held-out rows ``(X, y)``
        at the end of every live round: ``history()`` gains ``heldout_cm`` ``[rounds_run, C, C]`` (int64),
        ``heldout_loss`` ``[rounds_run]`` (mean softmax cross-entropy: the fp32 sum / n in float64; the
        sums themselves under ``heldout_loss_sum``) and ``heldout_best_round`` (first round with the
        smallest loss sum under a plain ``<``: NaN never wins, ties keep the earlier round; -1: none).
        ``keep_best``: that round's model is kept (:meth:`best_flat`).  Call it before the first round or
        between ``run()`` calls (rounds run before it have all-zero rows).  The local metrics, the
        early-stop rule and every weight are untouched.  The data is not config: it is not saved, a
        resumed engine is given its set again before the state is loaded."""
        raise NotImplementedError

    def _check_heldout(self, X, y):
        X = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
        y = np.asarray(y)
        if X.ndim != 2 or X.shape[1] != self.dims[0]:
            raise ValueError(f"held-out X must be [n, {self.dims[0]}], got {tuple(X.shape)}")
        n = int(X.shape[0])
        if y.shape != (n,):
            raise ValueError(f"held-out y must be [{n}], got {tuple(y.shape)}")
        if not 1 <= n <= HELDOUT_MAX_ROWS:
            raise ValueError(f"held-out set: 1 .. {HELDOUT_MAX_ROWS} rows, got {n}")
        if not np.issubdtype(y.dtype, np.integer):
            raise ValueError(f"held-out labels must be integers, got dtype {y.dtype}")
        if int(y.min()) < 0 or int(y.max()) >= self.n_classes:
            raise ValueError(f"held-out labels must be in [0, {self.n_classes}), got [{int(y.min())}, {int(y.max())}]")
        return X, y.astype(np.int64)

    def _check_rows(self, X) -> np.ndarray:
        X = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
        if X.ndim != 2 or X.shape[1] != self.dims[0]:
            raise ValueError(f"X must be [n, {self.dims[0]}], got {tuple(X.shape)}")
        return X

    def heldout_step(self, r: int) -> None:
        """Held-out row of round ``r`` on the aggregated image a caller produced (host gather,
        :class:`~fedmi.fl.simulate.ClientGroup`), after :meth:`server_step`; nothing without a set."""
        raise NotImplementedError

    def best_flat(self) -> np.ndarray:
        """Dense weights of the round with the smallest held-out loss (``set_heldout(keep_best=True)``)."""
        raise NotImplementedError

    def predict_proba(self, X, which: str = "global") -> np.ndarray:
        """``[n, C]`` float32 softmax probabilities of the global (``which="global"``) or this client's
        local (``"local"``) model, or of the best held-out round's (``"best"``, with
        ``set_heldout(keep_best=True)``), from its fp32 weights."""
        raise NotImplementedError

    def predict(self, X, which: str = "global") -> np.ndarray:
        """``[n]`` int64 classes: the first-maximum argmax of the LOGITS, the confusion kernels' rule."""
        raise NotImplementedError

    def _heldout_state_out(self, best_flat) -> dict:
        """The held-out part of a portable state (the rows travel in the history)."""
        if not self.heldout:
            return {}
        return {"heldout": {"best_round": int(self.hist.ho_best_round), "best_loss_sum": float(self._ho_best_sum()),
                            "best_flat": best_flat}}

    def _heldout_state_in(self, st: dict):
        """The held-out part of a portable state for this engine, or None without held-out scoring; a
        state and an engine that disagree on having rows do not match."""
        has = st.get("heldout") is not None
        if has != bool(self.heldout):
            raise ValueError("checkpoint and engine disagree on held-out scoring: the state "
                             + ("carries" if has else "has no") + " held-out rows, the engine "
                             + ("scores a held-out set" if self.heldout else "has none (set_heldout)"))
        return st["heldout"] if has else None

    def _allreduce_scalar(self, x: float) -> float:
        if self.world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64)
        import torch.distributed as dist
        dist.all_reduce(t)
        return float(t.item())

    # subclass API
    def run(self, n_rounds: int) -> int:
        raise NotImplementedError

    def global_flat(self) -> np.ndarray:
        raise NotImplementedError

    def local_flat(self) -> np.ndarray:
        raise NotImplementedError

    def get_weights(self) -> Dict[str, np.ndarray]:
        return flat_to_dict(self.local_flat(), self.dims)

    def history(self) -> dict:
        return self.hist.as_dict()

    # -- resume (round index, Adam m/v, StepLR counter, early-stop state) --
    def portable_state(self) -> dict:
        """Engine-independent resume state (dense reference layout, numpy only).  A state
        written by one backend loads into the other."""
        raise NotImplementedError

    def load_portable_state(self, st: dict) -> None:
        raise NotImplementedError

    def _load_history(self, h: dict) -> None:
        n = int(h.get("rounds_run", 0))
        self.hist.rounds_run = n
        if n:
            self.hist.glob[:n] = np.asarray(h["global"], dtype=np.float64).reshape(n, 4)
            self.hist.rank[:n] = np.asarray(h["per_rank"], dtype=np.float64).reshape(n, self.world, 4)
            self.hist.loss[:n] = np.asarray(h["loss"], dtype=np.float32).reshape(n)
        self.hist.stop_round = int(h.get("stop_round", -1))
        self.hist.stop_trigger = int(h.get("stop_trigger", -1))
        if self.hist.norm is not None and n and "update_norm" in h:
            self.hist.norm[:n] = np.asarray(h["update_norm"], dtype=np.float32).reshape(n)
        if self.hist.cstat is not None and n and "compress_stat" in h:
            self.hist.cstat[:n] = np.asarray(h["compress_stat"], dtype=np.float32).reshape(n)
        if self.hist.clamped is not None and n and "secagg_clamped" in h:
            self.hist.clamped[:n] = np.asarray(h["secagg_clamped"], dtype=np.int64).reshape(n)
        if self.hist.screen is not None and n and "screen_kept" in h:
            self.hist.screen[:n] = np.asarray(h["screen_kept"], dtype=np.uint64).reshape(n)
        if self.hist.ho_cm is not None:
            C = self.n_classes
            if n and "heldout_cm" in h:
                self.hist.ho_cm[:n] = np.asarray(h["heldout_cm"], dtype=np.int64).reshape(n, C, C)
                self.hist.ho_loss[:n] = np.asarray(h["heldout_loss_sum"], dtype=np.float32).reshape(n)
            self.hist.ho_best_round = int(h.get("heldout_best_round", -1))

    def _load_dp_seed(self, st: dict) -> None:
        """A resumed DP engine continues the checkpoint's noise stream (a private seed drawn at
        construction is replaced by the saved one)."""
        if self.dp and st.get("dp_seed") is not None:
            self._set_dp_seed(int(st["dp_seed"]))

    def _set_dp_seed(self, seed: int) -> None:
        self.dp_seed = int(seed)

    def _load_compress_seed(self, st: dict) -> None:
        """A resumed engine with a stochastic compressor continues the checkpoint's stream (a private
        seed drawn at construction is replaced by the saved one)."""
        if self.compress_random and st.get("compress_seed") is not None:
            self._set_compress_seed(int(st["compress_seed"]))

    def _set_compress_seed(self, seed: int) -> None:
        self.compress_seed = int(seed)

    def _compress_state_out(self, residual) -> dict:
        """The compression entries of a portable state: the dense residual and, stochastic kinds, the seed."""
        if not self.compress:
            return {}
        return {"compress_residual": residual,
                **({"compress_seed": int(self.compress_seed)} if self.compress_random else {})}

    def uplink_bytes(self) -> int:
        """Bytes per round a real uplink would carry for this client's contribution (the exchange
        itself stays dense: compression is simulated)."""
        return uplink_bytes(self.cfg.compress, self.compress_k, self.P, int(self.cfg.compress_levels))

    def _compress_state_in(self, st: dict):
        """The dense compression residual of a portable state for this engine, or None without
        compression; a state and an engine that disagree on having one do not match."""
        has = st.get("compress_residual") is not None
        if has != bool(self.compress):
            raise ValueError("checkpoint and engine disagree on compression: the state "
                             + ("carries" if has else "has no") + " compress_residual, the engine has compress="
                             + repr(self.cfg.compress))
        if not self.compress:
            return None
        if (st.get("compress_seed") is not None) != self.compress_random:
            raise ValueError("checkpoint and engine disagree on compression: the state "
                             + ("carries" if not self.compress_random else "has no")
                             + " compress_seed, the engine has compress=" + repr(self.cfg.compress))
        e = np.asarray(st["compress_residual"], np.float32).reshape(-1)
        if e.shape != (self.P,):
            raise ValueError(f"compression residual has {e.shape[0]} entries, the model {self.P}")
        return e

    def _server_state_in(self, st: dict):
        """The dense (server_m, server_v) of a portable state for this engine, or None without a
        server optimizer; a state and an engine that disagree on having one do not match."""
        has = st.get("server_m") is not None
        if has != bool(self.server):
            raise ValueError("checkpoint and engine disagree on the server optimizer: the state "
                             + ("carries" if has else "has no") + " server_m / server_v, the engine has server_opt="
                             + repr(self.cfg.server_opt))
        if not self.server:
            return None
        m = np.asarray(st["server_m"], np.float32).reshape(-1)
        v = np.asarray(st["server_v"], np.float32).reshape(-1)
        if m.shape != (self.P,) or v.shape != (self.P,):
            raise ValueError(f"server optimizer state has {m.shape[0]} / {v.shape[0]} entries, the model {self.P}")
        return m, v


# ---------------------------------------------------------------------------------------
# Torch (CPU / oracle) engine
# ---------------------------------------------------------------------------------------
class TorchRoundEngine(RoundEngineBase):
    def __init__(self, X, y, n_classes, cfg: EngineConfig, comm, init_flat, n_total=None,
                 device="cpu", X_dtype=torch.float32, client_sizes=None):
        super().__init__(X, y, n_classes, cfg, comm, init_flat, n_total, client_sizes)
        self.device = torch.device(device)
        self.X = torch.as_tensor(np.asarray(X), dtype=X_dtype, device=self.device)
        self.y = torch.as_tensor(np.asarray(y), dtype=torch.long, device=self.device)
        self.model = MLPModel(self.dims[0], self.dims[1:-1], self.dims[-1], device=self.device)
        with torch.no_grad():
            self.model.flat.copy_(torch.as_tensor(init_flat))
        self.criterion = torch.nn.CrossEntropyLoss()
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=cfg.lr, betas=tuple(cfg.betas),
                                          eps=cfg.eps, weight_decay=cfg.weight_decay)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=cfg.step_size,
                                                         gamma=cfg.gamma)
        self.stopper = EarlyStopper(cfg.patience, cfg.tolerance, cfg.rtol, enabled=cfg.early_stop)
        self.global_params = self.model.flat.detach().clone()
        self.rounds_issued = 0
        if self.server:
            # server optimizer state in dense named_parameters() order (v starts at tau^2)
            self.server_m = torch.zeros(self.P, dtype=torch.float32)
            self.server_v = torch.full((self.P,), float(np.float32(cfg.server_tau)) ** 2, dtype=torch.float32)
        if self.compress:
            self.compress_residual = torch.zeros(self.P, dtype=torch.float32)   # dense order
            self._compressed = (-1, None)   # (round, x + C(u)) of the last compressed round

    def train_one_epoch(self) -> float:
        """``local_steps`` full-batch Adam steps + one StepLR step (reference C:63-73)."""
        self.model.train()
        anchor = self.model.flat.detach().clone() if self.cfg.prox_mu else None
        loss_v = 0.0
        for _ in range(self.cfg.local_steps):
            self.optimizer.zero_grad()
            out = self.model(self.X)
            loss = self.criterion(out, self.y)
            loss.backward()
            if anchor is not None:
                with torch.no_grad():
                    for (name, shape, off), p in zip(self.model.layout, self.model.parameters()):
                        n = int(np.prod(shape))
                        p.grad.add_(self.cfg.prox_mu * (p.detach() - anchor[off:off + n].view(shape)))
            self.optimizer.step()
            loss_v = float(loss.detach())
        self._scheduler_step()
        return loss_v

    def _scheduler_step(self) -> None:
        """StepLR follows the global round index (C:73 steps it once per round) for every
        client, sampled or not; only a sampled client's Adam takes a step."""
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)  # "scheduler.step() before optimizer.step()"
            self.scheduler.step()

    def confusion(self, X=None, y=None, flat=None) -> np.ndarray:
        Xt = self.X if X is None else torch.as_tensor(np.asarray(X), dtype=torch.float32, device=self.device)
        yt = self.y if y is None else torch.as_tensor(np.asarray(y), dtype=torch.long, device=self.device)
        model = self.model
        if flat is not None:
            model = MLPModel(self.dims[0], self.dims[1:-1], self.dims[-1], device=self.device)
            with torch.no_grad():
                model.flat.copy_(torch.as_tensor(flat))
        model.eval()
        with torch.no_grad():
            _, pred = torch.max(model(Xt), 1)
        return confusion_matrix(yt.cpu().numpy(), pred.cpu().numpy(), self.n_classes)

    def _apply_early_stop(self) -> None:
        cfg = self.cfg
        self.stopper = EarlyStopper(cfg.patience, cfg.tolerance, cfg.rtol, enabled=cfg.early_stop)

    # -- held-out scoring (the HIP engine's definitions in torch fp32: its own oracle, not bit-equal) --
    def set_heldout(self, X, y, keep_best: bool = False) -> None:
        X, y = self._check_heldout(X, y)
        self.ho_X = torch.as_tensor(X, device=self.device)
        self.ho_y = torch.as_tensor(y, dtype=torch.long, device=self.device)
        self.hist.enable_heldout(self.n_classes, len(X))
        if not self.heldout:
            self._ho_best = np.float32(np.inf)
            self._ho_best_flat = None
        self.heldout, self.keep_best = True, bool(keep_best)

    def _ho_best_sum(self) -> float:
        return float(self._ho_best)

    def heldout_step(self, r: int) -> None:
        if not self.heldout:
            return
        self.model.eval()
        with torch.no_grad():
            z = self.model(self.ho_X).to(torch.float32)
            _, pred = torch.max(z, 1)
            loss = np.float32(_softmax_ce_rows(z, self.ho_y).sum().item())
        self.hist.ho_cm[r] = confusion_matrix(self.ho_y.cpu().numpy(), pred.cpu().numpy(), self.n_classes)
        self.hist.ho_loss[r] = loss
        if loss < self._ho_best:    # plain <: NaN never wins, ties keep the earlier round
            self._ho_best = loss
            self.hist.ho_best_round = int(r)
            if self.keep_best:
                self._ho_best_flat = self.model.flat.detach().cpu().numpy().copy()

    def best_flat(self) -> np.ndarray:
        if not (self.heldout and self.keep_best):
            raise RuntimeError("best_flat: needs set_heldout(X, y, keep_best=True)")
        if self._ho_best_flat is None:
            raise RuntimeError("best_flat: no round has won yet")
        return self._ho_best_flat.copy()

    def _logits(self, X, which: str) -> torch.Tensor:
        if which not in ("global", "local", "best"):
            raise ValueError(f"which must be 'global', 'local' or 'best', got {which!r}")
        Xt = torch.as_tensor(self._check_rows(X), device=self.device)
        model = self.model
        if which != "local":
            model = MLPModel(self.dims[0], self.dims[1:-1], self.dims[-1], device=self.device)
            with torch.no_grad():
                model.flat.copy_(self.global_params if which == "global" else torch.as_tensor(self.best_flat()))
        model.eval()
        with torch.no_grad():
            return model(Xt).to(torch.float32)

    def predict_proba(self, X, which: str = "global") -> np.ndarray:
        return torch.softmax(self._logits(X, which), 1).cpu().numpy().astype(np.float32).reshape(-1, self.n_classes)

    def predict(self, X, which: str = "global") -> np.ndarray:
        z = self._logits(X, which)
        if z.shape[0] == 0:
            return np.zeros(0, np.int64)
        return torch.max(z, 1)[1].cpu().numpy().astype(np.int64)

    # -- step-by-step API (reference train_one_epoch / evaluate_local / federated_averaging)
    def step_train(self) -> None:
        r = self.rounds_issued
        self._active = self.rank in self.participants(r)
        if self.dp or self.compress or self.attack_stage:
            self._dp_input = self.model.flat.detach().cpu().clone()   # the image the round trains from
        if self._active:
            self._loss = self.train_one_epoch()
        else:
            self._loss = 0.0
            self._scheduler_step()

    def step_eval(self) -> np.ndarray:
        self._cm = self.confusion()
        return self._cm

    def fedavg_contribution(self) -> torch.Tensor:
        """This client's operand of the round's SUM all-reduce:
        [w * n_i/N | per-rank (confusion, loss) tails] (+ n_i when sampling clients)."""
        if self.robust:
            return self._robust_contribution()
        if self.secagg:
            return self._secagg_contribution()
        sampling = float(self.cfg.participation) < 1.0 and self.world > 1
        buf = torch.zeros(self.P + self.world * self.tail_stride + int(sampling), dtype=torch.float32)
        active = getattr(self, "_active", True)
        model = self.model.flat.detach().cpu()
        noise = None
        if self.dp:
            # DP-FedAvg: the clipped model x + c (local - x) takes the local model's place, and the
            # client's share of the round's Gaussian noise (the device's Philox stream) is added
            r = self.rounds_issued
            self.hist.norm[r] = 0.0
            if active:
                model, noise = self._dp_clip_and_noise(r, model)
        if self.compress:
            model = self._compressed_model(model, active)
        if not sampling:
            buf[:self.P] = model * self.agg_scale
            if noise is not None:
                buf[:self.P] += noise
        elif active:
            # weights n_i * w_i and, in the last slot, n_i: divided by the sampled total after the sum
            buf[:self.P] = model * float(self.n_local)
            if noise is not None:
                buf[:self.P] += noise * float(sum(self._client_sizes[k] for k in self.participants(r)))
            buf[-1] = float(self.n_local)
        t0 = self.P + self.rank * self.tail_stride
        buf[t0:t0 + self.n_classes ** 2] = torch.as_tensor(self._cm.reshape(-1), dtype=torch.float32)
        buf[t0 + self.n_classes ** 2] = self._loss
        return buf

    def attack_rows(self, bufs: Sequence[torch.Tensor]) -> None:
        """The attack stage over the clients' :meth:`fedavg_contribution` rows (rank order), in place, in the
        rows' dtype (``attack_torch``), with the weights those rows carry: 1 in robust mode, the fp32 table
        weight under secure aggregation, ``n_j / N`` under the mean and ``n_j`` under the mean with client
        sampling (divided by the sampled total after the sum).  Nothing without a launched attack kind."""
        if not self.attack_stage:
            return
        r = self.rounds_issued
        part = [int(k) for k in self.participants(r)]
        if self.robust:
            w = None
        elif self.secagg:
            if getattr(self, "_attack_wtab", None) is None:
                self._attack_wtab = self.attack_weights()
            w = [float(v) for v in self._attack_wtab[r]]
        elif float(self.cfg.participation) < 1.0:
            w = [float(n) for n in self._client_sizes]
        else:
            w = [float(n) / float(self.n_total) for n in self._client_sizes]
        par = self.attack_par
        attack_torch(bufs, self._dp_input, [k in part for k in range(self.world)], self.attack_bad, par["kind"],
                     par["scale"], par["z"], self.P, weights=w, seed=int(self.cfg.attack_seed), round=r)

    def _dp_clip_and_noise(self, r: int, local: torch.Tensor):
        """(x + c (local - x), this client's noise vector or None) of round r; records the pre-clip
        norm.  An unclipped round keeps the local model as it is (c = 1)."""
        from ..privacy.philox import dp_normals
        x = self._dp_input.to(local.dtype)
        delta = local - x
        norm = float(torch.linalg.vector_norm(delta.double()))
        self.hist.norm[r] = norm
        S = float(self.cfg.dp_clip)
        if norm > S:
            local = x + delta * (S / norm)
        if float(self.cfg.dp_noise) == 0.0:
            return local, None
        xi = float(self.dp_sigma[r]) * dp_normals(self.P, r, self.rank, self.dp_seed)
        return local, torch.as_tensor(xi).to(local.dtype)

    def _compressed_model(self, local: torch.Tensor, active: bool) -> torch.Tensor:
        """x + C((local - x) + e) of the round being issued, in fp32 (fedmi/fl/compress.py); updates the
        residual and records the round's statistic once per round.  An unsampled client keeps both."""
        r = self.rounds_issued
        if self._compressed[0] == r:
            return self._compressed[1]
        self.hist.cstat[r] = 0.0
        out = local
        if active:
            x = self._dp_input.to(torch.float32)
            u = (local.to(torch.float32) - x) + self.compress_residual
            rnd = (dict(levels=int(self.cfg.compress_levels), seed=self.compress_seed, round=r, client=self.rank)
                   if self.compress_random else {})
            c, self.compress_residual, stat = compress_torch(u, self.cfg.compress, self.compress_k,
                                                             bool(self.cfg.error_feedback), **rnd)
            self.hist.cstat[r] = stat
            out = x + c
        self._compressed = (r, out)
        return out

    def _secagg_contribution(self) -> torch.Tensor:
        """Secure aggregation: this client's clear row in the HIP engines' weighted form,
        [w_i(r) * model (+ noise) (zeros when not sampled) | per-rank (confusion, loss) tails] with the
        per-round table's fp32 weight -- no trailing n_i slot and no division after the sum, so both
        backends quantise the same quantity.  :meth:`secagg_mask_` masks it in place."""
        r = self.rounds_issued
        buf = torch.zeros(self.P + self.world * self.tail_stride, dtype=torch.float32)
        active = getattr(self, "_active", True)
        model = self.model.flat.detach().cpu()
        noise = None
        if self.dp:
            self.hist.norm[r] = 0.0
            if active:
                model, noise = self._dp_clip_and_noise(r, model)
        if self.compress:
            model = self._compressed_model(model, active)
        if active:
            buf[:self.P] = model.to(torch.float32) * torch.tensor(self.fedavg_weight(r), dtype=torch.float32)
            if noise is not None:
                buf[:self.P] += noise.to(torch.float32)
        t0 = self.P + self.rank * self.tail_stride
        buf[t0:t0 + self.n_classes ** 2] = torch.as_tensor(self._cm.reshape(-1), dtype=torch.float32)
        buf[t0 + self.n_classes ** 2] = self._loss
        return buf

    def secagg_mask_(self, buf: torch.Tensor) -> torch.Tensor:
        """Quantise and pair-mask the parameters of this client's contribution row in place (the host
        model, fedmi/fl/secagg.py): the words' bit patterns take the floats' places.  An unsampled
        client's row is left alone.  Records the round's clamp count."""
        r = self.rounds_issued
        part = [int(k) for k in self.participants(r)]
        self.hist.clamped[r] = 0
        if self.rank in part:
            q, self.hist.clamped[r] = secagg_quantize(buf[:self.P].numpy(), int(self.cfg.secagg_bits), len(part))
            y = secagg_mask(q, self.rank, part, r, self.secagg_seed)
            buf[:self.P].view(torch.int32).copy_(torch.as_tensor(y.view(np.int32)))
        return buf

    def secagg_combine(self, bufs: Sequence[torch.Tensor]) -> torch.Tensor:
        """The clients' masked rows (rank order) -> [opened sum of the sampled clients' words | tails
        summed in rank order], the buffer :meth:`fedavg_apply` adopts."""
        part = [int(k) for k in self.participants(self.rounds_issued)]
        out = bufs[0].clone()
        for b in bufs[1:]:
            out[self.P:] += b[self.P:]
        ys = np.stack([bufs[k][:self.P].contiguous().view(torch.int32).numpy().view(np.uint32) for k in part])
        out[:self.P] = torch.as_tensor(secagg_open(ys, int(self.cfg.secagg_bits)))
        return out

    def _robust_contribution(self) -> torch.Tensor:
        """Robust aggregators: this client's row of the round's gather, [unscaled local model (zeros
        when not sampled) | per-rank (confusion, loss) tails | 1 when sampled, else 0]."""
        buf = torch.zeros(self.P + self.world * self.tail_stride + 1, dtype=torch.float32)
        active = getattr(self, "_active", True)
        model = self.model.flat.detach().cpu()
        if self.compress:
            model = self._compressed_model(model, active)
        if active:
            buf[:self.P] = model
            buf[-1] = 1.0
        t0 = self.P + self.rank * self.tail_stride
        buf[t0:t0 + self.n_classes ** 2] = torch.as_tensor(self._cm.reshape(-1), dtype=torch.float32)
        buf[t0 + self.n_classes ** 2] = self._loss
        return buf

    def robust_combine(self, bufs: Sequence[torch.Tensor]) -> torch.Tensor:
        """The clients' :meth:`fedavg_contribution` rows (rank order) -> [robust aggregate of the sampled
        clients' images | tails summed in rank order], the buffer :meth:`fedavg_apply` adopts."""
        stack = torch.stack([b[:self.P] for b in bufs])
        out = bufs[0][:-1].clone()
        for b in bufs[1:]:
            out += b[:-1]
        active = [float(b[-1]) != 0.0 for b in bufs]
        if self.screen:
            # multi-Krum: the rule runs over the clients the screen keeps (fp32 distances in torch's order)
            active = screen_select(pair_distances_torch(stack, active), active, int(self.cfg.screen_byzantine),
                                   self.cfg.screen_keep)
            self.hist.screen[self.rounds_issued] = mask_bits(active)
        if ALL_AGGREGATORS[self.robust] == "geomed":
            out[:self.P] = geomed_torch(stack, active, int(self.cfg.geomed_iters), float(self.cfg.geomed_nu))
        else:
            out[:self.P] = robust_aggregate_torch(stack, active, AGGREGATORS[self.robust], self.robust_beta)
        return out

    def step_aggregate(self) -> None:
        # one SUM all-reduce of [w * n_i/N | per-rank (confusion, loss) tails]
        buf = self.fedavg_contribution()
        if self.robust:
            # robust aggregators: every client's row is gathered, the rule applied on every rank alike
            rows = [torch.as_tensor(b) for b in self.comm.allgather(buf.numpy())]
            self.attack_rows(rows)   # (Byzantine attack model: every rank rewrites its copy of the bad ranks' rows)
            buf = self.robust_combine(rows)
        elif self.secagg:
            # secure aggregation: every client's MASKED row is gathered, the sum opened on every rank alike
            self.secagg_mask_(buf)
            buf = self.secagg_combine([torch.as_tensor(b) for b in self.comm.allgather(buf.numpy())])
        elif self.comm is not None:
            self.comm.allreduce_(buf)
        self.fedavg_apply(buf)

    def fedavg_apply(self, buf: torch.Tensor) -> None:
        """Adopt the all-reduced buffer: new global weights, metrics, early-stop rule."""
        r = self.rounds_issued
        sampling = float(self.cfg.participation) < 1.0 and self.world > 1 and not self.robust and not self.secagg
        if sampling:
            buf[:self.P] /= buf[-1]
            buf = buf[:-1]
        new = buf[:self.P]
        if self.server:
            # the aggregated image is a pseudo-gradient step from the image the round trained from
            new = server_step(self.server, self.cfg, self.global_params.detach().cpu().to(torch.float32),
                              new.to(torch.float32), self.server_m, self.server_v)
        with torch.no_grad():
            self.model.flat.copy_(new.to(self.device))
        self.global_params = self.model.flat.detach().clone()
        self.heldout_step(r)
        self._finalize(r, buf[self.P:].numpy())
        self.rounds_issued += 1

    def run(self, n_rounds: int) -> int:
        ran = 0
        for _ in range(n_rounds):
            if self.stopper.stopped or self.rounds_issued >= self.cfg.max_rounds:
                break
            self.step_train()
            self.step_eval()
            self.step_aggregate()
            ran += 1
        return ran

    def sync_history(self) -> None:
        pass

    def run_streaming(self, n_rounds: int, chunk: int = 16, on_history=None, guard=None) -> int:
        """:meth:`run` round by round, ``on_history`` after every round (host-driven rounds: each
        round's metrics are on the host as soon as it ends)."""
        import contextlib
        ran = 0
        for _ in range(int(n_rounds)):
            if self.stopper.stopped or self.rounds_issued >= self.cfg.max_rounds:
                break
            with (guard(f"round {self.rounds_issued}") if guard else contextlib.nullcontext()):
                ran += self.run(1)
            if on_history is not None:
                on_history(self.history())
        return ran

    @property
    def stopped(self) -> bool:
        return self.stopper.stopped

    def _finalize(self, r: int, tail: np.ndarray) -> None:
        if self.cfg.debug:
            _check_finite(r, "aggregated weights", self.model.flat.detach())
            _check_finite(r, "loss/confusion tail", torch.as_tensor(tail))
        tails = tail.reshape(self.world, self.tail_stride)
        C = self.n_classes
        per = [metrics_from_confusion(t[:C * C].reshape(C, C)) for t in tails]
        # global metrics / loss: the round's sampled clients (every client without sampling);
        # per-client metrics are recorded for all (an unsampled client scores the global model)
        part = self.participants(r)
        if self.cfg.metric_mode == "mean":
            g = metric_vector({k: float(np.mean([per[i][k] for i in part])) for k in METRIC_NAMES})
        else:
            g = metric_vector(metrics_from_confusion(tails[part, :C * C].sum(0).reshape(C, C)))
        self.hist.glob[r] = g
        self.hist.rank[r] = np.stack([metric_vector(m) for m in per])
        self.hist.loss[r] = float(tails[part, C * C].astype(np.float64).sum() / len(part))
        self.hist.rounds_run = r + 1
        if self.stopper.update(g):
            self.hist.stop_trigger = r
            self.hist.stop_round = r + 1

    def global_flat(self) -> np.ndarray:
        return self.global_params.cpu().numpy().copy()

    def local_flat(self) -> np.ndarray:
        return self.model.flat.detach().cpu().numpy().copy()

    def set_global_flat(self, flat: np.ndarray) -> None:
        with torch.no_grad():
            self.model.flat.copy_(torch.as_tensor(flat))
        self.global_params = self.model.flat.detach().clone()

    def state_dict(self) -> dict:
        return {"params": self.global_flat(), "optimizer": self.optimizer.state_dict(),
                "scheduler": self.scheduler.state_dict(), "stopper": self.stopper.state_dict(),
                "rounds": self.rounds_issued, "history": self.hist.as_dict()}

    def portable_state(self) -> dict:
        params = list(self.model.parameters())
        m = [self.optimizer.state.get(p, {}).get("exp_avg") for p in params]
        v = [self.optimizer.state.get(p, {}).get("exp_avg_sq") for p in params]
        cat = (lambda ts: np.zeros(self.P, np.float32) if ts[0] is None else
               torch.cat([t.detach().reshape(-1).cpu() for t in ts]).numpy().astype(np.float32))
        sp = self.stopper
        st0 = self.optimizer.state.get(params[0], {}).get("step")
        return {
            "rounds": int(self.rounds_issued), "global": self.global_flat(), "local": self.local_flat(),
            "exp_avg": cat(m), "exp_avg_sq": cat(v), "opt_steps": int(st0) if st0 is not None else 0,
            "es": {"count": int(sp.count), "has_prev": sp.prev is not None,
                   "prev": [0.0] * 4 if sp.prev is None else [float(x) for x in sp.prev],
                   "stopped": bool(sp.stopped), "stop_round": int(self.hist.stop_round)},
            "history": self.hist.as_dict(),
            **({"dp_seed": int(self.dp_seed)} if self.dp else {}),
            **({"server_m": self.server_m.numpy().copy(), "server_v": self.server_v.numpy().copy()}
               if self.server else {}),
            **self._compress_state_out(self.compress_residual.numpy().copy() if self.compress else None),
            **self._heldout_state_out(None if not self.heldout or self._ho_best_flat is None
                                      else self._ho_best_flat.copy()),
        }

    def load_portable_state(self, st: dict) -> None:
        r = int(st["rounds"])
        cfg = self.cfg
        sv = self._server_state_in(st)
        ce = self._compress_state_in(st)
        ho = self._heldout_state_in(st)
        if ho is not None:
            self._ho_best = np.float32(ho["best_loss_sum"])
            self._ho_best_flat = (None if ho.get("best_flat") is None or not self.keep_best
                                  else np.asarray(ho["best_flat"], np.float32).copy())
        if sv is not None:
            self.server_m = torch.as_tensor(sv[0].copy())
            self.server_v = torch.as_tensor(sv[1].copy())
        if ce is not None:
            self.compress_residual = torch.as_tensor(ce.copy())
            self._compressed = (-1, None)
        with torch.no_grad():
            self.model.flat.copy_(torch.as_tensor(np.asarray(st["global"], np.float32)))
        self.global_params = self.model.flat.detach().clone()
        steps = int(st.get("opt_steps", self.own_steps(r)))   # this client's own Adam steps
        if steps:
            off = 0
            for p in self.model.parameters():
                n = p.numel()
                self.optimizer.state[p] = {
                    "step": torch.tensor(float(steps)),
                    "exp_avg": torch.as_tensor(np.asarray(st["exp_avg"][off:off + n], np.float32)).view_as(p).clone(),
                    "exp_avg_sq": torch.as_tensor(np.asarray(st["exp_avg_sq"][off:off + n], np.float32)).view_as(p).clone(),
                }
                off += n
        lr = cfg.lr * cfg.gamma ** (r // cfg.step_size)
        for g in self.optimizer.param_groups:
            g["lr"] = lr
        self.scheduler.last_epoch = r
        self.scheduler._step_count = r + 1
        self.scheduler._last_lr = [lr]
        es = st["es"]
        self.stopper.count = int(es["count"])
        self.stopper.prev = np.asarray(es["prev"], np.float64) if es["has_prev"] else None
        self.stopper.stopped = bool(es["stopped"])
        self.rounds_issued = r
        self._load_history(st["history"])
        self._load_dp_seed(st)
        self._load_compress_seed(st)


# ---------------------------------------------------------------------------------------
# HIP engine
# ---------------------------------------------------------------------------------------
_STATE_DTYPE = np.dtype([("next_round", "<i4"), ("finalized", "<i4"), ("stopped", "<i4"), ("live", "<i4"),
                         ("cur_round", "<i4"), ("count", "<i4"), ("has_prev", "<i4"), ("stop_round", "<i4"),
                         ("calls", "<u4"), ("late", "<i4"), ("prev", "<f8", (4,))])


class HipRoundEngine(RoundEngineBase):
    """Device-resident client.  ``X``/``y`` may be numpy arrays (uploaded once) or CUDA
    tensors already on the device (e.g. from the synthetic generator)."""

    def __init__(self, X, y, n_classes, cfg: EngineConfig, comm, init_flat, n_total=None, device=None,
                 comm_buffers=None, emulate_clients: bool = False, client_sizes=None, stream=None):
        """``stream``: the torch stream the engine issues on (default: a new one).  Engines created one
        after another in a process (bench.py's timed runs) should share one: with ranks sharing a
        GPU, a second engine on a fresh stream ran its Adam-exchange rounds 2.3x slower
        (108 vs 46 us per round, profiles/bench_r4_n2_share_stream.log).
        ``comm_buffers``: optional pair of float32 device views of length
        :meth:`comm_len` to use as the double-buffered FedAvg buffers (trial packing shares one
        all-reduce between engines by handing each a slice of one allocation).
        ``client_sizes``: every client's shard size (client sampling weighs the sampled clients
        by n_i / their sum); gathered over ``comm`` when needed and not given."""
        from ..ops import native
        if int(cfg.local_steps) > MAX_LOCAL_STEPS:
            raise ValueError(f"HipRoundEngine: at most {MAX_LOCAL_STEPS} local steps per round (got {cfg.local_steps})")
        if cfg.compress != "none" and comm_buffers is not None:
            raise ValueError(f"trial packing (comm_buffers) does not run compression (compress={cfg.compress!r})")
        if screen_id(cfg, comm.size if comm is not None else 1) and comm_buffers is not None:
            raise ValueError(f"trial packing (comm_buffers) does not run client screening (screen={cfg.screen!r})")
        if cfg.aggregator != "mean" and comm_buffers is not None:
            raise ValueError(f"trial packing (comm_buffers) does not run a robust aggregator (aggregator={cfg.aggregator!r})")
        if bool(cfg.secagg) and comm_buffers is not None:
            raise ValueError("trial packing (comm_buffers) does not run secure aggregation (secagg)")
        world = comm.size if comm is not None else 1
        if attack_stage(cfg, world) and comm_buffers is not None:
            raise ValueError(f"trial packing (comm_buffers) does not run an attack stage (attack={cfg.attack!r})")
        if attack_stage(cfg, world) and cfg.gather_plane == "xgmi":
            raise ValueError(f"attack={cfg.attack!r} does not run on gather_plane='xgmi': the one-shot select kernel never "
                             "holds the stack of contributions the stage rewrites; use gather_plane='host'")
        # robust rule / secure aggregation over the one-shot xGMI peer kernel: one node's ranks at most
        from ..parallel.peer import PEER_MAX_WORLD
        xgmi_select = (bool(gather_plane_id(cfg)) and comm is not None and int(comm.size) > 1
                       and (aggregator_id(cfg) != 0 or bool(secagg_id(cfg))))
        if xgmi_select and int(comm.size) > PEER_MAX_WORLD:
            raise ValueError(f"gather_plane='xgmi' takes at most {PEER_MAX_WORLD} ranks (the peers of one node), "
                             f"got {int(comm.size)}; use gather_plane='host'")
        self.m = native()
        self._packed = comm_buffers is not None   # an engine of a trial batch (shared FedAvg buffers)
        if device is None:
            device = comm.device if comm is not None else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if isinstance(X, torch.Tensor):
            Xn_len = X.shape[0]
            Xshape1 = X.shape[1]
        else:
            Xn_len, Xshape1 = X.shape
        super().__init__(_ShapeOnly(Xn_len, Xshape1), y, n_classes, cfg, comm, init_flat, n_total, client_sizes)
        if (self.dp or self.secagg) and client_sizes is None:
            client_sizes = getattr(self, "_client_sizes", None)
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.X = (X if isinstance(X, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(X, np.float32))).to(**f32).contiguous()
        self.y = (y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))).to(dtype=torch.int32, device=dev).contiguous()
        # rows per workgroup: 0 = auto (32 when the model's LDS image fits, else 16); -1 = the
        # largest that fits, 64 first (bf16: half the workgroups and gradient-slab rows -- what
        # packed trial batches want, whose throughput is workgroup-slots x workgroup latency)
        rpb = int(cfg.rows_per_block)
        # (auto: small shards -- the reference's 8000 // k rows at k >= 4 -- run twice the
        # workgroups at 16 rows each, lower per-workgroup latency; profiles/round_emulate_r4_shards.log)
        auto = [16, 32] if (Xn_len <= SMALL_SHARD_ROWS and cfg.dtype == "bf16") else [32, 16]
        R_try = auto if rpb == 0 else ([64, 32, 16] if cfg.dtype == "bf16" else [32, 16]) if rpb == -1 else [rpb]
        R = R_try[0]
        # device parameter buffers use the padded image layout (fl_common.h)
        self.Pimg = image_layout(self.dims)[2]
        # lagged evaluation carries a second metric region after the tails (fl_common.h)
        # (emulate_clients: one process measures the multi-client round shape, tools/round_emulate.py)
        # (with early stopping the native engine runs lagged rounds with the Adam-fused exchange,
        # which folds each round's metrics in time, or over RCCL, folded one round late with the
        # round run past a stop discarded bit-exactly: FLEngine.late_fold)
        # (differential privacy: classic rounds, see fl_engine.cpp)
        # (robust aggregators: classic rounds aggregated from Python, see _aggregate, or by the peer
        # kernel's select call, gather_plane="xgmi")
        # (compression: classic rounds, as with differential privacy)
        # (secure aggregation: classic rounds masked and opened from Python, see _aggregate, or by the
        # native engine on the peer plane, gather_plane="xgmi")
        self._lag = ((self.world > 1 or emulate_clients) and cfg.dtype == "bf16"
                     and comm_buffers is None and bool(cfg.lagged_eval) and not self.dp and not self.server
                     and not self.robust and not self.compress and not self.secagg)
        comm_len = self.Pimg + self.world * self.tail_stride * (2 if self._lag else 1)
        if comm_buffers is None:
            self.params = [torch.zeros(comm_len, **f32), torch.zeros(comm_len, **f32)]
        else:
            self.params = list(comm_buffers)
            for t in self.params:
                if t.numel() != comm_len or t.dtype != torch.float32 or t.device != dev:
                    raise ValueError("comm_buffers must be two float32 views of comm_len() on the engine device")
                t.zero_()
        self.params[0][:self.Pimg] = torch.as_tensor(dense_to_image(init_flat, self.dims))
        self.local = self.params[0][:self.Pimg].clone()
        self.mom = torch.zeros(self.Pimg, **f32)
        self.vel = torch.zeros(self.Pimg, **f32)
        sb = self.m.STATE_BYTES
        assert sb == _STATE_DTYPE.itemsize, (sb, _STATE_DTYPE.itemsize)
        init = np.zeros(1, dtype=_STATE_DTYPE)
        init["count"] = cfg.patience
        init["stop_round"] = -1
        st = torch.as_tensor(init.view(np.uint8).copy())
        self.state = [st.to(dev), st.to(dev)]
        if float(cfg.participation) < 1.0 and self.world > 1 and client_sizes is None:
            client_sizes = comm.allgather(self.n_local)
        sched, rtab = self._round_tables(client_sizes)
        self.sched = torch.as_tensor(sched, device=dev)
        self.rtab = torch.as_tensor(rtab, device=dev)
        mr = int(cfg.max_rounds)
        self.h_global = torch.zeros(mr * 4, dtype=torch.float64, device=dev)
        self.h_rank = torch.zeros(mr * self.world * 4, dtype=torch.float64, device=dev)
        self.h_loss = torch.zeros(mr, dtype=torch.float32, device=dev)
        # fp16 gradient slab guard: the Adam kernel sets it when a partial it reads is saturated at
        # +-65504 (slab_store_h's clamp) or not finite; read_history() reports it
        self.sat = torch.zeros(1, dtype=torch.int32, device=dev)
        self.slab_saturated = False
        ecfg = {
            "R": R, "n_rows": self.n_local, "world": self.world, "rank": self.rank, "agg_scale": self.agg_scale,
            "local_steps": int(cfg.local_steps), "lr": float(cfg.lr), "gamma": float(cfg.gamma),
            "step_size": int(cfg.step_size), "beta1": float(cfg.betas[0]), "beta2": float(cfg.betas[1]),
            "eps": float(cfg.eps), "weight_decay": float(cfg.weight_decay), "prox_mu": float(cfg.prox_mu),
            "early_stop": bool(cfg.early_stop), "patience": int(cfg.patience), "atol": float(cfg.tolerance),
            "rtol": float(cfg.rtol), "max_rounds": mr, "metric_mode": _metric_mode_id(cfg.metric_mode),
            "dtype": _dtype_id(cfg.dtype),
            # trial packing runs rounds through run_local + a shared all-reduce: classic rounds
            "fused_eval": bool(cfg.fused_eval) and comm_buffers is None,
            "eval_fedavg": bool(cfg.eval_fedavg),
            "lagged_eval": self._lag,
            "emulate_clients": bool(emulate_clients),
            "slab_f16": self._pick_slab_f16(cfg),
            # the native engine may keep its fp16 slab rows blocked (layout()["slab_blocked"]: the
            # reference shape's specialised train / Adam pair); engines of a trial batch keep dense rows
            "slab_blocked": comm_buffers is None,
            "plain_fwd": -1 if cfg.plain_fwd is None else int(bool(cfg.plain_fwd)),
        }
        bufs = {
            "X": self.X.data_ptr(), "y": self.y.data_ptr(),
            "local": self.local.data_ptr(), "m": self.mom.data_ptr(), "v": self.vel.data_ptr(),
            "hist_global": self.h_global.data_ptr(), "hist_rank": self.h_rank.data_ptr(),
            "hist_loss": self.h_loss.data_ptr(), "sched": self.sched.data_ptr(), "rtab": self.rtab.data_ptr(),
            "sat": self.sat.data_ptr(),
            "params0": self.params[0].data_ptr(),
            "params1": self.params[1].data_ptr(), "state0": self.state[0].data_ptr(),
            "state1": self.state[1].data_ptr(),
        }
        if self.dp:
            # per-round noise std (host table like `sched`) and this client's pre-clip update norms
            self.dp_sigma_dev = torch.as_tensor(self.dp_sigma, device=dev)
            self.dp_norm = torch.zeros(mr, dtype=torch.float32, device=dev)
            ecfg.update({"dp_clip": float(cfg.dp_clip), "dp_noise": float(cfg.dp_noise) > 0.0,
                         "dp_seed": int(self.dp_seed)})
            bufs.update({"dp_sigma": self.dp_sigma_dev.data_ptr(), "dp_norm": self.dp_norm.data_ptr()})
        if self.compress:
            # residual: two image-shaped fp32 halves, round r reads half r & 1 and writes half (r + 1) & 1
            # (fl_compress.hip); the per-round statistic
            self.cp_res = torch.zeros(2 * self.Pimg, **f32)
            self.cp_stat = torch.zeros(mr, dtype=torch.float32, device=dev)
            ecfg.update({"compress": int(self.compress), "compress_k": int(self.compress_k),
                         "error_feedback": bool(cfg.error_feedback)})
            if self.compress_random:
                ecfg.update({"compress_levels": int(cfg.compress_levels), "compress_seed": int(self.compress_seed)})
            bufs.update({"compress_residual": self.cp_res.data_ptr(), "compress_stat": self.cp_stat.data_ptr()})
        if self.server:
            # server optimizer state: image-shaped fp32 (m = 0; v = tau^2 everywhere, padding included)
            if comm_buffers is not None:
                raise ValueError("trial packing (comm_buffers) does not run a server optimizer (server_opt)")
            self.server_m = torch.zeros(self.Pimg, **f32)
            self.server_v = torch.full((self.Pimg,), float(np.float32(cfg.server_tau)) ** 2, **f32)
            ecfg.update({"server_opt": int(self.server), "server_lr": float(cfg.server_lr),
                         "server_momentum": float(cfg.server_momentum), "server_beta2": float(cfg.server_beta2),
                         "server_tau": float(cfg.server_tau)})
            bufs.update({"server_m": self.server_m.data_ptr(), "server_v": self.server_v.data_ptr()})
        if self.secagg:
            # this client's clamped / NaN coordinates per round (uint32 words; integer atomics of fl_secagg.hip)
            self.sa_clamp = torch.zeros(mr, dtype=torch.int32, device=dev)
        if self.screen:
            # the round's kept-client mask (uint64 words; written by fl_screen.hip's select launch)
            self.screen_hist = torch.zeros(mr, dtype=torch.int64, device=dev)
        # gather_plane="xgmi": the native engine aggregates with the peer kernel's select / open call once the
        # peer plane is attached below (it needs the rule's parameters; the host plane launches from Python)
        want_select = xgmi_select and bool(self.robust or self.secagg) and comm_buffers is None
        if want_select and self.robust:
            ecfg.update({"robust": int(self.robust), "trim_ratio": float(cfg.trim_ratio)})
        elif want_select:
            ecfg.update({"secagg": True, "secagg_bits": int(cfg.secagg_bits), "secagg_seed": int(self.secagg_seed)})
            bufs["sa_clamp"] = self.sa_clamp.data_ptr()
        for i, R in enumerate(R_try):
            # rows sized for the longest row the engine may choose (the blocked row of the reference shape)
            # (an older library loaded through FEDMI_NATIVE_SO for an A/B knows the dense row only)
            row = self.m.slab_row_floats(self.dims, R) if hasattr(self.m, "slab_row_floats") else ((self.P + 1) + 3) & ~3
            self.slab = torch.zeros(((self.n_local + R - 1) // R) * row, **f32)
            ecfg["R"] = R
            bufs["slab"] = self.slab.data_ptr()
            bufs["slab_floats"] = self.slab.numel()
            try:
                self.engine = self.m.FLEngine(self.dims, ecfg, bufs)
                break
            except RuntimeError as err:
                if "LDS" not in str(err) or i + 1 == len(R_try):
                    raise
        self.R = R
        self.layout = self.engine.layout()
        # the configured rule (one client: the identity -- "mean"); a screen runs "mean" as the unweighted
        # mean of the kept clients
        self.layout["aggregator"] = cfg.aggregator if self.robust else AGGREGATORS[0]
        self.layout["screen"] = SCREENS[self.screen]
        if ALL_AGGREGATORS[self.robust] == "geomed":
            self.layout["geomed"] = {"iters": int(cfg.geomed_iters), "nu": float(np.float32(cfg.geomed_nu)),
                                     "launches": int(cfg.geomed_iters) + 1}
        if self.secagg:
            self.layout["secagg"] = {"bits": int(cfg.secagg_bits), "stream": SECAGG_STREAM}
        if self.attack:
            self.layout["attack"] = dict(self.attack_par)
        self.slab_f16 = bool(self.layout["slab_f16"])
        iw, ib, _ = image_layout(self.dims)
        if (self.layout["Pimg"], list(self.layout["iw_off"]), list(self.layout["ib_off"])) != (self.Pimg, iw, ib):
            raise RuntimeError(f"image layout mismatch between C++ and Python: {self.layout}")
        # the engine owns a non-default stream: graph capture is illegal on the null stream
        self.stream = stream if stream is not None else torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        self.rounds_issued = 0
        self._stopped_seen = False
        self._native_comm = None
        # one-shot xGMI all-reduce of [image | tails] (collective set-up; None -> RCCL)
        self._peer = None
        # (a robust aggregator and secure aggregation gather over the host plane -- neither the sum's peer
        # plane nor RCCL is set up; every rank shares the config, so that is collectively consistent -- or,
        # with gather_plane="xgmi", aggregate inside the peer kernel: the select set-up below)
        self._agg = None   # gathered stack + launcher of the aggregation kernels over it (_gather_launch)
        if self.world > 1 and comm_buffers is None and getattr(comm, "peer_allreduce", False) and not self.robust \
                and not self.secagg:
            from ..parallel.peer import make_peer_allreduce
            torch.cuda.synchronize(dev)
            # lagged rounds reduce inside the Adam kernel: one chunk flag per Adam block + the
            # two metric-tail chunks
            n_chunks = (self.P + 63) // 64 + 2 if (self._lag and int(cfg.local_steps) == 1) else 0
            self._peer = make_peer_allreduce(comm, comm_len, dev, n_chunks=n_chunks)
            if self._peer is not None:
                self.engine.attach_peer(self._peer)
        if want_select:
            # the peer kernel selects / opens instead of summing: no chunk flags (classic rounds); a set-up
            # that fails does so on every rank (make_peer_allreduce), and every rank then stays on the host gather
            if getattr(comm, "peer_allreduce", False):
                from ..parallel.peer import make_peer_allreduce
                torch.cuda.synchronize(dev)
                self._peer = make_peer_allreduce(comm, comm_len, dev, n_chunks=0)
            if self._peer is not None:
                self.engine.attach_peer(self._peer)
                self.layout["peer_select"] = self.engine.layout()["peer_select"]
            else:
                import warnings
                warnings.warn("gather_plane='xgmi': the one-shot xGMI peer plane is unavailable on this communicator; "
                              "aggregating over the host gather", RuntimeWarning, stacklevel=2)
        self.layout["gather_plane"] = "xgmi" if (want_select and self._peer is not None) else "host"
        if self.world > 1 and self._peer is None and comm_buffers is None and comm is not None \
                and hasattr(comm, "rccl") and not self.robust and not self.secagg:
            # RCCL only when the peer plane is off or fell back (every rank agreed on that above),
            # so this lazy, bounded bootstrap runs on every rank or on none; if it fails too, every
            # rank continues on the host plane (aggregation 'host') instead of raising
            self._native_comm = comm.rccl_or_host() if hasattr(comm, "rccl_or_host") else comm.rccl()
        self._graph_ready = False

    def __del__(self):
        # the xGMI communicator's buffers are read by the peers: never freed with the engine, but
        # retired until the next collective set-up (fedmi.parallel.peer.retire)
        peer = getattr(self, "_peer", None)
        if peer is not None:
            try:
                from ..parallel.peer import retire
                retire(peer)
            except Exception:  # noqa: BLE001 -- interpreter shutdown
                pass

    def slab_partials(self) -> torch.Tensor:
        """The last train kernel's per-workgroup gradient partials as [n_slabs, P] (a copy of the
        slab rows, fp32 or fp16, in dense-parameter order).  fp16 partials are sums of the
        unscaled gradient (the Adam kernel applies the 1/n)."""
        lay = self.engine.layout()
        ns, stride, P = int(lay["n_slabs"]), int(lay["slab_stride"]), self.P
        if self.slab_f16:  # fp16 partial e at half e of the row (fl_device.h slab_store_h)
            rows = self.slab.view(torch.float16)[:ns * 2 * stride].view(ns, 2 * stride)
            if lay.get("slab_blocked"):  # blocked rows (fl_layout.h FlSlabBlk): gathered into dense order
                pos = torch.as_tensor(self.engine.slab_map(), dtype=torch.long, device=rows.device)
                return rows[:, pos].clone()
            return rows[:, :P].clone()
        return self.slab[:ns * stride].view(ns, stride)[:, :P].clone()

    def slab_losses(self) -> torch.Tensor:
        """The last train kernel's per-workgroup loss slots as fp32 [n_slabs]: slab row b holds the sum
        of its rows' cross-entropies divided by the shard's n (the Adam kernel sums the slots into the
        round's history loss).  The slot is the float at index P of a row -- of fp32 and of dense fp16
        rows alike (fl_train_body.inc, fl_train_bf16_body.inc) -- and in a blocked fp16 row the float at
        the index that is the row's count of gradient halves, pads included (fl_layout.h FlSlabBlk::P):
        one past the last bias gradient, the largest position of ``slab_map()``."""
        lay = self.engine.layout()
        ns, stride, slot = int(lay["n_slabs"]), int(lay["slab_stride"]), self.P
        if self.slab_f16 and lay.get("slab_blocked"):
            slot = max(self.engine.slab_map()) + 1
        if not slot < stride:
            raise RuntimeError(f"slab row of {stride} floats has no loss slot at {slot}")
        return self.slab[:ns * stride].view(ns, stride)[:, slot].clone()

    def _pick_slab_f16(self, cfg) -> bool:
        if cfg.grad_slab not in ("auto", "fp16", "fp32"):
            raise ValueError(f"grad_slab must be 'auto', 'fp16' or 'fp32', got {cfg.grad_slab!r}")
        if cfg.dtype != "bf16" or cfg.grad_slab == "fp32":
            return False
        if cfg.grad_slab == "fp16":
            return True
        if self.X.numel() == 0:
            return True
        lo, hi = torch.aminmax(self.X)  # two scalars, no |X| temporary of the whole shard
        return bool(max(-float(lo), float(hi)) <= FP16_SLAB_MAX_ABS_X)

    def _round_tables(self, client_sizes=None):
        """Host-built device tables (fl_common.h FLBuffers::sched / rtab): per optimizer-step
        slot the Adam/StepLR scalars of this client's own step count (torch's double arithmetic,
        rounded to fp32 once), per round its FedAvg weight and the sampled-client set."""
        cfg = self.cfg
        mr, LS = max(1, int(cfg.max_rounds)), max(1, int(cfg.local_steps))
        b1, b2 = float(cfg.betas[0]), float(cfg.betas[1])
        sched = np.zeros(2 * mr * LS, np.float32)
        scale = np.zeros(mr, np.float32)
        count = np.zeros(mr, np.float32)
        mask = np.zeros((mr, 2), np.uint32)
        t_own = 0
        for r in range(mr):
            part = self.participants(r)
            active = self.rank in part
            if self.robust:
                w = 1.0   # unweighted: the contribution is the local model itself
            elif len(part) == self.world:
                w = float(self.n_local) / float(self.n_total)
            else:
                w = float(self.n_local) / float(sum(int(client_sizes[k]) for k in part))
            scale[r] = w if active else 0.0
            count[r] = len(part)
            bits = sum(1 << int(k) for k in part)
            mask[r] = (bits & 0xFFFFFFFF, bits >> 32)
            lr = float(cfg.lr) * float(cfg.gamma) ** (r // int(cfg.step_size))
            for ls in range(LS):
                t_own += int(active)
                t = max(t_own, 1)
                sched[2 * (r * LS + ls)] = lr / (1.0 - b1 ** t)
                sched[2 * (r * LS + ls) + 1] = math.sqrt(1.0 - b2 ** t)
        rtab = np.zeros((mr, 4), np.uint32)
        rtab[:, 0] = scale.view(np.uint32)
        rtab[:, 1] = count.view(np.uint32)
        rtab[:, 2:] = mask
        return sched, rtab.reshape(-1).view(np.int32)

    def _apply_early_stop(self) -> None:
        cfg = self.cfg
        self.engine.set_early_stop(int(cfg.patience), float(cfg.tolerance), float(cfg.rtol))
        self._graph_ready = False
        for st in self.state:     # the patience counter starts at the new patience
            rec = st.cpu().numpy().view(_STATE_DTYPE).copy()
            rec["count"] = int(cfg.patience)
            st.copy_(torch.as_tensor(rec.view(np.uint8)).to(st.device))
        torch.cuda.synchronize(self.device)

    @property
    def aggregation(self) -> str:
        """Data plane of the FedAvg all-reduce: 'none' (one client), 'xgmi-oneshot', 'rccl' or 'host';
        'host-gather': a robust aggregator, or secure aggregation, over every rank's gathered buffer;
        'xgmi-select': the same rules inside the one-shot xGMI peer kernel (``gather_plane='xgmi'``)."""
        if self.world == 1:
            return "none"
        if self.robust or self.secagg:
            return "xgmi-select" if self._peer is not None else "host-gather"
        if self._peer is not None:
            return "xgmi-oneshot+adam" if self.engine.adam_exchange else "xgmi-oneshot"
        return "rccl" if self._native_comm is not None else "host"

    # -- execution --
    def _stream(self) -> int:
        return self.stream.cuda_stream

    def _engine_reduces(self) -> bool:
        """The native engine issues the all-reduce itself (peer kernel or RCCL)."""
        return self._peer is not None or self._native_comm is not None

    def _phase_allreduce(self, r: int) -> None:
        if self.world == 1:
            if self.server or self.heldout:   # FedAvg of one client is the identity; the server step and
                self.engine.phase(r, 2, self._stream(), None)   # the held-out record still run
            return
        if self._engine_reduces():
            self.engine.phase(r, 2, self._stream(), self._native_comm)
        else:
            with torch.cuda.stream(self.stream):
                self._aggregate(r)
            self.server_step(r)
            self.heldout_step(r)

    def _aggregate(self, r: int) -> None:
        """Aggregation of round ``r`` from Python, on the current stream, in place in the round's
        output buffer: the communicator's SUM all-reduce, or (robust aggregators) a gather of every
        rank's buffer over the host plane and one fl_robust launch over the gathered stack."""
        buf = self.params[(r + 1) & 1]
        if self.secagg:
            self._aggregate_secagg(r)
            return
        if not self.robust:
            self.comm.allreduce_(buf)
            return
        stack, agg = self._gather_launch()
        self.comm.allgather_device(buf, out=stack)
        s = torch.cuda.current_stream(self.device).cuda_stream
        if self.attack_stage:
            # Byzantine attack model: every rank rewrites its copy of the bad ranks' rows, then screens / aggregates
            agg.attack((r + 1) & 1, s)
        agg.robust((r + 1) & 1, s)

    def _gather_launch(self):
        """The gathered stack of every rank's buffer and the launcher of the aggregation kernels over it
        (sources: its rows; destination and masked buffer: this rank's ``params[par]``), built on first use."""
        if self._agg is None:
            # (a row is Pimg + tails floats, so rows past the first are float-aligned only when the tails are
            # no multiple of 4: the kernels' float4 loads of the rows rely on gfx950's global dwordx4 loads
            # taking dword-aligned addresses, as fl_robust's always have; the attack stage's K <= 8 buckets
            # also STORE float4s into the rows of the bad ranks -- global dwordx4 stores take dword-aligned
            # addresses in the same way, and tests/test_attack.py's three ranks run that case: rows of
            # Pimg + 30 floats)
            stack = torch.empty((self.world, self.params[0].numel()), dtype=torch.float32, device=self.device)
            rows = [stack[k] for k in range(self.world)]
            self._agg = (stack, _AggLaunch(self, [rows, rows], [[p] for p in self.params],
                                           clamps=[self.sa_clamp] if self.secagg else (), first_client=self.rank))
        return self._agg

    def _aggregate_secagg(self, r: int) -> None:
        """Secure aggregation of round ``r`` on the current stream: fl_secagg_mask on this rank's buffer, a
        gather of every rank's MASKED buffer over the host plane, fl_secagg_open over the gathered stack
        into the round's output buffer."""
        stack, agg = self._gather_launch()
        par = (r + 1) & 1
        s = torch.cuda.current_stream(self.device).cuda_stream
        agg.mask(par, s)
        self.comm.allgather_device(self.params[par], out=stack)
        agg.open(par, s)

    def server_step(self, r: int) -> None:
        """Server-optimizer step of round ``r`` on the aggregated image a caller summed into
        ``params[(r + 1) & 1]`` (host-plane all-reduce, :class:`~fedmi.fl.simulate.ClientGroup`);
        nothing without a server optimizer."""
        if self.server:
            self.engine.phase(r, 3, self._stream(), None)

    # -- held-out scoring of the global model (fedmi/ops/csrc/fl_heldout.hip), inference --
    def set_heldout(self, X, y, keep_best: bool = False) -> None:
        if self._packed:
            raise ValueError("trial packing (comm_buffers) does not run held-out scoring (set_heldout)")
        X, y = self._check_heldout(X, y)
        self.stream.synchronize()
        dev, C, mr = self.device, self.n_classes, int(self.cfg.max_rounds)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ho_X = torch.as_tensor(X, device=dev)
        self.ho_y = torch.as_tensor(y.astype(np.int32), device=dev)
        nblk = -(-len(X) // int(self.engine.heldout_rows_per_block))
        self.ho_scratch = torch.zeros(nblk * (C * C + 1), **i32)   # one partial per workgroup of the row launch
        if not self.heldout:
            self.ho_cm = torch.zeros(mr * C * C, **i32)
            self.ho_loss = torch.zeros(mr, dtype=torch.float32, device=dev)
            # {best loss sum (+inf), best round (-1)} as two words, and the best round's image
            self.ho_best = torch.as_tensor(np.array([0x7F800000, -1], np.int32), device=dev)
            self.ho_best_image = torch.zeros(self.Pimg, dtype=torch.float32, device=dev)
        self.hist.enable_heldout(C, len(X))
        torch.cuda.current_stream(dev).synchronize()
        # (the fold tracks the best round whether or not its image is kept: history()["heldout_best_round"])
        self.engine.set_heldout(self.ho_X.data_ptr(), self.ho_y.data_ptr(), len(X), self.ho_scratch.data_ptr(),
                                self.ho_cm.data_ptr(), self.ho_loss.data_ptr(), self.ho_best_image.data_ptr(),
                                self.ho_best.data_ptr(), True)
        self.heldout, self.keep_best = True, bool(keep_best)
        self._graph_ready = False   # the native engine dropped its graphs, as for set_debug
        self._mirror = None         # the streaming mirror gains the held-out buffers

    def heldout_step(self, r: int) -> None:
        if self.heldout:
            self.engine.phase(r, 4, self._stream(), None)

    def _ho_best_words(self):
        w = self.ho_best.cpu().numpy()
        return float(w.view(np.float32)[0]), int(w[1])

    def _ho_best_sum(self) -> float:
        self.stream.synchronize()
        return self._ho_best_words()[0]

    def _read_heldout(self, n: int, cm, loss, best) -> None:
        """Rows [0, n) and the best round from (device or pinned-host) copies of the held-out buffers."""
        C = self.n_classes
        if n:
            self.hist.ho_cm[:n] = cm[:n * C * C].cpu().numpy().reshape(n, C, C)
            self.hist.ho_loss[:n] = loss[:n].cpu().numpy()
        self.hist.ho_best_round = int(best.cpu().numpy()[1])

    def best_flat(self) -> np.ndarray:
        if not (self.heldout and self.keep_best):
            raise RuntimeError("best_flat: needs set_heldout(X, y, keep_best=True)")
        self.stream.synchronize()
        if self._ho_best_words()[1] < 0:
            raise RuntimeError("best_flat: no round has won yet")
        return image_to_dense(self.ho_best_image.cpu().numpy(), self.dims)

    def _predict(self, X, which: str, proba: bool):
        if which not in ("global", "local", "best"):
            raise ValueError(f"which must be 'global', 'local' or 'best', got {which!r}")
        X = self._check_rows(X)
        n, C, dev = int(X.shape[0]), self.n_classes, self.device
        out = np.zeros((n, C), np.float32) if proba else np.zeros(n, np.int64)
        if which == "best":
            self.best_flat()   # raises without keep_best or before a first win
        p = {"local": self.local, "best": getattr(self, "ho_best_image", None),
             "global": self.params[self.rounds_issued & 1][:self.Pimg]}[which]
        chunk = 1 << 20   # rows per launch (the kernel takes up to 2^24)
        for i0 in range(0, n, chunk):
            Xt = torch.as_tensor(X[i0:i0 + chunk], device=dev)
            m = int(Xt.shape[0])
            o = torch.empty((m, C), dtype=torch.float32, device=dev) if proba else \
                torch.empty(m, dtype=torch.int32, device=dev)
            self.stream.wait_stream(torch.cuda.current_stream(dev))
            self.engine.predict(Xt.data_ptr(), m, p.data_ptr(), o.data_ptr() if proba else 0,
                                0 if proba else o.data_ptr(), self._stream())
            self.stream.synchronize()
            out[i0:i0 + m] = o.cpu().numpy()
        return out

    def predict_proba(self, X, which: str = "global") -> np.ndarray:
        return self._predict(X, which, True)

    def predict(self, X, which: str = "global") -> np.ndarray:
        return self._predict(X, which, False)

    def _issue_debug(self, n: int) -> None:
        """Debug mode: every phase launched eagerly and synchronised, so a
        fault is attributed to its kernel, and weights / metric tails checked for NaN/Inf
        after every local step and every aggregation."""
        s = self._stream()
        for _ in range(n):
            r = self.rounds_issued
            out = self.params[(r + 1) & 1]
            self.engine.phase(r, 0, s, None)
            self.stream.synchronize()
            _check_finite(r, "local weights after the Adam step", self.local)
            self.engine.phase(r, 1, s, None)
            self.stream.synchronize()
            self._phase_allreduce(r)
            self.stream.synchronize()
            _check_finite(r, "aggregated weights / metric tails", out)
            self.rounds_issued += 1

    def profile(self, n: int) -> Dict[str, float]:
        """Run ``n`` live rounds eagerly with hipEvents around each phase; returns mean
        microseconds of local step (train + Adam kernels), eval, all-reduce and round."""
        s = self._stream()
        names = ("train", "eval", "allreduce")
        acc = dict.fromkeys(names + ("round",), 0.0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        n = min(n, self.cfg.max_rounds - self.rounds_issued)
        for _ in range(n):
            r = self.rounds_issued
            ev[0].record(self.stream)
            self.engine.phase(r, 0, s, None)
            ev[1].record(self.stream)
            self.engine.phase(r, 1, s, None)
            ev[2].record(self.stream)
            self._phase_allreduce(r)
            ev[3].record(self.stream)
            self.stream.synchronize()
            for i, k in enumerate(names):
                acc[k] += 1e3 * ev[i].elapsed_time(ev[i + 1])
            acc["round"] += 1e3 * ev[0].elapsed_time(ev[3])
            self.rounds_issued += 1
        self.sync_history()
        return {k + "_us": v / max(n, 1) for k, v in acc.items()}

    def trace(self, n: int, close: bool = False, gate_us: float = 5000.0, warm: int = 0) -> Dict[str, object]:
        """Per-kernel breakdown of ``n`` rounds of the engine's REAL round design (unlike
        :meth:`profile`, which runs classic phases): the native engine issues them eagerly with
        a hipEvent after every launch behind a gate kernel (FLEngine::trace), so the kernels
        run back to back.  Returns mean us per round by kernel kind (``train``, ``adam``,
        ``eval``, ``pack``, ``allreduce``, ``eval_fedavg``, ``dp``, ``compress``, ``server``, ``heldout``), ``round`` and launch counts.  Each
        interval carries the eager launch + event marker cost: measured on MI355X (bench N = 1,
        profiles/kernel_trace_r5.log) ~1.5 us per kernel over the rocprofv3 kernel durations
        (markers without the system-scope fence; ~3.2 us with it).
        Collective on multi-client engines (every rank must call it with the same ``n``);
        ``warm`` untraced rounds run first behind the gate (they absorb the ranks' start skew)."""
        if self.cfg.debug or (self.world > 1 and not self._engine_reduces()):
            raise RuntimeError("trace: needs an engine that issues its own FedAvg")
        n, warm = int(n), int(warm)
        if n < 1 or warm < 0 or self.rounds_issued + warm + n > self.cfg.max_rounds:
            raise RuntimeError("trace: needs n >= 1 and warm + n rounds left (max_rounds)")
        # (pending host-side weight changes etc. are handled inside run(), like eager rounds)
        out = dict(self.engine.trace(self.rounds_issued, n, self._stream(), self._native_comm,
                                     close=close, gate_us=gate_us, warm=warm))
        self.rounds_issued += warm + n
        return out

    def _issue(self, n: int, close: bool = True, graph_rounds: Optional[int] = None) -> None:
        """Issue rounds [rounds_issued, rounds_issued + n) on the current stream.

        ``close=False`` (lagged engines): the last round stays lagged -- its evaluation is
        done by the next issued round's train kernel, so every round of the call can be a
        graph replay.  The host must issue at least one more (closing) round before it reads
        the history.  ``graph_rounds``: rounds per replayed graph (default: the config's)."""
        if self.cfg.debug:
            self._issue_debug(n)
            return
        s = self._stream()
        r0 = self.rounds_issued
        g = int(self.cfg.graph_rounds if graph_rounds is None else graph_rounds)
        if self.world > 1 and not self._engine_reduces():
            # torch-owned communicator: all-reduce from Python between rounds
            with torch.cuda.stream(self.stream):
                for r in range(r0, r0 + n):
                    self.engine.run_local(r, s)
                    self._aggregate(r)
                    self.server_step(r)
                    self.heldout_step(r)
            self.rounds_issued += n
            return
        # lagged engines: graphs hold lagged rounds only, the last round of the call is eager and
        # evaluates itself (then every metric is in the buffers for the host)
        lag = bool(self.engine.lagged) and close
        r = r0
        while r < r0 + n:
            left = r0 + n - r
            if (g >= 2 and r % 2 == 0 and (left > g if lag else left >= g)
                    and not self.engine.needs_eager_round()):
                self._ensure_graph(g)
                self.engine.replay(s)
                r += g
            else:
                self.engine.run(r, 1, s, self._native_comm, close=(close and r == r0 + n - 1))
                r += 1
        self.rounds_issued = r

    def set_debug(self, ptr: int) -> None:
        """Phase stamps (fl_device.h) into the device buffer at ``ptr`` (0: off).  A configuration
        change: the native engine drops its cached graphs, and so does this side."""
        self.engine.set_debug(int(ptr))
        self._graph_ready = False

    def _ensure_graph(self, g: int) -> None:
        if not self._graph_ready or self.engine.graph_rounds() != g:
            self.engine.capture(g, self._stream(), self._native_comm)
            self._graph_ready = True

    def prime_graph(self, g: int, replays: int = 1) -> int:
        """Bring the engine to the steady state of a ``g``-round graph before a timed region:
        issue (uncounted by the caller) eager rounds until the next round is even and may start
        a graph, capture + instantiate the graph and replay it ``replays`` times (the second launch
        of a freshly instantiated graph runs ~0.6 us per round slower than later ones,
        profiles/short_region_r4*.log).  Afterwards ``_issue(k * g, close=False)`` is ``k`` graph
        replays.  Returns the rounds issued."""
        if g < 2 or g % 2:
            raise ValueError("graph rounds must be an even number >= 2")
        if self.world > 1 and not self._engine_reduces():
            raise RuntimeError("prime_graph: rounds aggregated from Python are not captured")
        self.cfg.graph_rounds = g
        r0 = self.rounds_issued
        s = self._stream()
        for _ in range(4):
            if self.rounds_issued % 2 == 0 and not self.engine.needs_eager_round():
                break
            self.engine.run(self.rounds_issued, 1, s, self._native_comm, close=False)
            self.rounds_issued += 1
        else:
            raise RuntimeError("prime_graph: engine did not reach a graph-capturable state")
        self._ensure_graph(g)
        for _ in range(max(1, int(replays))):
            self.engine.replay(s)
            self.rounds_issued += g
        return self.rounds_issued - r0

    def _read_state(self, idx: int) -> np.ndarray:
        self.stream.synchronize()
        self._check_peer()
        return self.state[idx].cpu().numpy().view(_STATE_DTYPE)[0]

    # -- step-by-step API (reference train_one_epoch / evaluate_local / federated_averaging)
    def step_train(self) -> None:
        self.engine.phase(self.rounds_issued, 0, self._stream(), None)

    def step_eval(self) -> np.ndarray:
        r = self.rounds_issued
        self.engine.phase(r, 1, self._stream(), None)
        self.stream.synchronize()
        C = self.n_classes
        t0 = self.Pimg + self.rank * self.tail_stride
        if self._peer is not None:  # published into the peer send buffer, not yet reduced
            cm = np.asarray(self._peer.read((r + 1) & 1, t0, C * C), dtype=np.float32)
        else:
            cm = self.params[(r + 1) & 1][t0:t0 + C * C].cpu().numpy()
        return cm.reshape(C, C).astype(np.int64)

    def step_aggregate(self) -> None:
        r = self.rounds_issued
        self._phase_allreduce(r)
        self.rounds_issued += 1
        st = self._read_state(self.rounds_issued & 1)
        if st["stopped"]:
            self._stopped_seen = True

    def run(self, n_rounds: int, check_every: int = 64) -> int:
        """Run up to ``n_rounds`` rounds; returns the number of live rounds.  The stop
        flag is polled once per ``check_every`` rounds (rounds issued past an early stop
        are exact no-ops on the device)."""
        before = self.hist.rounds_run
        left = min(n_rounds, self.cfg.max_rounds - self.rounds_issued)
        while left > 0 and not self._stopped_seen:
            n = min(left, check_every)
            self._issue(n)
            left -= n
            st = self._read_state(self.rounds_issued & 1)
            if st["stopped"]:
                self._stopped_seen = True
        self.sync_history()
        return self.hist.rounds_run - before

    def run_streaming(self, n_rounds: int, chunk: int = 16, on_history=None, guard=None) -> int:
        """:meth:`run` with the metrics streamed as the rounds complete: rounds are issued in
        chunks of ``chunk``, and after each chunk a finalize plus an asynchronous copy of the
        round state and metric history into pinned host memory are queued behind it.  Chunk k+1
        is issued BEFORE chunk k's copy is waited on, so the device never idles on the host, and
        ``on_history(history)`` sees round r while at most one chunk (<= ``chunk`` rounds) runs
        after it (the reference prints every round as it completes, C:139-179).  ``guard(desc)``:
        optional context manager around each chunk (the collective watchdog).  Returns the number
        of live rounds; rounds issued past an early stop are exact no-ops on the device."""
        import contextlib
        before = self.hist.rounds_run
        left = min(int(n_rounds), self.cfg.max_rounds - self.rounds_issued)
        if self.cfg.debug or (self.world > 1 and not self._engine_reduces()):
            while left > 0 and not self._stopped_seen:   # host-driven rounds: chunk by chunk
                n = min(chunk, left)
                with (guard(f"rounds {self.rounds_issued}..{self.rounds_issued + n - 1}") if guard
                      else contextlib.nullcontext()):
                    self.run(n, check_every=n)
                left -= n
                if on_history is not None:
                    on_history(self.history())
            return self.hist.rounds_run - before
        # graph rounds per chunk: lagged engines close every chunk with an eager self-evaluating
        # round, and a lagged graph starts only behind a lagged round that scored its predecessor
        # (FLEngine::needs_eager_round), so a chunk is 2 eager lagged rounds + the graph + 1 lagged
        # + the closing round (graph + 4, even, so every chunk starts on an even round)
        g = int(self.cfg.graph_rounds)
        if g >= 2:
            gs = max(2, (min(g, chunk) - (4 if self.engine.lagged else 0)) & ~1)
            step = gs + (4 if self.engine.lagged else 0)
        else:
            gs, step = 0, max(1, chunk)
        mirror = self._host_mirror()
        s = self._stream()
        pend = None
        slot = 0
        while True:
            new = None
            if left > 0 and not self._stopped_seen:
                n = min(step, left)
                desc = f"rounds {self.rounds_issued}..{self.rounds_issued + n - 1}"
                with (guard(desc) if guard else contextlib.nullcontext()):
                    self._issue(n, graph_rounds=gs)
                left -= n
                r = self.rounds_issued
                self.engine.finalize(r, s)
                m = mirror[slot]
                with torch.cuda.stream(self.stream):
                    m["state"].copy_(self.state[(r + 1) & 1], non_blocking=True)
                    m["glob"].copy_(self.h_global, non_blocking=True)
                    m["rank"].copy_(self.h_rank, non_blocking=True)
                    m["loss"].copy_(self.h_loss, non_blocking=True)
                    if self.dp:
                        m["norm"].copy_(self.dp_norm, non_blocking=True)
                    if self.compress:
                        m["cstat"].copy_(self.cp_stat, non_blocking=True)
                    if self.secagg:
                        m["clamp"].copy_(self.sa_clamp, non_blocking=True)
                    if self.screen:
                        m["screen"].copy_(self.screen_hist, non_blocking=True)
                    if self.heldout:
                        m["ho_cm"].copy_(self.ho_cm, non_blocking=True)
                        m["ho_loss"].copy_(self.ho_loss, non_blocking=True)
                        m["ho_best"].copy_(self.ho_best, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
                new = (ev, slot, desc)
                slot ^= 1
            if pend is not None:
                with (guard(pend[2]) if guard else contextlib.nullcontext()):
                    pend[0].synchronize()
                # fail fast: a failure reported on the xGMI plane (a peer died / stalled, or
                # aborted) invalidates this chunk's rounds -- raise before they are folded or printed
                self._check_peer()
                self._fold_mirror(mirror[pend[1]])
                if on_history is not None:
                    on_history(self.history())
            pend = new
            if pend is None:
                break
        self._check_peer()
        self._check_slab_saturation()
        return self.hist.rounds_run - before

    def _check_peer(self) -> None:
        """Raise (fedmi.parallel.peer.PeerFailure) if any rank reported a failure of the xGMI
        data plane; every host-visible result since then is invalid."""
        if self._peer is not None:
            from ..parallel.peer import check_peer_error
            check_peer_error(self._peer)

    def _host_mirror(self):
        """Two pinned-host copies (double-buffered by chunk) of the round state and history."""
        if getattr(self, "_mirror", None) is None:
            pin = torch.cuda.is_available()
            mk = lambda t: torch.empty(t.shape, dtype=t.dtype, pin_memory=pin)
            self._mirror = [{"state": mk(self.state[0]), "glob": mk(self.h_global), "rank": mk(self.h_rank),
                             "loss": mk(self.h_loss), **({"norm": mk(self.dp_norm)} if self.dp else {}),
                             **({"cstat": mk(self.cp_stat)} if self.compress else {}),
                             **({"clamp": mk(self.sa_clamp)} if self.secagg else {}),
                             **({"screen": mk(self.screen_hist)} if self.screen else {}),
                             **({"ho_cm": mk(self.ho_cm), "ho_loss": mk(self.ho_loss), "ho_best": mk(self.ho_best)}
                                if self.heldout else {})}
                            for _ in range(2)]
        return self._mirror

    def _fold_mirror(self, m) -> None:
        st = m["state"].numpy().view(_STATE_DTYPE)[0]
        n = int(st["finalized"])
        self.hist.rounds_run = n
        if n:
            self.hist.glob[:n] = m["glob"][:n * 4].numpy().reshape(n, 4)
            self.hist.rank[:n] = m["rank"][:n * self.world * 4].numpy().reshape(n, self.world, 4)
            self.hist.loss[:n] = m["loss"][:n].numpy()
            if self.dp:
                self.hist.norm[:n] = m["norm"][:n].numpy()
            if self.compress:
                self.hist.cstat[:n] = m["cstat"][:n].numpy()
            if self.secagg:
                self.hist.clamped[:n] = m["clamp"][:n].numpy().view(np.uint32)
            if self.screen:
                self.hist.screen[:n] = m["screen"][:n].numpy().view(np.uint64)
        if self.heldout:
            self._read_heldout(n, m["ho_cm"], m["ho_loss"], m["ho_best"])
        if st["stopped"]:
            self.hist.stop_round = int(st["stop_round"])
            self.hist.stop_trigger = int(st["stop_round"]) - 1
            self._stopped_seen = True

    @property
    def stopped(self) -> bool:
        return self._stopped_seen

    def sync_history(self) -> None:
        r = self.rounds_issued
        s = self._stream()
        self.engine.finalize(r, s)
        self.read_history()

    def read_history(self) -> None:
        """Copy the device history of the rounds issued into ``hist`` (after a finalize of
        ``rounds_issued``: this engine's ``sync_history`` or its trial batch's)."""
        r = self.rounds_issued
        st = self._read_state((r + 1) & 1)   # synchronizes the engine stream
        n = int(st["finalized"])
        self.hist.rounds_run = n
        if n:
            self.hist.glob[:n] = self.h_global[:n * 4].cpu().numpy().reshape(n, 4)
            self.hist.rank[:n] = self.h_rank[:n * self.world * 4].cpu().numpy().reshape(n, self.world, 4)
            self.hist.loss[:n] = self.h_loss[:n].cpu().numpy()
            if self.dp:
                self.hist.norm[:n] = self.dp_norm[:n].cpu().numpy()
            if self.compress:
                self.hist.cstat[:n] = self.cp_stat[:n].cpu().numpy()
            if self.secagg:
                self.hist.clamped[:n] = self.sa_clamp[:n].cpu().numpy().view(np.uint32)
            if self.screen:
                self.hist.screen[:n] = self.screen_hist[:n].cpu().numpy().view(np.uint64)
        if self.heldout:
            self._read_heldout(n, self.ho_cm, self.ho_loss, self.ho_best)
        if st["stopped"]:
            self.hist.stop_round = int(st["stop_round"])
            self.hist.stop_trigger = int(st["stop_round"]) - 1
            self._stopped_seen = True
        self._check_slab_saturation()

    def _check_slab_saturation(self) -> None:
        if self.slab_f16 and not self.slab_saturated and int(self.sat.item()):
            self.slab_saturated = True
            msg = ("fp16 gradient slab saturated (a per-workgroup partial reached +-65504 or is not finite): the "
                   "gradients of those rounds are clipped; rerun with EngineConfig(grad_slab='fp32')")
            if self.cfg.debug:
                raise FloatingPointError(msg)
            import warnings
            warnings.warn(msg, RuntimeWarning, stacklevel=2)

    def global_flat(self) -> np.ndarray:
        self.stream.synchronize()
        return image_to_dense(self.params[self.rounds_issued & 1][:self.Pimg].cpu().numpy(), self.dims)

    def local_flat(self) -> np.ndarray:
        self.stream.synchronize()
        return image_to_dense(self.local.cpu().numpy(), self.dims)

    def set_global_flat(self, flat: np.ndarray) -> None:
        self.stream.synchronize()
        self.params[self.rounds_issued & 1][:self.Pimg].copy_(torch.as_tensor(dense_to_image(flat, self.dims)))
        torch.cuda.current_stream(self.device).synchronize()
        self.engine.invalidate()

    def confusion(self, X=None, y=None, flat=None) -> np.ndarray:
        Xt = self.X if X is None else torch.as_tensor(np.ascontiguousarray(X, np.float32), device=self.device)
        yt = self.y if y is None else torch.as_tensor(np.asarray(y), dtype=torch.int32, device=self.device)
        if flat is None:
            p = self.local
        else:
            p = torch.as_tensor(dense_to_image(flat, self.dims), device=self.device)
        cm = torch.zeros(self.n_classes ** 2, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        self.engine.confusion(Xt.data_ptr(), yt.data_ptr(), int(Xt.shape[0]), p.data_ptr(), cm.data_ptr(),
                              self._stream())
        self.stream.synchronize()
        return cm.cpu().numpy().reshape(self.n_classes, self.n_classes).astype(np.int64)

    @property
    def compress_residual(self) -> np.ndarray:
        """The compression residual in dense order, as the next live round will read it (after
        :meth:`sync_history`: the half the last live round wrote)."""
        self.stream.synchronize()
        half = int(self.hist.rounds_run) & 1
        return image_to_dense(self.cp_res[half * self.Pimg:(half + 1) * self.Pimg].cpu().numpy(), self.dims)

    def portable_state(self) -> dict:
        self.sync_history()
        r = self.rounds_issued
        st = self._read_state((r + 1) & 1)   # the finalized copy (sync_history folded round r-1)
        return {
            "rounds": int(r), "global": self.global_flat(), "local": self.local_flat(),
            "exp_avg": image_to_dense(self.mom.cpu().numpy(), self.dims),
            "exp_avg_sq": image_to_dense(self.vel.cpu().numpy(), self.dims), "opt_steps": self.own_steps(int(r)),
            "es": {"count": int(st["count"]), "has_prev": bool(st["has_prev"]),
                   "prev": [float(x) for x in st["prev"]], "stopped": bool(st["stopped"]),
                   "stop_round": int(st["stop_round"])},
            "history": self.hist.as_dict(),
            **({"dp_seed": int(self.dp_seed)} if self.dp else {}),
            **({"server_m": image_to_dense(self.server_m.cpu().numpy(), self.dims),
                "server_v": image_to_dense(self.server_v.cpu().numpy(), self.dims)} if self.server else {}),
            **self._compress_state_out(self.compress_residual if self.compress else None),
            **self._heldout_state_out(None if not (self.heldout and self.keep_best and self._ho_best_words()[1] >= 0)
                                      else self.best_flat()),
        }

    def load_portable_state(self, st: dict) -> None:
        r = int(st["rounds"])
        if r > self.cfg.max_rounds:
            raise ValueError(f"checkpoint has {r} rounds > max_rounds {self.cfg.max_rounds}")
        sv = self._server_state_in(st)
        ce = self._compress_state_in(st)
        ho = self._heldout_state_in(st)
        self.stream.synchronize()
        dev = self.device
        img = lambda a: torch.as_tensor(dense_to_image(np.asarray(a, np.float32), self.dims), device=dev)
        with torch.cuda.stream(self.stream):
            self.params[r & 1][:self.Pimg].copy_(img(st["global"]))
            self.local.copy_(img(st["local"]))
            self.mom.copy_(img(st["exp_avg"]))
            self.vel.copy_(img(st["exp_avg_sq"]))
            if sv is not None:
                self.server_m.copy_(img(sv[0]))
                # padding of v keeps tau^2 (dense_to_image pads with zeros)
                pad = torch.as_tensor(dense_to_image(np.ones(self.P, np.float32), self.dims), device=dev) == 0
                self.server_v.copy_(torch.where(pad, torch.full_like(self.server_v, float(np.float32(self.cfg.server_tau)) ** 2),
                                                img(sv[1])))
            if ce is not None:   # both halves: whichever the next live round reads
                self.cp_res.copy_(img(ce).repeat(2))
            es = st["es"]
            rec = np.zeros(1, dtype=_STATE_DTYPE)
            rec["next_round"] = r
            rec["finalized"] = r
            rec["cur_round"] = r - 1
            rec["count"] = int(es["count"])
            rec["has_prev"] = int(bool(es["has_prev"]))
            rec["prev"] = np.asarray(es["prev"], np.float64)
            rec["stopped"] = int(bool(es["stopped"]))
            rec["stop_round"] = int(es["stop_round"])
            # the peer exchange's call counter stays monotonic (peers' flags hold past calls)
            rec["calls"] = max(int(self.state[q].cpu().numpy().view(_STATE_DTYPE)[0]["calls"]) for q in (0, 1))
            self.state[r & 1].copy_(torch.as_tensor(rec.view(np.uint8).copy()).to(dev))
            self._load_history(st["history"])
            n = self.hist.rounds_run
            if self.secagg:
                self.sa_clamp.zero_()   # the mask kernel ADDS to a round's count: rounds run again start from 0
            if n:
                self.h_global[:n * 4].copy_(torch.as_tensor(self.hist.glob[:n].reshape(-1), device=dev))
                self.h_rank[:n * self.world * 4].copy_(torch.as_tensor(self.hist.rank[:n].reshape(-1), device=dev))
                self.h_loss[:n].copy_(torch.as_tensor(self.hist.loss[:n], device=dev))
                if self.dp:
                    self.dp_norm[:n].copy_(torch.as_tensor(self.hist.norm[:n], device=dev))
                if self.compress:
                    self.cp_stat[:n].copy_(torch.as_tensor(self.hist.cstat[:n], device=dev))
                if self.secagg:
                    self.sa_clamp[:n].copy_(torch.as_tensor(self.hist.clamped[:n].astype(np.uint32).view(np.int32),
                                                            device=dev))
                if self.screen:
                    self.screen_hist[:n].copy_(torch.as_tensor(self.hist.screen[:n].view(np.int64), device=dev))
            if ho is not None:
                # the rows continue behind the checkpoint's, the best so far stays the round to beat
                C = self.n_classes
                self.ho_cm.zero_()
                self.ho_loss.zero_()
                if n:
                    self.ho_cm[:n * C * C].copy_(torch.as_tensor(self.hist.ho_cm[:n].reshape(-1).astype(np.int32),
                                                                 device=dev))
                    self.ho_loss[:n].copy_(torch.as_tensor(self.hist.ho_loss[:n], device=dev))
                words = np.array([np.float32(ho["best_loss_sum"]).view(np.int32), int(self.hist.ho_best_round)], np.int32)
                if ho.get("best_flat") is not None:
                    self.ho_best_image.copy_(img(ho["best_flat"]))
                elif self.keep_best:
                    # a state saved without keep_best has no image of its best round: the next round to
                    # score starts the search again, so best_flat() never returns an image nobody wrote
                    words = np.array([0x7F800000, -1], np.int32)
                    self.hist.ho_best_round = -1
                self.ho_best.copy_(torch.as_tensor(words, device=dev))
        self.stream.synchronize()
        self._load_dp_seed(st)
        self._load_compress_seed(st)
        self.engine.invalidate()
        self.engine.reset_pending()
        self.rounds_issued = r
        self._stopped_seen = bool(st["es"]["stopped"])

    def _set_dp_seed(self, seed: int) -> None:
        self.dp_seed = int(seed)
        self.engine.set_dp_seed(int(seed))   # a kernel argument: the native engine drops its graphs
        self._graph_ready = False

    def _set_compress_seed(self, seed: int) -> None:
        self.compress_seed = int(seed)
        self.engine.set_compress_seed(int(seed))   # a kernel argument: the native engine drops its graphs
        self._graph_ready = False

    def state_dict(self) -> dict:
        self.stream.synchronize()
        return {"params": self.global_flat(), "local": self.local_flat(),
                "exp_avg": image_to_dense(self.mom.cpu().numpy(), self.dims),
                "exp_avg_sq": image_to_dense(self.vel.cpu().numpy(), self.dims), "rounds": self.rounds_issued,
                "state": self.state[self.rounds_issued & 1].cpu().numpy(), "history": self.hist.as_dict()}


def _check_finite(r: int, what: str, t: torch.Tensor) -> None:
    if not bool(torch.isfinite(t).all()):
        bad = int((~torch.isfinite(t)).sum())
        raise FloatingPointError(f"round {r}: {bad} non-finite values in {what}")


def comm_len(dims: Sequence[int], world: int) -> int:
    """Floats in one FedAvg buffer of the HIP engine: parameter image + per-rank tails."""
    n_classes = int(dims[-1])
    return image_layout(list(dims))[2] + world * (n_classes * n_classes + 1)


class _ShapeOnly:
    """Stand-in so the base class can read ``len(X)``/``X.shape`` of device tensors."""

    def __init__(self, n, f):
        self.shape = (n, f)

    def __len__(self):
        return self.shape[0]


def make_engine(X, y, n_classes, cfg: EngineConfig, comm, init_flat, n_total=None, backend: str = "auto"):
    if backend == "auto":
        backend = "hip" if (comm is not None and comm.device.type == "cuda") or \
            (comm is None and torch.cuda.is_available()) else "torch"
    if backend == "hip":
        return HipRoundEngine(X, y, n_classes, cfg, comm, init_flat, n_total)
    if backend == "torch":
        return TorchRoundEngine(X, y, n_classes, cfg, comm, init_flat, n_total)
    raise ValueError(f"unknown engine backend {backend!r}")

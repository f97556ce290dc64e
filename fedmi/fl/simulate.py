"""Several federated clients in ONE process (simulation mode).

The deployment model is one process per GPU, each GPU one client (``fedmi.parallel.comm``).
Some studies need more clients than processes -- the rounds-to-target distributions at
k = 2/4/8 on a one-GPU box, k > 8 clients on one node, quick CPU oracles -- so this module
runs k clients' round engines side by side in one process and replaces the cross-process
all-reduce with an in-process sum of their FedAvg buffers in rank order (the same left fold
the one-shot xGMI kernel uses, so the result equals a real k-rank run's arithmetic).

Semantics are the reference's, client for client: every client owns its shard
(``_split_data``, FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py:48-61), trains
(C:145), evaluates its post-step local model (C:148), and all clients adopt the
sample-weighted average (C:101-120); the global metrics / early-stop rule see every
client's tail (C:165-192).

* ``backend='hip'``: k :class:`~fedmi.fl.engine.HipRoundEngine` on one device stream, classic
  rounds (train + Adam + eval kernels per client), the k FedAvg buffers summed on the device.
* ``backend='torch'``: k :class:`~fedmi.fl.engine.TorchRoundEngine` (CPU oracle).

With a robust aggregator (``EngineConfig.aggregator``) the in-process sum is replaced by the
coordinate-wise median / trimmed mean of the sampled clients' buffers: one ``fl_robust`` launch,
in place over the k buffers, on the device; ``robust_aggregate_torch`` on the CPU.  ``"geomed"``
takes the same place with its ``geomed_iters + 1`` launches (``fl_geomed.hip``); ``geomed_torch`` on
the CPU.

With a client screen (``EngineConfig.screen``, multi-Krum) two more launches run in front of that one
-- the pairwise distances of the sampled clients' images and the selection of the kept clients
(``fl_screen.hip``) -- and the rule takes the kept clients; ``pair_distances_torch`` and
``screen_select`` on the CPU.

With secure aggregation (``EngineConfig.secagg``, ``fedmi/fl/secagg.py``) the k buffers are
quantised and pair-masked before they are summed: one ``fl_secagg_mask`` launch over the k buffers
and one ``fl_secagg_open`` launch in place on the device, the host model on the CPU.  The ``wire``
hook sees the buffers between the two -- what a peer would receive.

With an attack model (``EngineConfig.attack``, ``fedmi/fl/attack.py``) the Byzantine clients' buffers are
rewritten after the ``tamper`` hook and before all of the above: one ``fl_attack`` launch in place over the
k buffers on the device, ``attack_torch`` on the CPU; ``"label_flip"`` flips the bad clients' shard labels
instead.  The launched kinds make every client start from one common model.
"""
from __future__ import annotations

import copy
import os
from typing import Callable, List, Optional

import numpy as np
import torch

from ..data.sharding import shard_indices
from ..models.mlp import init_flat
from .aggregate import _AggLaunch
from .attack import attack_id, flip_labels
from .engine import EngineConfig, HipRoundEngine, TorchRoundEngine, common_init, gather_plane_id, heldout_metrics


class SimRank:
    """Stand-in communicator of one simulated client: rank / size / device only.  The
    collective is performed by :class:`ClientGroup`."""

    peer_allreduce = False
    native = None
    in_process = True   # the group holds every client's contribution: the attack stage runs whatever the rule

    def __init__(self, size: int, rank: int, device):
        self.size, self.rank, self.device = int(size), int(rank), torch.device(device)

    def Barrier(self) -> None:  # the group's clients run in program order
        pass


class ClientGroup:
    """k clients of one federation in this process."""

    def __init__(self, X, y, k: int, cfg: EngineConfig, backend: str = "hip", shard_mode: str = "compat",
                 seed: int = 0, alpha: float = 0.5, device=None, n_classes: Optional[int] = None,
                 tamper: Optional[Callable[[int, List[torch.Tensor]], None]] = None,
                 wire: Optional[Callable[[int, List[torch.Tensor]], None]] = None,
                 heldout=None, keep_best: bool = False):
        """``heldout=(X, y)``: the lead client scores the round's global model on these rows after the
        aggregation and the server steps of every round (``set_heldout``): :meth:`history` carries the
        held-out keys, ``keep_best`` keeps the best round's model for :meth:`best_flat`.
        ``tamper(r, bufs)``: optional hook for Byzantine-client studies, called every round after the
        local steps and before the aggregation with the round index and the k clients' contribution
        buffers in client order (hip: the device FedAvg buffers, on the group's stream, the padded
        parameter image first; torch: the ``fedavg_contribution`` rows, the dense parameters first);
        what it writes is what gets aggregated.  ``None`` changes nothing.
        ``wire(r, bufs)``: optional hook called with the same arguments after the secure-aggregation mask
        step (``EngineConfig.secagg``) and before the sum is opened: what a peer sees on the wire (tamper
        sees the clear contributions).  Not called without secure aggregation."""
        X = np.asarray(X)
        y = np.asarray(y)
        self.k = int(k)
        self.backend = backend
        n_classes = int(n_classes if n_classes is not None else len(np.unique(y)))
        idx = [shard_indices(len(X), r, self.k, mode=shard_mode, seed=seed, labels=y, alpha=alpha)
               for r in range(self.k)]
        n_total = int(sum(len(i) for i in idx))
        dims = [int(X.shape[1]), *[int(h) for h in cfg.hidden], n_classes]
        if backend == "hip":
            self.device = torch.device(device if device is not None else "cuda")
        else:
            self.device = torch.device("cpu")
        if bool(cfg.secagg) and cfg.secagg_seed is None:
            # one mask seed for the group (config only: no result depends on it)
            cfg = copy.deepcopy(cfg)
            cfg.secagg_seed = int.from_bytes(os.urandom(8), "little")
        # Byzantine attack model: validated against the group's size; "label_flip" poisons the bad clients' shards
        flipped = set(int(b) for b in cfg.attack_clients) if (attack_id(cfg, self.k) and cfg.attack == "label_flip") else ()
        self.clients: List = []
        for r in range(self.k):
            c = copy.deepcopy(cfg)
            if backend == "hip":
                c.lagged_eval = False    # classic rounds: each client evaluates itself
                c.graph_rounds = 0
                gather_plane_id(c)       # (validated; the group aggregates in place over its clients' buffers)
                c.gather_plane = "host"
            comm = SimRank(self.k, r, self.device)
            # FederatedMLPLearning's seeding: one init stream per (seed, rank)
            # (server optimizer, attack stage: one common starting model, see FederatedMLPLearning)
            flat0 = init_flat(dims, seed * 1000003 + (0 if common_init(cfg) else r))
            y_r = flip_labels(y[idx[r]], n_classes) if r in flipped else y[idx[r]]
            if backend == "hip":
                e = HipRoundEngine(X[idx[r]], y_r, n_classes, c, comm, flat0, n_total=n_total,
                                   device=self.device, client_sizes=[len(i) for i in idx])
            elif backend == "torch":
                e = TorchRoundEngine(X[idx[r]], y_r, n_classes, c, comm, flat0, n_total=n_total,
                                     client_sizes=[len(i) for i in idx])
            else:
                raise ValueError(f"unknown backend {backend!r}")
            self.clients.append(e)
        self.tamper = tamper
        self.wire = wire
        if self.clients[0].screen:
            # one kept-mask history for the group (the lead's launches / rule write it): every client reports it
            lead = self.clients[0]
            for e in self.clients[1:]:
                if backend == "hip":
                    e.screen_hist = lead.screen_hist
                else:
                    e.hist.screen = lead.hist.screen
        if backend == "hip":
            lead = self.clients[0]
            if lead.robust or lead.secagg or lead.attack_stage:   # in place over the k clients' buffers, client r = buffer r
                bufs = [[e.params[q] for e in self.clients] for q in (0, 1)]
                self._agg = _AggLaunch(lead, bufs, bufs, clamps=[e.sa_clamp for e in self.clients] if lead.secagg else ())
            self.stream = torch.cuda.Stream(device=self.device)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            for e in self.clients:
                e.stream = self.stream   # one stream: every client's kernels and the sums in order
        if heldout is not None:
            Xv, yv = heldout
            self.clients[0].set_heldout(Xv, yv, keep_best=keep_best)   # only the lead holds the set
        self.rounds = 0

    # ---- rounds ----
    def _round_hip(self, r: int) -> None:
        s = self.stream.cuda_stream
        for e in self.clients:
            e.engine.run_local(r, s)      # train + Adam + eval into its own FedAvg buffer
        lead = self.clients[0]
        par = (r + 1) & 1
        bufs = [e.params[par] for e in self.clients]
        if self.tamper is not None:
            with torch.cuda.stream(self.stream):
                self.tamper(r, bufs)
        if lead.attack_stage:
            # Byzantine attack model: one launch rewrites the bad sampled clients' buffers in place
            self._agg.attack(par, s)
        if lead.robust:
            # one launch, in place: every client's buffer is a source and a destination; the round's
            # live flag, index and sampled mask are the lead client's (identical on all)
            self._agg.robust(par, s)
        elif lead.secagg:
            # one mask launch over the k buffers, the wire hook, one open launch in place
            self._agg.mask(par, s)
            if self.wire is not None:
                with torch.cuda.stream(self.stream):
                    self.wire(r, bufs)
            self._agg.open(par, s)
        else:
            self._sum_hip(bufs)
        for e in self.clients:
            e.server_step(r)              # server optimizer: every client steps its replica of the sum
            e.rounds_issued = r + 1
        lead.heldout_step(r)              # held-out row of the round's finished global image (lead only)

    def _sum_hip(self, bufs) -> None:
        with torch.cuda.stream(self.stream):
            tot = getattr(self, "_tot", None)
            if tot is None or tot.shape != bufs[0].shape:
                tot = self._tot = torch.empty_like(bufs[0])   # one accumulation buffer for all rounds
            tot.copy_(bufs[0])
            for b in bufs[1:]:
                tot += b                  # rank order
            for b in bufs:
                b.copy_(tot)

    def _round_torch(self) -> None:
        for e in self.clients:
            e.step_train()
            e.step_eval()
        bufs = [e.fedavg_contribution() for e in self.clients]
        if self.tamper is not None:
            self.tamper(self.rounds, bufs)
        self.clients[0].attack_rows(bufs)   # Byzantine attack model (nothing when off)
        if self.clients[0].robust:
            tot = self.clients[0].robust_combine(bufs)
        elif self.clients[0].secagg:
            for e, b in zip(self.clients, bufs):
                e.secagg_mask_(b)
            if self.wire is not None:
                self.wire(self.rounds, bufs)
            tot = self.clients[0].secagg_combine(bufs)
        else:
            tot = bufs[0].clone()
            for b in bufs[1:]:
                tot += b
        for e in self.clients:
            e.fedavg_apply(tot.clone())

    @property
    def stopped(self) -> bool:
        return bool(self.clients[0].stopped)

    def run(self, n_rounds: int, check_every: int = 32) -> int:
        lead = self.clients[0]
        before = self.rounds
        left = min(n_rounds, lead.cfg.max_rounds - self.rounds)
        while left > 0 and not self.stopped:
            n = min(left, check_every)
            for _ in range(n):
                if self.backend == "hip":
                    self._round_hip(self.rounds)
                else:
                    if self.stopped:
                        break
                    self._round_torch()
                self.rounds += 1
            left -= n
            if self.backend == "hip":
                st = lead._read_state(self.rounds & 1)
                if st["stopped"]:
                    lead._stopped_seen = True
        self.sync_history()
        return self.rounds - before

    def sync_history(self) -> None:
        if self.backend == "hip":
            for e in self.clients:
                e.sync_history()

    def history(self) -> dict:
        return self.clients[0].history()

    def global_flat(self) -> np.ndarray:
        return self.clients[0].global_flat()

    def best_flat(self) -> np.ndarray:
        """Dense weights of the round with the smallest held-out loss (``heldout=..., keep_best=True``)."""
        return self.clients[0].best_flat()


def rounds_to_target(X, y, k: int, cfg: EngineConfig, backend: str = "hip", seed: int = 0,
                     targets=(0.80, 0.83), shard_mode: str = "compat", heldout=None) -> dict:
    """Reference-compat convergence of k clients: first round reaching each global-accuracy
    target, the early-stop round and the final accuracy.  ``heldout=(X, y)``: the
    targets and ``final_acc`` are read from the global model's accuracy on these rows instead of the
    mean of the clients' local training accuracies, and the result's ``"metric"`` says so
    (``"heldout_accuracy"``); without it the result is what it always was."""
    g = ClientGroup(X, y, k, cfg, backend=backend, shard_mode=shard_mode, seed=seed, heldout=heldout)
    g.run(cfg.max_rounds)
    h = g.history()
    acc = h["global"][:, 0] if heldout is None else heldout_metrics(h)[:, 0]
    out = {}
    for t in targets:
        hit = np.flatnonzero(acc >= t)
        out[f"{t:.2f}"] = int(hit[0]) + 1 if len(hit) else None
    out["early_stop_round"] = int(h["stop_round"]) if h["stop_round"] >= 0 else None
    out["final_acc"] = float(acc[-1]) if len(acc) else None
    out["rounds_run"] = int(h["rounds_run"])
    if heldout is not None:
        out["metric"] = "heldout_accuracy"
    return out

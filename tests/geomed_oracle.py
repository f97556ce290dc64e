"""Shared pieces of the geometric-median tests (tests/test_geomed_cpu.py, tests/test_geomed.py): the
float64 group oracle and the tamper hooks that work on every backend's contribution buffers."""
import warnings

import numpy as np
import torch

from fedmi.fl.aggregate import geomed_torch

from .reference_oracle import Float64RoundOracle
from .server_oracle import server_step_f64


def tamper_two(n, nan_client=1, big_client=4):
    """``ClientGroup(tamper=...)``: every round client ``nan_client`` publishes NaN and client ``big_client``
    ``1e12 * sign(its model)`` over the first ``n`` floats of their buffers (the padded image of a hip group,
    the dense parameters of a torch group or of the float64 oracle; ``sign(0) = 0`` keeps image padding 0)
    -- never the tails."""
    def tamper(r, bufs):
        bufs[nan_client][:n] = float("nan")
        bufs[big_client][:n] = 1e12 * torch.sign(bufs[big_client][:n])
    return tamper


class Float64GeomedGroupOracle:
    """The arithmetic of ``ClientGroup(backend="torch")`` with ``aggregator="geomed"`` in float64: every
    client starts round 0 from its own model and later rounds from the global one; the sampled clients
    train; ``tamper(r, rows)`` rewrites their float64 models; ``geomed_torch`` aggregates them in float64;
    an optional server step follows."""

    def __init__(self, shards, n_classes, cfg, flats, participants, tamper=None):
        self.cfg, self.participants, self.tamper = cfg, participants, tamper
        self.clients = [Float64RoundOracle(X, y, n_classes, cfg, f) for (X, y), f in zip(shards, flats)]
        self.x = None
        P = self.clients[0].weights().size
        self.sm = np.zeros(P)
        self.sv = None if cfg.server_opt in ("none", "sgd") else np.full(P, float(cfg.server_tau) ** 2)
        self.rounds = 0

    @staticmethod
    def _set(o, flat):
        off = 0
        with torch.no_grad():
            for p in o.params:
                p.copy_(torch.as_tensor(flat[off:off + p.numel()]).view_as(p))
                off += p.numel()

    def run(self, n):
        for _ in range(n):
            part = [int(k) for k in self.participants(self.rounds)]
            x = self.x if self.x is not None else self.clients[0].weights().copy()
            for k, o in enumerate(self.clients):
                if self.x is not None:
                    self._set(o, self.x)
                if k in part:
                    o.run(1)
                else:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore", UserWarning)
                        o.scheduler.step()
            rows = [torch.as_tensor(o.weights().copy()) for o in self.clients]
            if self.tamper is not None:
                self.tamper(self.rounds, rows)
            a = geomed_torch(torch.stack(rows), [k in part for k in range(len(self.clients))],
                             int(self.cfg.geomed_iters), float(self.cfg.geomed_nu)).numpy()
            if self.cfg.server_opt != "none":
                a, self.sm, self.sv = server_step_f64(x, a, self.sm, self.sv, self.cfg)
            self.x = a
            self.rounds += 1

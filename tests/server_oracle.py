"""Shared pieces of the server-optimizer tests (tests/test_server_opt_cpu.py, tests/test_server_opt.py):
the float64 model of one server step, a float64 round oracle that applies it after every round, and
the cases.

Shapes: ``income`` = make_multiclass(300, 14, 2) with 14-50-200-2 and ``small`` = make_multiclass(96,
17, 3) with 17-24-3: K = 14, 17, 50, 200 (none a multiple of 16, 17 odd), N = 2 and 3, rows of both
swizzle parities.  Server settings: FedAvgM at lr 1, momentum 0.9; the adaptive optimizers at lr 1e-2
(the middle of Reddi et al.'s grid), tau 1e-3, b1 0.9, b2 0.99.
"""
import warnings

import numpy as np
import torch

from fedmi.fl.engine import SERVER_OPTS, EngineConfig

from .reference_oracle import DATA_SEED, INIT_SEED, Float64RoundOracle, make_multiclass

SERVER_ROUNDS = 6
OPTS = ("sgd", "adagrad", "adam", "yogi")
# name -> (rows, F, C, hidden)
SERVER_SHAPES = {"income": (300, 14, 2, (50, 200)), "small": (96, 17, 3, (24,))}
SERVER_KW = {
    "sgd": dict(server_opt="sgd", server_lr=1.0, server_momentum=0.9),
    "adagrad": dict(server_opt="adagrad", server_lr=1e-2, server_tau=1e-3),
    "adam": dict(server_opt="adam", server_lr=1e-2, server_tau=1e-3),
    "yogi": dict(server_opt="yogi", server_lr=1e-2, server_tau=1e-3),
}


def server_cfg(opt, shape="income", **kw):
    hidden = SERVER_SHAPES[shape][3]
    base = dict(hidden=hidden, max_rounds=SERVER_ROUNDS + 2, early_stop=False, graph_rounds=0)
    return EngineConfig(**{**base, **SERVER_KW[opt], **kw})


def shape_data(shape):
    rows, F, C, hidden = SERVER_SHAPES[shape]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    from fedmi.models.mlp import init_flat
    return X, y, C, init_flat([F, *hidden, C], INIT_SEED)


def server_scalars(cfg, fp32=False):
    """(lr, b1, 1 - b1, b2, 1 - b2, tau) as doubles; ``fp32``: the values the HIP kernel is handed
    (each rounded to fp32 once, 1 - b formed in double first)."""
    b1, b2 = float(cfg.server_momentum), float(cfg.server_beta2)
    s = (float(cfg.server_lr), b1, 1.0 - b1, b2, 1.0 - b2, float(cfg.server_tau))
    return tuple(float(np.float32(t)) for t in s) if fp32 else s


def server_step_f64(x, a, m, v, cfg, fp32_scalars=False):
    """float64 model of one server step: (new global, m', v') from the image the round trained from
    ``x``, the aggregated image ``a`` and the state.  ``v`` / v' are None for ``sgd``."""
    kind = SERVER_OPTS.index(cfg.server_opt)
    assert kind >= 1
    lr, b1, omb1, b2, omb2, tau = server_scalars(cfg, fp32_scalars)
    x, a, m = (np.asarray(t, np.float64) for t in (x, a, m))
    d = a - x
    if kind == 1:
        m = b1 * m + d
        return x + lr * m, m, None
    v = np.asarray(v, np.float64)
    m = b1 * m + omb1 * d
    d2 = d * d
    if kind == 2:
        v = v + d2
    elif kind == 3:
        v = b2 * v + omb2 * d2
    else:
        v = v - omb2 * d2 * np.sign(v - d2)
    return x + lr * m / (np.sqrt(v) + tau), m, v


class Float64ServerOracle(Float64RoundOracle):
    """One client's rounds in float64 with a server optimizer: FedAvg of one client is the identity,
    so the round's aggregated image is the post-step local model; the server step's output replaces
    it as the next round's input.  The client's Adam moments persist."""

    def __init__(self, X, y, n_classes, cfg, init_flat):
        super().__init__(X, y, n_classes, cfg, init_flat)
        P = self.weights().size
        self.server_m = np.zeros(P)
        self.server_v = None if cfg.server_opt == "sgd" else np.full(P, float(cfg.server_tau) ** 2)
        self.dmax = 0.0   # largest |pseudo-gradient component| seen

    def run(self, n_rounds):
        for _ in range(n_rounds):
            x = self.weights().copy()
            super().run(1)
            self.dmax = max(self.dmax, float(np.abs(self.weights() - x).max()))
            new, self.server_m, self.server_v = server_step_f64(x, self.weights(), self.server_m, self.server_v,
                                                                self.cfg)
            off = 0
            with torch.no_grad():
                for p in self.params:
                    p.copy_(torch.as_tensor(new[off:off + p.numel()]).view_as(p))
                    off += p.numel()


class Float64GroupOracle:
    """k clients of one federation in float64 (the arithmetic of ClientGroup(backend="torch")): every
    client starts a round from the global model, the round's sampled clients (``participants(r)`` of
    an engine of the group) train, their models are averaged with weights n_i / (sampled total), and
    the server step of that average from the round's input is the next global model.  A client that
    sits a round out only steps its LR schedule."""

    def __init__(self, shards, n_classes, cfg, init_flat, participants):
        self.cfg = cfg
        self.clients = [Float64RoundOracle(X, y, n_classes, cfg, init_flat) for X, y in shards]
        self.sizes = [len(y) for _, y in shards]
        self.participants = participants
        self.x = np.asarray(init_flat, np.float64)
        self.server_m = np.zeros(self.x.size)
        self.server_v = None if cfg.server_opt == "sgd" else np.full(self.x.size, float(cfg.server_tau) ** 2)
        self.rounds = 0

    @staticmethod
    def _set(o, flat):
        off = 0
        with torch.no_grad():
            for p in o.params:
                p.copy_(torch.as_tensor(flat[off:off + p.numel()]).view_as(p))
                off += p.numel()

    def run(self, n_rounds):
        for _ in range(n_rounds):
            part = [int(k) for k in self.participants(self.rounds)]
            tot = float(sum(self.sizes[k] for k in part))
            a = np.zeros_like(self.x)
            for k, o in enumerate(self.clients):
                self._set(o, self.x)
                if k in part:
                    o.run(1)
                    a += o.weights() * (self.sizes[k] / tot)
                else:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore", UserWarning)   # "scheduler.step() before optimizer.step()"
                        o.scheduler.step()
            self.x, self.server_m, self.server_v = server_step_f64(self.x, a, self.server_m, self.server_v, self.cfg)
            self.rounds += 1

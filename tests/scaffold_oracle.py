"""The SCAFFOLD tests' shapes, group factory and float64 group oracle: ``scaffold_fold`` on float64 tensors around
``Float64GroupOracle``, whose clients' gradients take the correction through tensor hooks."""
import copy

import torch

from fedmi.fl.engine import EngineConfig
from fedmi.fl.scaffold import scaffold_fold
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, make_multiclass
from .server_oracle import Float64GroupOracle

# name -> (features, classes, hidden): P = 507 (no multiple of 4 or 64) and the income shape
SCAFFOLD_SHAPES = {"small": (17, 3, (24,)), "income": (14, 2, (50, 200))}


def scaffold_group(backend, shape, local_steps=3, participation=1.0, **kw):
    """Four label-skew clients (alpha 0.3) on 1200 seeded rows, clients' Adam eps 1e-4, no early stop."""
    F, C, hidden = SCAFFOLD_SHAPES[shape]
    cfg = EngineConfig(**{**dict(hidden=hidden, max_rounds=8, early_stop=False, graph_rounds=0, eps=1e-4, seed=3,
                                 local_steps=local_steps, participation=participation, scaffold=True), **kw})
    return ClientGroup(*make_multiclass(1200, F, C, DATA_SEED), 4, cfg, backend=backend, shard_mode="label_skew",
                       alpha=0.3, seed=2, n_classes=C)


def _hook(cl):
    """Every gradient of the oracle client ``cl`` gains ``cl.corr`` (before the FedProx term, which its round adds to
    ``.grad`` afterwards); the round's first raw gradients are kept in ``cl.g0``."""
    cl.corr, cl.g0, off = None, {}, 0
    for i, p in enumerate(cl.params):
        def hook(g, i=i, lo=off, p=p):
            cl.g0.setdefault(i, g.detach().reshape(-1).clone())
            return g + cl.corr[lo:lo + p.numel()].view_as(p)
        p.register_hook(hook)
        off += p.numel()


def scaffold_group_f64(tg, shape, rounds):
    """(weights, c, [c_i]) of the torch group ``tg``'s float64 oracle after ``rounds`` rounds."""
    F, C, hidden = SCAFFOLD_SHAPES[shape]
    lead = tg.clients[0]
    cfg = copy.deepcopy(lead.cfg)
    if cfg.server_opt == "none":   # (the group oracle always steps: x + 1 (a - x) is a to float64 rounding)
        cfg.server_opt, cfg.server_lr, cfg.server_momentum = "sgd", 1.0, 0.0
    o = Float64GroupOracle([(e.X.numpy(), e.y.numpy()) for e in tg.clients], C, cfg,
                           init_flat([F, *hidden, C], 2 * 1000003), lead.participants)
    K = len(o.clients)
    c = torch.zeros(o.x.size, dtype=torch.float64)
    ci = [c.clone() for _ in range(K)]
    for cl in o.clients:
        _hook(cl)
    for r in range(rounds):
        part = [int(k) for k in lead.participants(r)]
        for k, cl in enumerate(o.clients):
            cl.corr = c - ci[k]
            cl.g0.clear()
        o.run(1)
        deltas = [torch.cat([cl.g0[i] for i in range(len(cl.params))]) - ci[k] if k in part else c
                  for k, cl in enumerate(o.clients)]
        c = scaffold_fold(c, deltas, [k in part for k in range(K)], K)
        for k in part:
            ci[k] = ci[k] + deltas[k]
    return o.x, c.numpy(), [x.numpy() for x in ci]

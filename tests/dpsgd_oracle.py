"""float64 oracle of record-level DP-SGD (``EngineConfig.dpsgd_clip`` / ``dpsgd_noise``): per-example
gradients from an explicit per-row autograd loop -- no ghost formula, nothing shared with the code under
test but the Philox noise model."""
import numpy as np
import torch
from torch import nn

from fedmi.privacy.philox import dpsgd_normals

from .reference_oracle import Float64RoundOracle, _dense_layers

DPSGD_SHAPES = [(14, 50, 200, 2), (17, 24, 3), (11, 20, 36, 18, 4)]


def row_grads_f64(flat, dims, X, y):
    """``(G [n, P], ce [n])``: every row's own gradient of its own cross-entropy (dense order), float64."""
    params = [t.requires_grad_() for Wb in _dense_layers(flat, list(dims)) for t in Wb]
    Xt = torch.as_tensor(np.asarray(X, np.float32)).to(torch.float64)
    yt = torch.as_tensor(np.asarray(y), dtype=torch.long)
    G, ce = [], []
    for r in range(len(Xt)):
        a = Xt[r:r + 1]
        for l in range(0, len(params), 2):
            a = a @ params[l].T + params[l + 1]
            if l + 2 < len(params):
                a = torch.relu(a)
        loss = nn.functional.cross_entropy(a, yt[r:r + 1])
        g = torch.autograd.grad(loss, params)
        G.append(torch.cat([t.reshape(-1) for t in g]).numpy())
        ce.append(float(loss))
    return np.stack(G), np.asarray(ce)


def clipped_sum(G, C, n):
    """sum_r min(1, C / ||g_r||) g_r / n over the rows of ``G``."""
    norms = np.sqrt((G * G).sum(1))
    return (G * np.minimum(1.0, C / norms)[:, None]).sum(0) / n


class Float64DpSgdOracle(Float64RoundOracle):
    """One client's DP-Adam rounds in float64: every local step's gradient is the clipped per-row sum over n
    plus z C / n times the engines' noise stream of (round, step, rank 0); FedProx and weight decay after it."""

    def __init__(self, X, y, n_classes, cfg, init_flat, seed):
        super().__init__(X, y, n_classes, cfg, init_flat)
        self.seed, self.Xn, self.yn = int(seed), np.asarray(X, np.float32), np.asarray(y)

    def run(self, n_rounds):
        cfg = self.cfg
        C, z, n = float(cfg.dpsgd_clip), float(cfg.dpsgd_noise), len(self.Xn)
        for _ in range(n_rounds):
            r = len(self.loss)
            anchor = [p.detach().clone() for p in self.params]
            for ls in range(cfg.local_steps):
                G, ce = row_grads_f64(self.weights(), self.dims, self.Xn, self.yn)
                g = clipped_sum(G, C, n)
                if z:
                    g = g + z * C / n * dpsgd_normals(g.size, r, ls, 0, self.seed)
                off = 0
                for p, a in zip(self.params, anchor):
                    p.grad = torch.as_tensor(g[off:off + p.numel()]).view_as(p).clone()
                    if cfg.prox_mu:
                        p.grad.add_(cfg.prox_mu * (p.detach() - a))
                    off += p.numel()
                self.optimizer.step()
            self.scheduler.step()
            self.loss.append(float(ce.mean()))

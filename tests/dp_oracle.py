"""Shared pieces of the differential-privacy tests (tests/test_dp_cpu.py, tests/test_dp_fedavg.py):
the end-to-end cases, the float64 host model of one contribution, and a float64 DP round oracle.

Clipping bounds.  Each case's S sits between the update norms the fp32 torch oracle records in the
six measured rounds, at least 1 % away from every one of them, with at least two rounds clipped and
two not (``assert_clip_decisions``): a rounding difference between two implementations then cannot
flip a clip decision, and no case passes with clipping always or never active.  Norms of the fp32
oracle (data seed 3, init seed 1), clipping only / z = 0.02:

    income   300x14x2, 50-200         S = 0.37    z = 0     0.4242 0.3853 0.3627 0.3500 0.3440 0.3413
                                                  z = 0.02  0.4242 0.3757 0.3570 0.3440 0.3386 0.3346
    steps2   the same, local_steps 2  S = 0.70    z = 0     0.7880 0.7115 0.6868 0.6766 0.6546 0.6134
                                      S = 0.685   z = 0.02  0.7880 0.6935 0.6717 0.6580 0.6231 0.5836
    small    96x17x3, 24              S = 0.0863  z = 0     0.0901 0.0875 0.0851 0.0839 0.0830 0.0822
                                                  z = 0.02  0.0901 0.0874 0.0850 0.0841 0.0833 0.0825

(steps2's norms fall by about 1 % per round around the bound and the noise shifts them by more
than that, so its bound is chosen per noise multiplier.)
"""
import numpy as np
import torch

from fedmi.privacy.philox import dp_normals

from .reference_oracle import Float64RoundOracle

DP_ROUNDS = 6
DP_SEED = 20240607
DP_Z = 0.02
# name -> (rows, F, C, hidden, {noise multiplier: S}, extra EngineConfig fields)
DP_CASES = {
    "income": (300, 14, 2, (50, 200), {0.0: 0.37, DP_Z: 0.37}, {}),
    "steps2": (300, 14, 2, (50, 200), {0.0: 0.70, DP_Z: 0.685}, {"local_steps": 2}),
    "small": (96, 17, 3, (24,), {0.0: 0.0863, DP_Z: 0.0863}, {}),
}


def assert_clip_decisions(norms, S):
    """>= 2 rounds clipped, >= 2 not, none within 1 % of S (on the ORACLE's recorded norms)."""
    norms = np.asarray(norms, np.float64)
    assert (norms > S).sum() >= 2, (norms, S)
    assert (norms < S).sum() >= 2, (norms, S)
    assert np.min(np.abs(norms - S)) >= 0.01 * S, (norms, S)


def contribution_f64(local, x, w, S, sigma, normals):
    """float64 model of one client's contribution: (w (x + c D) + sigma n, ||D||, c) from the fp32
    local model and round input (exact in float64), c = min(1, S / ||D||)."""
    local = np.asarray(local, np.float64)
    x = np.asarray(x, np.float64)
    delta = local - x
    norm = float(np.sqrt(np.sum(delta * delta)))
    c = min(1.0, S / norm) if norm > 0.0 else 1.0
    out = w * (x + c * delta)
    if normals is not None:
        out = out + sigma * np.asarray(normals, np.float64)
    return out, norm, c


class Float64DPOracle(Float64RoundOracle):
    """One client's DP rounds in float64 (world 1: w = 1, K = 1, so sigma = z S, taken at the fp32
    value both engines use): the round's output x + c D + sigma n replaces the local model as the
    next round's input; the Adam moments persist.  The noise is the engines' Philox stream."""

    def __init__(self, X, y, n_classes, cfg, init_flat, seed):
        super().__init__(X, y, n_classes, cfg, init_flat)
        self.seed = int(seed)
        self.norms = []

    def run(self, n_rounds):
        cfg = self.cfg
        S = float(cfg.dp_clip)
        sigma = float(np.float32(float(cfg.dp_noise) * S))
        for _ in range(n_rounds):
            r = len(self.loss)
            x = self.weights().copy()
            super().run(1)
            P = x.size
            nrm = dp_normals(P, r, 0, self.seed) if cfg.dp_noise else None
            out, norm, _ = contribution_f64(self.weights(), x, 1.0, S, sigma, nrm)
            self.norms.append(norm)
            off = 0
            with torch.no_grad():
                for p in self.params:
                    p.copy_(torch.as_tensor(out[off:off + p.numel()]).view_as(p))
                    off += p.numel()

"""Privacy accounting of DP-FedAvg rounds (``EngineConfig.dp_clip`` / ``dp_noise``).

Each round is one Gaussian mechanism on the weighted sum of the clients' clipped updates: the
sum changes by at most ``S * max_j w_j`` in L2 norm when one client's data changes, and the
clients' noise shares add up to a Gaussian of standard deviation ``z`` times that sensitivity.
The Renyi divergence of order ``alpha`` of such a mechanism is ``alpha / (2 z^2)`` (Mironov,
"Renyi differential privacy", 2017); it adds over the ``T`` rounds, and RDP converts to

    eps(delta) = min over alpha > 1 of [ T * alpha / (2 z^2) + ln(1 / delta) / (alpha - 1) ]
               = T / (2 z^2) + sqrt(2 T ln(1 / delta)) / z      (alpha* = 1 + z sqrt(2 ln(1/delta) / T)).

What the figure does and does not say:

* **Client-level.**  Two federations are neighbours when they differ in ONE client's whole
  shard; nothing is claimed per row.
* **Shard sizes are public.**  The FedAvg weights ``n_i / N`` depend on them, and the noise scale
  is calibrated to ``max_j w_j``.
* **No subsampling amplification.**  Under ``participation < 1`` every round is counted as if the
  client had taken part in it.  The un-amplified figure is a valid upper bound on the privacy
  loss (a client that sits a round out loses nothing in it), just not the tightest one.
* The noise is distributed: each client adds its ``1 / sqrt(K)`` share before the exchange, so
  the guarantee holds for the aggregate and everything computed from it; a single peer's own
  contribution carries only its share.
"""
from __future__ import annotations

import math

import numpy as np


def _check(noise_multiplier: float, rounds: int, delta: float) -> None:
    if not (0.0 < float(delta) < 1.0):
        raise ValueError(f"delta must be in (0, 1), got {delta!r}")
    if int(rounds) < 0:
        raise ValueError(f"rounds must be >= 0, got {rounds!r}")
    if float(noise_multiplier) < 0.0:
        raise ValueError(f"noise multiplier must be >= 0, got {noise_multiplier!r}")


def gaussian_rdp(noise_multiplier: float, alpha) -> np.ndarray:
    """Renyi divergence of order ``alpha`` of one round: ``alpha / (2 z^2)``."""
    return np.asarray(alpha, np.float64) / (2.0 * float(noise_multiplier) ** 2)


def epsilon_closed_form(noise_multiplier: float, rounds: int, delta: float) -> float:
    """``T / (2 z^2) + sqrt(2 T ln(1/delta)) / z``; ``inf`` without noise, 0 without rounds."""
    _check(noise_multiplier, rounds, delta)
    z, T = float(noise_multiplier), int(rounds)
    if T == 0:
        return 0.0
    if z == 0.0:
        return math.inf
    return T / (2.0 * z * z) + math.sqrt(2.0 * T * math.log(1.0 / float(delta))) / z


def epsilon_rdp(noise_multiplier: float, rounds: int, delta: float, alphas=None) -> float:
    """The same bound as a minimum over a grid of Renyi orders (default: 1 + a geometric grid
    from 1e-4 to 1e4, 20001 points); never below :func:`epsilon_closed_form`."""
    _check(noise_multiplier, rounds, delta)
    z, T = float(noise_multiplier), int(rounds)
    if T == 0:
        return 0.0
    if z == 0.0:
        return math.inf
    a = 1.0 + np.geomspace(1e-4, 1e4, 20001) if alphas is None else np.asarray(alphas, np.float64)
    if np.any(a <= 1.0):
        raise ValueError("Renyi orders must be > 1")
    return float(np.min(T * gaussian_rdp(z, a) + math.log(1.0 / float(delta)) / (a - 1.0)))


def privacy_statement(noise_multiplier: float, rounds: int, delta: float) -> str:
    """One line for the end of a run (the [C] entry point prints it on rank 0)."""
    eps = epsilon_closed_form(noise_multiplier, rounds, delta)
    return (f"Differential privacy: epsilon = {eps:.4g} at delta = {float(delta):g} over {int(rounds)} rounds "
            f"(noise multiplier {float(noise_multiplier):g}; client-level, no subsampling amplification)")

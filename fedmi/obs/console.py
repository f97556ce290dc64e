"""Reference-format console output and JSONL metric streams.

The reference prints, per round, ``Round r:`` then every rank's local metrics in rank
order (forced by 2*k barriers, C:151-162), then ``Global Metrics`` on rank 0 (C:172-179)
and the early-stop messages (C:135, C:188).  Users parse those lines, so the format is
kept byte-for-byte; but here rank 0 prints *all* ranks' lines from the device-side
metric history (the all-reduced per-rank confusion matrices), so printing costs no
collectives and no barriers.
"""
from __future__ import annotations

import json
import time
from typing import IO, Optional

import numpy as np

from ..fl.metrics import METRIC_NAMES


def _fmt(v) -> str:
    return (f"[accuracy: {v[0]:.4f}, precision: {v[1]:.4f}, "
            f"recall: {v[2]:.4f}, f1: {v[3]:.4f}]")


def format_round(r: int, per_rank: np.ndarray, glob: np.ndarray) -> str:
    lines = [f"\nRound {r + 1}:\n"]
    for k in range(per_rank.shape[0]):
        lines.append(f"  RANK {k} - Local Metrics (Round {r + 1}): {_fmt(per_rank[k])}")
    lines.append(f"  Global Metrics (Round {r + 1}): {_fmt(glob)}")
    return "\n".join(lines)


def print_history(hist: dict, patience: int, start: int = 0, out: Optional[IO] = None,
                  print_fn=print) -> int:
    """Print rounds [start, rounds_run) of an engine history in the reference format;
    returns the next round to print."""
    n = hist["rounds_run"]
    for r in range(start, n):
        print_fn(format_round(r, hist["per_rank"][r], hist["global"][r]), flush=True)
        if hist.get("stop_trigger", -1) == r:
            print_fn(f"Early stopping triggered: No significant change in metrics for {patience} rounds.",
                     flush=True)
    if hist.get("stop_round", -1) >= 0 and n == hist["stop_round"] and start <= n:
        print_fn(f"Training stopped early at round {hist['stop_round']}.", flush=True)
    return n


class JsonlWriter:
    """One JSON object per line (round metrics, timings, bench results)."""

    def __init__(self, path: Optional[str]):
        self.f = open(path, "a") if path else None

    def write(self, **rec) -> None:
        if self.f is None:
            return
        rec.setdefault("ts", time.time())
        self.f.write(json.dumps(rec, default=_default) + "\n")
        self.f.flush()

    def history(self, hist: dict, **extra) -> None:
        for r in range(hist["rounds_run"]):
            # (DP engines: this client's pre-clip update norm of the round, 0 when not sampled)
            norm = {"update_norm": float(hist["update_norm"][r])} if "update_norm" in hist else {}
            # (compressing engines: the round's statistic -- k-th kept magnitude / sign scale / qsgd norm / rand-k quantile)
            if "compress_stat" in hist:
                norm["compress_stat"] = float(hist["compress_stat"][r])
            # (secure aggregation: this client's clamped / NaN coordinates of the round)
            if "secagg_clamped" in hist:
                norm["secagg_clamped"] = int(hist["secagg_clamped"][r])
            # (held-out scoring: the round's global model on the held-out set)
            if "heldout_cm" in hist:
                from ..fl.metrics import metrics_from_confusion
                ho = metrics_from_confusion(hist["heldout_cm"][r])
                norm.update({f"heldout_{k}": float(ho[k]) for k in METRIC_NAMES})
                norm["heldout_loss"] = float(hist["heldout_loss"][r])
            self.write(round=r + 1, **{k: float(hist["global"][r][i]) for i, k in enumerate(METRIC_NAMES)},
                       per_rank=hist["per_rank"][r].tolist(), loss=float(hist["loss"][r]), **norm, **extra)

    def close(self) -> None:
        if self.f is not None:
            self.f.close()
            self.f = None


def _default(o):
    if isinstance(o, np.ndarray):
        return o.tolist()
    if isinstance(o, (np.floating, np.integer)):
        return o.item()
    raise TypeError(type(o))

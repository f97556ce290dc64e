"""Float64 host models of the bf16 kernels' forward pass, and evaluation shards planted with the
rows on which the split-bf16 forward and a plain bf16 one disagree.

The bf16 engine scores with z = a_hi.W_hi + (a_lo.W_hi + a_hi.W_lo) (docs/ARCHITECTURE.md 2.3).
Every scoring path shares the packed hi/lo image, the layouts and the K-split logits layer, so the
paths agreeing with each other says nothing about the lo terms.  Here the model of each forward is
plain torch float64, and a shard is built so that a kernel that dropped or misplaced the lo terms, or
mis-scored one row of a partial block, gets a different confusion matrix and a different loss:

* ``bf16_logits(flat, dims, X, mode)``: ``"split"`` (the kernels' scoring forward), ``"plain"``
  (hi.hi only: the training forward of several clients, FLConfig::plain_fwd) or ``"exact"``
  (float64 of the fp32 parameters);
* ``trained_flat(dims)``: 40 rounds of the fp32 torch oracle at lr 0.02 on 300 rows (a fresh model
  predicts one or two classes only), once per shape;
* ``planted_shard(flat, dims, n_rows, R, seed)``: ``n_rows`` of 20 000 candidate rows.  Rows whose
  split top-2 margin is below 1e-5 max|z_split| are never taken, so the expected confusion matrix
  is exact.  Rows with argmax(split) != argmax(plain), both margins above that threshold, are the
  "discriminating" rows: as many as there are (at most n_rows // 2) are taken, the first ones at
  row 0, row R - 1, the first row of the last block and the last row, where row masking goes
  wrong.  Labels are the candidates' own teacher labels (a teacher the model was not trained on),
  so the loss is an ordinary CE and the confusion matrix has off-diagonal mass.

No GPU anywhere in this module; tests/test_bf16_oracle_cpu.py holds the models to each other."""
import functools
from typing import NamedTuple

import numpy as np
import torch

from fedmi.fl.engine import EngineConfig, TorchRoundEngine
from fedmi.fl.metrics import metric_vector, metrics_from_confusion
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, _bf16_forward, float64_logits, make_multiclass

MODES = ("split", "plain", "exact")
N_CANDIDATES = 20000
MARGIN = 1e-5          # a row is sure when its top-2 logit margin is at least MARGIN * max|z_split|
TRAIN_ROWS, TRAIN_ROUNDS, TRAIN_LR = 300, 40, 0.02

# (dims, R) of the bf16 scoring tests and, per case, the shards: R + 1 rows (a second workgroup
# with one live row) and 3 R - 1 (a partial last block)
SCORING_CASES = [
    ((14, 50, 200, 2), 32),    # the shape-specialised kernels
    ((14, 50, 200, 2), 16),
    ((14, 33, 17, 9, 5), 16),
    ((14, 33, 17, 9, 5), 32),
    ((33, 65, 3), 32),
    ((1, 16, 2), 16),
    ((14, 40, 16), 32),
    ((40, 40, 96, 4), 32),     # second bf16 k-step of layer 0
    ((14, 7, 2), 64),
]
SHARD_SEED = 0


def shard_sizes(R):
    return (R + 1, 3 * R - 1)


def case_id(dims, R, n_rows=None):
    s = "-".join(map(str, dims)) + f"@R{R}"
    return s if n_rows is None else s + f"x{n_rows}"


def bf16_logits(flat, dims, X, mode):
    """Logits [n, C] (float64 numpy) of the MLP with dense fp32 parameters ``flat`` on rows ``X``
    under the forward ``mode`` names."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    if mode == "exact":
        return float64_logits(flat, list(dims), X)
    return _bf16_forward(flat, X, list(dims), plain=(mode == "plain"))[2].numpy()


def cross_entropy(z, y):
    """Mean softmax cross-entropy of float64 logits, in float64."""
    return float(torch.nn.functional.cross_entropy(torch.as_tensor(z, dtype=torch.float64),
                                                   torch.as_tensor(np.asarray(y), dtype=torch.long)))


def confusion(y, z, C):
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (np.asarray(y), np.argmax(z, 1)), 1)
    return cm


def _margin(z):
    top = np.sort(z, 1)
    return top[:, -1] - top[:, -2]


@functools.lru_cache(maxsize=None)
def trained_flat(dims):
    """Dense fp32 parameters of the ``dims`` MLP after TRAIN_ROUNDS rounds of the fp32 torch oracle
    (read-only, computed once per shape)."""
    dims = tuple(int(d) for d in dims)
    F, C, hidden = dims[0], dims[-1], dims[1:-1]
    X, y = make_multiclass(TRAIN_ROWS, F, C, DATA_SEED)
    cfg = EngineConfig(hidden=hidden, max_rounds=TRAIN_ROUNDS, early_stop=False, lr=TRAIN_LR)
    ref = TorchRoundEngine(X, y, C, cfg, None, init_flat(list(dims), INIT_SEED))
    ref.run(TRAIN_ROUNDS)
    flat = ref.global_flat()
    flat.setflags(write=False)
    return flat


class Candidates(NamedTuple):
    X: np.ndarray
    y: np.ndarray
    z: dict            # mode -> logits [N_CANDIDATES, C]
    sc: float          # max|z_split|
    sure: np.ndarray   # split margin >= MARGIN * sc
    disc: np.ndarray   # argmax(split) != argmax(plain), both margins >= MARGIN * sc


@functools.lru_cache(maxsize=None)
def _candidates(flat_bytes, dims, seed):
    flat = np.frombuffer(flat_bytes, np.float32)
    X, y = make_multiclass(N_CANDIDATES, dims[0], dims[-1], seed)
    z = {m: bf16_logits(flat, dims, X, m) for m in MODES}
    sc = float(np.abs(z["split"]).max())
    sure = _margin(z["split"]) >= MARGIN * sc
    disc = sure & (_margin(z["plain"]) >= MARGIN * sc) & (np.argmax(z["split"], 1) != np.argmax(z["plain"], 1))
    for a in (X, y, sure, disc, *z.values()):
        a.setflags(write=False)
    return Candidates(X, y, z, sc, sure, disc)


def candidates(flat, dims, seed=DATA_SEED + 1):
    """The candidate rows of ``planted_shard`` with their logits under every mode (cached)."""
    return _candidates(np.ascontiguousarray(flat, np.float32).tobytes(), tuple(int(d) for d in dims), int(seed))


class Shard(NamedTuple):
    X: np.ndarray
    y: np.ndarray
    cm_split: np.ndarray
    cm_plain: np.ndarray
    ce_split: float
    ce_plain: float
    ce_exact: float
    disc_rows: np.ndarray   # positions of the discriminating rows in the shard
    index: np.ndarray       # the candidates taken, in shard order

    def metrics(self, mode="split"):
        """The 4-metric vector of the model's confusion matrix."""
        return metric_vector(metrics_from_confusion(self.cm_split if mode == "split" else self.cm_plain))

    @property
    def ce_gap(self):
        """|CE_plain - CE_split| / CE_split: what a forward without the lo terms moves the loss by."""
        return abs(self.ce_plain - self.ce_split) / self.ce_split


def edge_rows(n_rows, R):
    """Row 0, row R - 1, the first row of the last block, the last row (without repeats)."""
    out = []
    for p in (0, R - 1, ((n_rows - 1) // R) * R, n_rows - 1):
        if 0 <= p < n_rows and p not in out:
            out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def _planted(flat_bytes, dims, n_rows, R, seed):
    cand = _candidates(flat_bytes, dims, DATA_SEED + 1)
    rng = np.random.default_rng([int(seed), int(n_rows), int(R)])
    disc = np.flatnonzero(cand.disc)[:n_rows // 2]
    plainrows = rng.permutation(np.flatnonzero(cand.sure & ~cand.disc))[:n_rows - len(disc)]
    edges = edge_rows(n_rows, R)
    others = [int(p) for p in rng.permutation(n_rows) if p not in edges]
    pos = np.asarray((edges + others)[:len(disc)], np.int64)
    index = np.full(n_rows, -1, np.int64)
    index[pos] = disc
    index[index < 0] = plainrows
    assert cand.sure[index].all() and len(set(index.tolist())) == n_rows
    X, y = cand.X[index].copy(), cand.y[index].copy()
    C = dims[-1]
    zs, zp, ze = (cand.z[m][index] for m in MODES)
    out = Shard(X, y, confusion(y, zs, C), confusion(y, zp, C), cross_entropy(zs, y), cross_entropy(zp, y),
                cross_entropy(ze, y), np.sort(pos), index)
    for a in (out.X, out.y, out.cm_split, out.cm_plain, out.disc_rows, out.index):
        a.setflags(write=False)
    return out


def planted_shard(flat, dims, n_rows, R, seed=SHARD_SEED):
    """An evaluation shard of ``n_rows`` sure candidate rows with the discriminating rows planted at
    the block edges of ``R`` rows per workgroup, and what the split and the plain model make of it
    (cached per model, shape and seed; every array read-only)."""
    return _planted(np.ascontiguousarray(flat, np.float32).tobytes(), tuple(int(d) for d in dims), int(n_rows),
                    int(R), int(seed))


# ---- loss tolerance of the GPU tests ----
# history()["loss"] of a bf16 engine is held to the host model's CE within loss_tolerance(shard):
# the project's 1e-4 (tests/test_hip_engine_shapes.py), and never more than 1/8 of what dropping the
# lo terms moves this shard's CE by.  That gap is a signed sum over the rows and can cancel (seed 0
# of 14-40-16 at 95 rows: 5e-6), so a scoring shard takes the first seed whose tolerance is at least
# LOSS_NOISE, an allowance for what an fp32-accumulating kernel may differ from the float64 host
# model by: the loss is an fp32 sum of at most 200 per-row terms whose logits are fp32 sums of at
# most 200 exact bf16 products (2^-24 per operation, random signs: about sqrt(200) 2^-24 = 1e-6 of
# the largest term), stored as fp32 (6e-8) -- 1e-6, times ten.  The rule reads host models only.
LOSS_RTOL = 1e-4
LOSS_NOISE = 1e-5


def loss_tolerance(shard):
    return min(LOSS_RTOL, shard.ce_gap / 8.0)


@functools.lru_cache(maxsize=None)
def scoring_shard(dims, R, n_rows):
    """(trained parameters, planted shard) of one GPU scoring case: the smallest seed from
    SHARD_SEED on whose loss tolerance is at least LOSS_NOISE."""
    flat = trained_flat(dims)
    for seed in range(SHARD_SEED, SHARD_SEED + 64):
        shard = planted_shard(flat, dims, n_rows, R, seed)
        if loss_tolerance(shard) >= LOSS_NOISE:
            return flat, shard
    raise AssertionError(f"{case_id(dims, R, n_rows)}: no seed separates the split and the plain loss")

"""Held-out ROC AUC on the GPU (fedmi/ops/csrc/fl_auc.hip): the rank kernel alone on synthetic keys against
the numpy count, and the key + rank launches inside the round against ``auc_u2_model`` of the engine's own
``predict_proba``.  Every comparison is integer (or bitwise) equality."""
import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.fl.metrics import auc_u2_from_keys, auc_u2_model
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import init_flat
from fedmi.ops import native

from .reference_oracle import make_multiclass

pytestmark = pytest.mark.gpu

PATTERNS = ["uniform", "three_values", "all_equal", "pos_above", "pos_below", "top_byte", "low_byte", "no_positive"]


def _keys(pattern, n, rng):
    """uint32 keys (bits << 1) | flag of one class, bits below 2^30."""
    flag = rng.integers(0, 2, n).astype(np.uint32)
    bits = {"uniform": lambda: rng.integers(0, 1 << 30, n),
            "three_values": lambda: rng.choice([0x3E800000, 0x3F000000, 0x3F400000], n),
            "all_equal": lambda: np.full(n, 0x3F000000),
            "pos_above": lambda: rng.integers(0, 1 << 29, n) + (flag.astype(np.int64) << 29),
            "pos_below": lambda: rng.integers(0, 1 << 29, n) + ((1 - flag.astype(np.int64)) << 29),
            "top_byte": lambda: (rng.integers(0, 128, n) << 23) | 0x1234,   # key bits 24..30 differ, and the flag
            "low_byte": lambda: 0x3F000000 | rng.integers(0, 128, n),       # key bits 0..7 differ
            "no_positive": lambda: rng.integers(0, 1 << 30, n)}[pattern]().astype(np.uint32)
    if pattern == "no_positive":
        flag[:] = 0
    return (bits << np.uint32(1)) | flag


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 32768])
def test_rank_kernel(n, pattern):
    k0 = _keys(pattern, n, np.random.default_rng(n))
    keys = np.stack([k0, k0 ^ np.uint32(1)])   # class 1: the complement (for no_positive: no negative)
    dk = torch.as_tensor(keys.view(np.int32)).cuda()
    out = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    native().auc_rank(dk.data_ptr(), n, 2, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    P, N = int((k0 & 1).sum()), int(n - (k0 & 1).sum())
    want = {"pos_above": [2 * P * N, 0], "pos_below": [0, 2 * P * N], "no_positive": [0, 0]}.get(
        pattern, [auc_u2_from_keys(keys[0]), auc_u2_from_keys(keys[1])])
    assert out.tolist() == want


SHAPES = {"income": ([14, 50, 200, 2], 77), "three": ([17, 24, 3], 130)}
_RUNS = {}


def _run(shape, dtype, auc, graph_rounds=0, steps=(4,)):
    """(history, global weights, local weights, per-run() U2 rows of the model) of one client, once per case."""
    key = (shape, dtype, auc, graph_rounds, steps)
    if key not in _RUNS:
        dims, n_val = SHAPES[shape]
        X, y = make_multiclass(200, dims[0], dims[-1], 3)
        Xv, yv = make_multiclass(n_val, dims[0], dims[-1], 11)
        Xv, yv = np.ascontiguousarray(Xv, np.float32), np.asarray(yv).astype(np.int64)
        cfg = EngineConfig(hidden=tuple(dims[1:-1]), max_rounds=8, early_stop=False, dtype=dtype, graph_rounds=graph_rounds)
        e = HipRoundEngine(np.ascontiguousarray(X, np.float32), np.asarray(y).astype(np.int64), dims[-1], cfg, None,
                           init_flat(dims, 1))
        e.set_heldout(Xv, yv, auc=auc)
        model = []
        for k in steps:
            e.run(k)
            p = e.predict_proba(Xv, which="global")
            model.append([auc_u2_model(p[:, c], yv == c) for c in range(dims[-1])])
        _RUNS[key] = (e.history(), e.global_flat(), e.local_flat(), model, e.layout.get("heldout_auc"))
    return _RUNS[key]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_round_rows(shape, dtype):
    h, gflat, lflat, model, lay = _run(shape, dtype, True, steps=(1, 1, 1, 1))
    assert lay == {"max_rows": 32768, "launches": 2}
    assert h["heldout_auc_u2"].dtype == np.int64 and h["heldout_auc_u2"].tolist() == model
    assert (h["heldout_auc_u2"] > 0).all()
    for graph_rounds in (0, 2):   # four rounds in one run(), eager and replayed
        h4 = _run(shape, dtype, True, graph_rounds)[0]
        assert h4["heldout_auc_u2"].tolist() == model
    h0, g0, l0, _, lay0 = _run(shape, dtype, False)   # the same run without auc: nothing else moves
    assert lay0 is None and "heldout_auc_u2" not in h0
    for k in ("heldout_cm", "heldout_loss_sum", "global", "per_rank", "loss"):
        assert np.asarray(h0[k]).tobytes() == np.asarray(h[k]).tobytes(), k
    assert g0.tobytes() == gflat.tobytes() and l0.tobytes() == lflat.tobytes()


def test_client_group_median():
    dims, n_val = SHAPES["three"]
    X, y = make_multiclass(240, dims[0], dims[-1], 3)
    Xv, yv = make_multiclass(n_val, dims[0], dims[-1], 11)
    yv = np.asarray(yv).astype(np.int64)
    cfg = EngineConfig(hidden=tuple(dims[1:-1]), max_rounds=8, early_stop=False, aggregator="median")
    g = ClientGroup(np.ascontiguousarray(X, np.float32), np.asarray(y).astype(np.int64), 3, cfg, backend="hip",
                    shard_mode="iid", heldout=(np.ascontiguousarray(Xv, np.float32), yv), heldout_auc=True)
    for r in range(3):
        g.run(1)
        p = g.clients[0].predict_proba(Xv, which="global")
        assert g.history()["heldout_auc_u2"][r].tolist() == [auc_u2_model(p[:, c], yv == c) for c in range(3)]


def test_row_cap():
    dims = SHAPES["income"][0]
    X, y = make_multiclass(64, dims[0], 2, 3)
    Xv = np.zeros((32769, dims[0]), np.float32)
    yv = np.arange(32769) % 2
    e = HipRoundEngine(np.ascontiguousarray(X, np.float32), np.asarray(y).astype(np.int64), 2,
                       EngineConfig(hidden=(50, 200), max_rounds=4), None, init_flat(dims, 1))
    with pytest.raises(ValueError, match="auc"):
        e.set_heldout(Xv, yv, auc=True)
    e.set_heldout(Xv, yv, auc=False)
    assert e.heldout and "heldout_auc" not in e.layout

"""Every bf16 scoring path against the float64 host model of the split-bf16 forward
(tests/bf16_oracle.py), on shards planted with the rows a plain bf16 forward scores differently.

An engine built with lr = 0 (no weight decay, no FedProx term, no early stop) from trained
parameters ``flat`` never moves them -- asserted bit for bit on local_flat() and global_flat() -- so
every round's evaluation scores, and every round's training forward computes the loss of, exactly
``flat`` on the planted shard.  Per (shape, rows per workgroup) the shards have R + 1 rows (a second
workgroup with one live row) and 3 R - 1 rows (a partial last block), with the discriminating rows
at row 0, row R - 1, the first row of the last block and the last row.  The paths:

(a) the stand-alone bf16 eval kernel (step API): the confusion matrix, cell by cell;
(b) one client's fused scoring inside fl_train_bf16 (the shape-specialised kernel at 14-50-200-2,
    R = 32), eager and replayed from a 2-round graph, with the closing flush by the eval kernel;
(c) several (emulated) clients' lagged scoring: in registers on workgroups of their own and on the
    training workgroups' idle waves (FEDMI_SPLIT_SCORE=1 / 0) where layout()["lag_reg"] holds, the
    serial pass where it does not (C = 5, C = 16, more than 32 features, R = 64) and under
    FEDMI_LAG_REG=0.

Each must reproduce the split model's confusion matrix / 4-metric vector (atol 1e-12) in every
round, which the plain model's differs from (tests/test_bf16_oracle_cpu.py), and every round's
history loss must sit within bf16_oracle.loss_tolerance of the CE of the forward the engine's
layout()["plain_fwd"] names: the split model's, or -- the training pass of several clients scored in
registers -- the plain model's; (c) runs once more with plain_fwd=False, so both forwards are
checked on the same shard.  The tolerance is min(1e-4, 1/8 of that shard's |CE_plain - CE_split| /
CE_split), between 1.0e-5 and 1e-4.

Measured on MI355X, worst |loss - CE_model| / CE_model over all rounds and shards of a path:
(a) 3.3e-7, (b) 3.3e-7, (c) 3.3e-7 against the split model and 1.1e-7 against the plain one
(fp32 accumulation order; at most 1/50 of the case's tolerance, the smallest of which is 1.03e-5).
With the plain model's expectations in the split model's place all 72 cases of (a)-(c) fail.

The training pass itself: the slab-summed gradient of one fl_train_bf16 launch of an emulated
client against the host model of the forward the layout names, 1e-3 per tensor, and closer to that
model than to the other one."""
import numpy as np
import pytest

from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.models.mlp import init_flat

from . import bf16_oracle as bo
from .reference_oracle import DATA_SEED, INIT_SEED, _split_bf16_reference_grad, make_multiclass

pytestmark = pytest.mark.gpu

CASES = [(dims, R, n) for dims, R in bo.SCORING_CASES for n in bo.shard_sizes(R)]
IDS = [bo.case_id(*c) for c in CASES]
# (dims, R) whose lagged rounds score in registers (fl_layout.h fl_lag_reg_ok: one or two hidden
# layers, at most 32 features, C <= 4, R = 16 or 32)
LAG_REG = {((14, 50, 200, 2), 32), ((14, 50, 200, 2), 16), ((1, 16, 2), 16)}
SPEC = ((14, 50, 200, 2), 32)


def _engine(dims, R, shard, flat, emulate=False, **kw):
    cfg = EngineConfig(hidden=tuple(dims[1:-1]), lr=0.0, weight_decay=0.0, prox_mu=0.0, early_stop=False,
                       max_rounds=8, rows_per_block=R, dtype="bf16", **kw)
    # (copies: the cached shard is read-only)
    e = HipRoundEngine(shard.X.copy(), shard.y.copy(), dims[-1], cfg, None, flat, emulate_clients=emulate)
    assert e.R == R and e.layout["dtype"] == 1
    assert int(e.layout["n_slabs"]) == (len(shard.y) + R - 1) // R >= 2
    return e


def _check_history(e, shard, flat, rounds, what):
    """Every round scored the split model; every round's loss is the CE of the forward that ran;
    the parameters never moved."""
    h = e.history()
    assert h["rounds_run"] == rounds, h["rounds_run"]
    want, other = shard.metrics("split"), shard.metrics("plain")
    assert np.abs(want - other).max() > 1e-9
    for r in range(rounds):
        np.testing.assert_allclose(h["per_rank"][r, 0], want, rtol=0, atol=1e-12, err_msg=f"{what} round {r}")
        np.testing.assert_allclose(h["global"][r], want, rtol=0, atol=1e-12, err_msg=f"{what} round {r}")
        assert np.abs(h["per_rank"][r, 0] - other).max() > 1e-9, (what, r)
    plain = bool(e.layout["plain_fwd"])
    ce = shard.ce_plain if plain else shard.ce_split
    tol = bo.loss_tolerance(shard)
    err = np.abs(h["loss"].astype(np.float64) - ce) / ce
    print(f"LOSS {what} forward={'plain' if plain else 'split'} max|loss-CE|/CE {err.max():.3e} tolerance {tol:.3e} "
          f"other model {abs(shard.ce_plain - shard.ce_split) / shard.ce_split:.3e}")
    assert (err <= tol).all(), (what, err, tol)
    assert np.array_equal(e.local_flat(), flat), what
    assert np.array_equal(e.global_flat(), flat), what
    return plain


# ---- (a) the stand-alone eval kernel ----
@pytest.mark.parametrize("dims,R,n", CASES, ids=IDS)
def test_eval_kernel_scores_the_split_model(dims, R, n):
    flat, shard = bo.scoring_shard(dims, R, n)
    e = _engine(dims, R, shard, flat, fused_eval=False, graph_rounds=0)
    assert not e.engine.fused and not e.engine.lagged and not e.layout["plain_fwd"]
    for r in range(2):
        e.step_train()
        cm = e.step_eval()
        e.step_aggregate()
        np.testing.assert_array_equal(cm, shard.cm_split, err_msg=f"round {r}")
        assert not np.array_equal(cm, shard.cm_plain)
    e.sync_history()
    _check_history(e, shard, flat, 2, "eval " + bo.case_id(dims, R, n))


# ---- (b) one client's fused scoring ----
@pytest.mark.parametrize("graph_rounds", [0, 2])
@pytest.mark.parametrize("dims,R,n", CASES, ids=IDS)
def test_fused_scoring_scores_the_split_model(dims, R, n, graph_rounds):
    flat, shard = bo.scoring_shard(dims, R, n)
    e = _engine(dims, R, shard, flat, fused_eval=True, graph_rounds=graph_rounds)
    assert e.engine.fused and not e.layout["plain_fwd"]
    assert e.layout["shape_spec"] is ((dims, R) == SPEC), e.layout
    assert e.run(3) == 3
    assert e.engine.graph_captures == (1 if graph_rounds else 0)
    assert e.engine.eval_launches == 1   # rounds 0 and 1 were scored by the next train kernel, round 2 by the flush
    _check_history(e, shard, flat, 3, f"fused g{graph_rounds} " + bo.case_id(dims, R, n))


# ---- (c) several clients' lagged scoring ----
@pytest.mark.parametrize("dims,R,n", CASES, ids=IDS)
def test_lagged_scoring_scores_the_split_model(dims, R, n, monkeypatch):
    flat, shard = bo.scoring_shard(dims, R, n)
    reg = (dims, R) in LAG_REG
    # (FEDMI_LAG_REG, FEDMI_SPLIT_SCORE, EngineConfig.plain_fwd)
    variants = [(None, "1", None), (None, "0", None), ("0", None, None), (None, "0", False)] if reg else \
        [(None, None, None)]
    ran = set()
    for lag_reg, split, plain_fwd in variants:
        for name, v in (("FEDMI_LAG_REG", lag_reg), ("FEDMI_SPLIT_SCORE", split)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        e = _engine(dims, R, shard, flat, emulate=True, fused_eval=False, lagged_eval=True, graph_rounds=0,
                    plain_fwd=plain_fwd)
        lay = e.layout
        assert e.engine.lagged and not e.engine.fused
        assert lay["lag_reg"] is (reg and lag_reg is None), lay
        assert lay["plain_fwd"] is (reg and lag_reg is None and plain_fwd is None), lay
        assert lay["split_score"] is (reg and lag_reg is None and split == "1"), lay
        assert e.run(4) == 4
        assert e.engine.eval_launches == 1   # the closing round evaluates itself, the others are scored lagged
        ran.add(_check_history(e, shard, flat, 4, f"lagged LAG_REG={lag_reg} SPLIT_SCORE={split} plain_fwd={plain_fwd} "
                               + bo.case_id(dims, R, n)))
    assert ran == ({True, False} if reg else {False})


# ---- the training pass of several clients ----
GRAD_CASES = [((40, 40, 96, 4), False),   # more than 32 features: no register scoring, the split forward trains
              ((14, 40, 96, 4), True)]    # register scoring: the plain forward trains


@pytest.mark.parametrize("dims,plain", GRAD_CASES, ids=["-".join(map(str, d)) for d, _ in GRAD_CASES])
def test_emulated_clients_train_kernel_gradient(dims, plain):
    """One fl_train_bf16 launch of an emulated client at R = 32 with the fp16 slab (300 rows, fresh
    parameters, as tests/test_hip_engine_shapes.py): the slab-summed gradient against the host model
    of the forward layout()["plain_fwd"] names -- at 14-40-96-4 the plain one, at 40-40-96-4, where
    the 40 features rule register scoring and with it the plain forward out, the split one -- within
    1e-3 per tensor, and closer to it than to the other model, per tensor and overall.
    Measured on MI355X, overall |g - model| / |model|: 14-40-96-4 1.1e-4 to the plain model and
    1.4e-2 to the split one; 40-40-96-4 1.3e-4 to the split model and 2.3e-2 to the plain one (worst
    tensor to its own model 1.6e-4, best tensor to the other model 1.3e-3)."""
    F, C, hidden = dims[0], dims[-1], tuple(dims[1:-1])
    X, y = make_multiclass(300, F, C, DATA_SEED)
    flat = init_flat(list(dims), INIT_SEED)
    e = HipRoundEngine(X, y, C, EngineConfig(hidden=hidden, max_rounds=4, early_stop=False, rows_per_block=32,
                                             dtype="bf16", graph_rounds=0, grad_slab="fp16", fused_eval=False),
                       None, flat, emulate_clients=True)
    assert e.R == 32 and e.slab_f16 and e.engine.lagged
    assert e.layout["plain_fwd"] is plain and e.layout["lag_reg"] is plain, e.layout
    e.step_train()
    e.stream.synchronize()
    g = e.slab_partials().double().sum(0).cpu().numpy() / len(X)
    ref = {p: _split_bf16_reference_grad(flat, X, y, list(dims), scaled_delta=False, plain=p) for p in (False, True)}
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    off = 0
    for l in range(len(dims) - 1):
        for k in (dims[l] * dims[l + 1], dims[l + 1]):
            sl = slice(off, off + k)
            own, other = rel(g[sl], ref[plain][sl]), rel(g[sl], ref[not plain][sl])
            print("GRAD", dims, "layer", l, "n", k, "own model", own, "other model", other)
            assert own <= 1e-3, (l, k, own)
            assert own < other, (l, k, own, other)
            off += k
    own, other = rel(g, ref[plain]), rel(g, ref[not plain])
    print("GRAD", dims, "overall: own model", own, "other model", other)
    assert own <= 1e-3 and own < other, (own, other)

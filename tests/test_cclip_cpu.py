"""Centered clipping on the CPU: ``cclip_model`` against the float64 rule, validation, a torch group against the
float64 group oracle (nerr <= 2e-5).  No float64 distance of the model test lies within 1e-3 of ``tau`` (asserted)."""
import numpy as np
import pytest
import torch

from fedmi.fl import aggregate as A
from fedmi.fl.engine import EngineConfig, TorchRoundEngine, aggregator_id, common_init
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, init_flat, param_count

from .cclip_oracle import cclip_group_f64
from .geomed_oracle import tamper_two
from .reference_oracle import DATA_SEED, make_multiclass, nerr

SMALL, TAU = (17, 24, 3), 1.0


def _clients(dims, seed):
    """Images, padding 0: x and five clients: 0 NaN, 1 at 1e12 sign, 2 within tau (0.3 tau), 3 and 4 outside (5 tau)."""
    real = dense_to_image(np.ones(param_count(list(dims)), np.float32), list(dims)) != 0
    rng = np.random.default_rng(seed)
    draw = lambda s: np.where(real, np.float32(s) * rng.standard_normal(real.size).astype(np.float32), np.float32(0))
    x = draw(1.0)
    a = np.stack([x + draw(r * TAU / np.sqrt(real.sum())) for r in (1.0, 1.0, 0.3, 5.0, 5.0)])
    a[0, np.flatnonzero(real)[7]] = np.nan
    a[1] = np.float32(1e12) * np.sign(a[1])
    return x, a, real


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("dims", [SMALL, (14, 50, 200, 2)], ids=["small", "income"])
def test_model_against_the_float64_rule(dims, T):
    x, a, real = _clients(dims, 11)
    t32, t64 = [], []
    z = A.cclip_model(a, [True] * 5, real, x, T, TAU, trace=t32)
    ref = A.cclip_torch(torch.as_tensor(a[:, real]).double(), [True] * 5, torch.as_tensor(x[real]), T, TAU, trace=t64).numpy()
    assert len(t32) == len(t64) == T
    for q32, q64 in zip(t32, t64):
        assert q32["mask"] == q64["mask"] == 0b11110
        assert (q32["c"] == 1).tolist() == (q64["c"] == 1).tolist() == [False, False, True, False, False]
        assert (np.abs(np.sqrt(q64["d"][1:]) - TAU) > 1e-3).all()      # the float64 rule alone is stable here
    assert (z[~real].view(np.int32) == 0).all() and np.isfinite(ref).all() and nerr(z[real], ref) <= 2e-5
    a[:, np.flatnonzero(real)[7]], tr = np.nan, []     # nobody included: z stays x bit for bit
    z = A.cclip_model(a, [True] * 5, real, x, T, TAU, trace=tr)
    assert [q["mask"] for q in tr] == [0] * T and all(np.isinf(q["d"]).all() and (q["c"] == 0).all() for q in tr)
    np.testing.assert_array_equal(z.view(np.int32), x.view(np.int32))
    np.testing.assert_array_equal(A.cclip_torch(torch.as_tensor(a), [True] * 5, torch.as_tensor(x), T, TAU).numpy(), x)


def test_validation_and_refusals():
    assert A.AGGREGATORS == ("mean", "median", "trimmed_mean") and A.ITERATIVE_AGGREGATORS == ("geomed",)
    assert A.ALL_AGGREGATORS == A.AGGREGATORS + A.ITERATIVE_AGGREGATORS and A.CENTERED_AGGREGATORS == ("cclip",)
    assert A.AGGREGATOR_NAMES.index("cclip") == 4 == aggregator_id(EngineConfig(aggregator="cclip"))
    assert "cclip_tau" not in EngineConfig().to_dict() and common_init(EngineConfig(aggregator="cclip"))
    for kw in [dict(cclip_iters=v) for v in (0, 9, 2.5, "3", None, True)] + [
            dict(cclip_tau=v) for v in (0.0, -1.0, float("nan"), float("inf"), 1e-60, None, "x", True)]:
        with pytest.raises(ValueError, match=next(iter(kw))):
            aggregator_id(EngineConfig(aggregator="cclip", **kw))
    for kw, msg in ((dict(aggregator="krum"), "aggregator must be one of"), (dict(dp_clip=1.0), "differential privacy"),
                    (dict(gather_plane="xgmi"), "gather_plane='host'")):
        with pytest.raises(ValueError, match=msg):
            aggregator_id(EngineConfig(**{"aggregator": "cclip", **kw}))
    X, y = make_multiclass(40, 5, 2, DATA_SEED)
    with pytest.raises(ValueError, match="secagg does not combine"):
        TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, aggregator="cclip", secagg=True), SimRank(3, 0, "cpu"),
                         init_flat([5, 4, 2], 0), n_total=120)


def test_torch_group_against_the_float64_group_oracle(monkeypatch):
    X, y = make_multiclass(140, 17, 3, DATA_SEED)
    cfg = EngineConfig(hidden=(24,), max_rounds=6, early_stop=False, graph_rounds=0, aggregator="cclip")
    tamper = tamper_two(param_count(list(SMALL)), 1, 4)
    g = ClientGroup(X, y, 7, cfg, backend="torch", shard_mode="iid", seed=2, tamper=tamper)
    assert g.run(4) == 4 and g.clients[0].robust == 4 and g.clients[0].agg_scale == 1.0
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), g.global_flat())
    ref = cclip_group_f64(monkeypatch, [(c.X.numpy(), c.y.numpy()) for c in g.clients], 3, cfg, init_flat(list(SMALL), 2 * 1000003), 4, tamper)
    assert nerr(g.global_flat(), ref) <= 2e-5

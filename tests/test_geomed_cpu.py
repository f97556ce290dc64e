"""Geometric-median aggregation on the CPU: config validation and refusals, the fp32 numpy model of the
kernels (``geomed_model``) against the float64 oracle (``geomed_torch`` in float64), the robustness
property, the edge cases, and torch client groups against a float64 group oracle.

Model against oracle.  The limit is the project's nerr, max|err| / max|ref| <= 2e-5; a numpy prototype of
the rule gave 8e-8 .. 3.2e-7 at P = 11352 for K = 3 .. 64 and T = 1 .. 8.  No squared distance of the
inputs overflows fp32 (the "huge" tamperer is scaled by 1e12, squared distance ~1e28): float64 would
include, with a weight of ~1e-32, a client that fp32 excludes, so the included sets of every iteration
are asserted equal in both precisions.
"""
import functools
import os

import numpy as np
import pytest
import torch

from fedmi.fl.aggregate import (AGGREGATORS, ALL_AGGREGATORS, ITERATIVE_AGGREGATORS, geomed_block_sums, geomed_model,
                                geomed_torch, robust_aggregate_torch)
from fedmi.fl.engine import EngineConfig, TorchRoundEngine, aggregator_id
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .geomed_oracle import Float64GeomedGroupOracle, tamper_two
from .reference_oracle import DATA_SEED, make_multiclass, nerr

SMALL, INCOME = (17, 24, 3), (14, 50, 200, 2)
NU = 1e-6


# ---- validation ----
def test_config_validation_and_refusals():
    assert AGGREGATORS == ("mean", "median", "trimmed_mean") and ITERATIVE_AGGREGATORS == ("geomed",)
    assert ALL_AGGREGATORS == AGGREGATORS + ITERATIVE_AGGREGATORS and ALL_AGGREGATORS.index("geomed") == 3
    assert aggregator_id(EngineConfig(aggregator="geomed")) == 3
    d = EngineConfig()
    assert (d.geomed_iters, d.geomed_nu) == (3, 1e-6) and {"geomed_iters", "geomed_nu"} <= set(d.to_dict())
    for bad in (0, -1, 33, 2.5, "3", None, True):
        for agg in ("geomed", "mean"):      # the fields are validated whatever the rule, as trim_ratio is
            with pytest.raises(ValueError, match="geomed_iters"):
                aggregator_id(EngineConfig(aggregator=agg, geomed_iters=bad))
    for bad in (0.0, -1e-6, float("nan"), float("inf"), 1e-60, None, "x", True):
        with pytest.raises(ValueError, match="geomed_nu"):
            aggregator_id(EngineConfig(aggregator="geomed", geomed_nu=bad))
    for T in (1, 32):
        aggregator_id(EngineConfig(aggregator="geomed", geomed_iters=T, geomed_nu=0.5))
    with pytest.raises(ValueError, match="aggregator must be one of"):
        aggregator_id(EngineConfig(aggregator="krum"))
    with pytest.raises(ValueError, match="differential privacy"):
        aggregator_id(EngineConfig(aggregator="geomed", dp_clip=1.0))
    with pytest.raises(ValueError, match="gather_plane='host'"):
        aggregator_id(EngineConfig(aggregator="geomed", gather_plane="xgmi"))
    aggregator_id(EngineConfig(aggregator="median", gather_plane="xgmi"))
    X, y = make_multiclass(40, 5, 2, DATA_SEED)
    flat = init_flat([5, 4, 2], 0)
    cfg = lambda **kw: EngineConfig(hidden=(4,), max_rounds=2, aggregator="geomed", **kw)
    with pytest.raises(ValueError, match="differential privacy"):
        TorchRoundEngine(X, y, 2, cfg(dp_clip=0.5, dp_seed=1), None, flat)
    with pytest.raises(ValueError, match="secagg does not combine"):
        TorchRoundEngine(X, y, 2, cfg(secagg=True), SimRank(3, 0, "cpu"), flat, n_total=120)
    with pytest.raises(ValueError, match="at most 64 clients"):
        TorchRoundEngine(X, y, 2, cfg(), SimRank(65, 0, "cpu"), flat, n_total=65 * 40)
    with pytest.raises(ValueError, match="gather_plane='host'"):
        TorchRoundEngine(X, y, 2, cfg(gather_plane="xgmi"), SimRank(3, 0, "cpu"), flat, n_total=120)
    # one client: the aggregate is the identity, nothing is refused
    e = TorchRoundEngine(X, y, 2, cfg(gather_plane="xgmi"), None, flat)
    assert e.robust == 0 and e.run(2) == 2
    e3 = TorchRoundEngine(X, y, 2, cfg(), SimRank(3, 0, "cpu"), flat, n_total=120)
    assert e3.robust == 3 and e3.agg_scale == 1.0
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    with pytest.raises(ValueError, match="robust-aggregator"):
        FedTrialGroup(X, y, 2, [FedTrial((4,), 0.01, 1)], None, EngineConfig(max_rounds=2, aggregator="geomed"),
                      backend="torch")
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="robust aggregator"):
        WideClient(torch.zeros(4, 14), torch.zeros(4, dtype=torch.long), [14, 8, 2], aggregator="geomed")
    from fedmi.fl.engine import HipRoundEngine
    with pytest.raises(ValueError, match="comm_buffers"):   # refused before anything touches a device
        HipRoundEngine(X, y, 2, cfg(), None, flat, comm_buffers=[torch.zeros(8), torch.zeros(8)])
    for fn in (geomed_torch, lambda s, a, T, nu: geomed_model(s.numpy(), a, np.ones(8, bool), T, nu)):
        s = torch.zeros(3, 8)
        for args in (([True] * 2, 3, NU), ([False] * 3, 3, NU), ([True] * 3, 0, NU), ([True] * 3, 33, NU),
                     ([True] * 3, 3, 0.0), ([True] * 3, 3, float("nan"))):
            with pytest.raises(ValueError):
                fn(s, *args)


# ---- the model against the float64 oracle ----
@functools.lru_cache(maxsize=None)
def _real(dims):
    return dense_to_image(np.ones(param_count(list(dims)), np.float32), list(dims)) != 0


def _images(dense, dims):
    return np.stack([dense_to_image(np.ascontiguousarray(row), list(dims)) for row in dense])


def _dense(img, dims):
    """The dense parameters of an image: the image of 1 .. P names every real position."""
    P = param_count(list(dims))
    pos = dense_to_image(np.arange(1, P + 1, dtype=np.float32), list(dims))   # (P < 2^24: exact)
    out = np.zeros(P, img.dtype)
    out[pos[pos != 0].astype(np.int64) - 1] = img[pos != 0]
    return out


def _clients(dims, K, seed, n_bad):
    """[K, P] fp32: honest c + 0.01 N(0, I); the first ``n_bad`` odd clients are wrong -- alternately
    1e12 * sign(.) and one NaN among honest values."""
    P = param_count(list(dims))
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(P).astype(np.float32)
    a = (c + np.float32(0.01) * rng.standard_normal((K, P)).astype(np.float32)).astype(np.float32)
    bad = list(range(1, K, 2))[:n_bad]
    for j, k in enumerate(bad):
        if j % 2 == 0:
            a[k] = np.float32(1e12) * np.sign(a[k])
        else:
            a[k, int(rng.integers(P))] = np.nan
    return a, [k for k in range(K) if k not in bad]


@pytest.mark.parametrize("dims", [SMALL, INCOME], ids=["small", "income"])
@pytest.mark.parametrize("K", [3, 5, 7, 64])
def test_model_against_the_float64_oracle(dims, K):
    real = _real(dims)
    a, honest = _clients(dims, K, 40 + K, n_bad={3: 1, 5: 2, 7: 2, 64: 30}[K])
    img = _images(a, dims)
    act = [True] * K
    for T in (1, 3, 8):
        t32, t64 = [], []
        z = geomed_model(img, act, real, T, NU, trace=t32)
        ref = geomed_torch(torch.as_tensor(a).double(), act, T, NU, trace=t64).numpy()
        assert t32 == t64 and len(t32) == T, (K, T)      # the same clients included in every iteration
        assert all(set(honest) <= set(s) for s in t32)
        assert (z[~real].view(np.int32) == 0).all()
        err = nerr(_dense(z, dims), ref)
        print(f"dims={list(dims)} K={K} T={T}: model vs float64 {err:.3g}")
        assert np.isfinite(ref).all() and err <= 2e-5, (K, T, err)


# ---- the robustness property ----
@pytest.mark.parametrize("K,n_bad", [(7, 2), (64, 30)])
def test_robustness_property(K, n_bad):
    dims = SMALL
    a, honest = _clients(dims, K, 9 + K, n_bad)
    act = [True] * K
    h = a[honest].astype(np.float64)
    center = h.mean(0)
    spread = max(float(np.linalg.norm(h[i] - h[j])) for i in range(len(h)) for j in range(i))
    # the float64 oracle first, then the fp32 model
    z64 = geomed_torch(torch.as_tensor(a).double(), act, 3, NU).numpy()
    z32 = _dense(geomed_model(_images(a, dims), act, _real(dims), 3, NU), dims)
    for name, z in (("float64", z64), ("fp32", z32)):
        dist = float(np.linalg.norm(z.astype(np.float64) - center))
        print(f"K={K}, {n_bad} wrong: {name} |z - mean(honest)| = {dist / spread:.3f} of the honest spread")
        assert np.isfinite(z).all() and dist <= spread, (name, dist, spread)
    with np.errstate(all="ignore"):
        assert not np.isfinite(a.astype(np.float64).mean(0)).all()      # the unscreened mean is poisoned


# ---- edge cases ----
def _both(a, act, T, nu=NU, real=None):
    """(fp32 model on all-real "images", geomed_torch in fp32, in float64) of the rows of ``a``."""
    a = np.asarray(a, np.float32)
    real = np.ones(a.shape[1], bool) if real is None else real
    return (geomed_model(a, act, real, T, nu), geomed_torch(torch.as_tensor(a), act, T, nu).numpy(),
            geomed_torch(torch.as_tensor(a).double(), act, T, nu).numpy())


def test_edge_cases():
    rng = np.random.default_rng(3)
    P = 300
    a = rng.standard_normal((5, P)).astype(np.float32)
    # K_r = 1: the client itself (d = 0, the nu clamp: b = 1 / nu; b v / b is within 1 ulp of v)
    one = [False, False, True, False, False]
    for z in _both(a, one, 3):
        np.testing.assert_allclose(z, a[2], rtol=2.0 ** -23, atol=0)
    # K_r = 2: z_0 is the midpoint, both clients at equal distance, the combine stays there
    two = [True, False, False, True, False]
    mid = (a[0].astype(np.float64) + a[3]) / 2
    for z in _both(a, two, 3):
        assert nerr(z, mid) <= 2e-5
    # all clients identical: d = 0 exactly, the nu clamp, finite.  Two clients: b v + b v and b + b are exact,
    # so z = fl(fl(b v) / b), within 1 ulp of the input.  Four: 3 p and 3 b round once more each (2 p, 2 b
    # are exact; 4 p, 4 b take a last rounding), so the relative error is at most
    # (1 + 3/4 + 1 + 3/4 + 1 + 1) 2^-24 = 5.5 x 2^-24 to first order; asserted as 6 x 2^-24
    for n, rtol in ((2, 2.0 ** -23), (4, 6 * 2.0 ** -24)):
        same = np.repeat(a[:1], n, axis=0)
        rec = []
        z = geomed_model(same, [True] * n, np.ones(P, bool), 2, NU, records=rec)
        q = rec[0]     # (the second iteration measures the rounding of z_1, its equal weights give the same z)
        assert (q["d"] == 0).all() and (q["b"] == np.float32(1.0) / np.float32(NU)).all() and q["mask"] == 2 ** n - 1
        for z in (z, *_both(same, [True] * n, 2)):
            assert np.isfinite(z).all()
            np.testing.assert_allclose(z, a[0], rtol=rtol, atol=0)
    # every client non-finite: nobody is ever included, the result is z_0
    bad = a.copy()
    bad[:, 7] = np.nan
    bad[1] = np.inf
    tr, rec = [], []
    z = geomed_model(bad, [True] * 5, np.ones(P, bool), 3, NU, trace=tr, records=rec)
    z0 = robust_aggregate_torch(torch.as_tensor(bad), [True] * 5, "median", 0.0).numpy()
    assert tr == [[], [], []] and all(r["mask"] == 0 and np.isinf(r["d"]).all() for r in rec)
    np.testing.assert_array_equal(z.view(np.int32)[~np.isnan(z0)], z0.view(np.int32)[~np.isnan(z0)])
    assert np.isnan(z[7]) and np.isnan(z0[7])
    zt = geomed_torch(torch.as_tensor(bad), [True] * 5, 3, NU).numpy()
    np.testing.assert_array_equal(np.isnan(zt), np.isnan(z0))
    np.testing.assert_array_equal(zt[~np.isnan(z0)], z0[~np.isnan(z0)])
    # an iteration that includes nobody after one that combined keeps that combine's z: identical clients with
    # 1e35 at one position give d = 0, b = 1e6 and an overflowing b v, so z_1 holds +inf and nobody is at a
    # finite distance from it
    huge = np.repeat(a[:1], 4, axis=0)
    huge[:, 9] = 1e35
    tr, rec = [], []
    z = geomed_model(huge, [True] * 4, np.ones(P, bool), 3, NU, trace=tr, records=rec)
    assert tr == [[0, 1, 2, 3], [], []] and [q["mask"] for q in rec] == [15] * 3
    assert np.isposinf(z[9]) and np.isfinite(np.delete(z, 9)).all()
    np.testing.assert_array_equal(z, geomed_model(huge, [True] * 4, np.ones(P, bool), 1, NU))
    np.testing.assert_array_equal(z, geomed_torch(torch.as_tensor(huge), [True] * 4, 3, NU).numpy())
    # T = 1: one combine from the median
    act = [True] * 5
    tr = []
    z1 = geomed_model(a, act, np.ones(P, bool), 1, NU, trace=tr)
    assert tr == [[0, 1, 2, 3, 4]]
    med = robust_aggregate_torch(torch.as_tensor(a), act, "median", 0.0).numpy()
    d = ((a.astype(np.float64) - med) ** 2).sum(1)
    w = 1.0 / np.sqrt(d)
    assert nerr(z1, (w[:, None] * a).sum(0) / w.sum()) <= 2e-5
    # padding never enters a distance and comes out 0 whatever it holds
    real = np.ones(P, bool)
    real[50:60] = False
    dirty = a.copy()
    dirty[0, 50:60], dirty[1, 50:60] = np.nan, 1e30
    zc, zd = geomed_model(np.where(real, a, 0), act, real, 3, NU), geomed_model(dirty, act, real, 3, NU)
    np.testing.assert_array_equal(zc.view(np.int32), zd.view(np.int32))
    assert (zd[~real].view(np.int32) == 0).all()
    # a keep mask that removes the tamperers: the rule over mask & keep never reads them
    t = a.copy()
    t[1], t[3] = np.nan, 1e12
    keep = [True, False, True, False, True]
    clean = np.delete(a, [1, 3], axis=0)
    for got, want in zip(_both(t, keep, 3), _both(clean, [True] * 3, 3)):
        np.testing.assert_array_equal(got, want)


def test_block_sums_follow_the_stated_order():
    rng = np.random.default_rng(0)
    sq = (rng.standard_normal((2, 700)) ** 2).astype(np.float32)
    got = geomed_block_sums(sq)
    for k in range(2):
        pad = np.zeros(768, np.float32)
        pad[:700] = sq[k]
        d = np.float32(0.0)
        for blk in pad.reshape(3, 4, 64):
            s = np.float32(0.0)
            for run in blk:
                x = run.copy()
                for off in (32, 16, 8, 4, 2, 1):
                    x = x + x[np.arange(64) ^ off]
                s = np.float32(s + x[0])
            d = np.float32(d + s)
        assert got[k] == d
    assert nerr(got, sq.astype(np.float64).sum(1)) <= 1e-6


# ---- engine rounds ----
ROUNDS = 6
BAD = (1, 4)


def _group(agg, tampered, k=7, **kw):
    X, y = make_multiclass(140, 17, 3, DATA_SEED)
    cfg = EngineConfig(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, aggregator=agg, **kw)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, cfg, backend="torch", shard_mode="iid", seed=2,
                    tamper=tamper_two(param_count(list(SMALL)), *BAD) if tampered else None)
    return g


@pytest.mark.parametrize("tampered", [False, True], ids=["clean", "tampered"])
def test_torch_group_against_the_float64_group_oracle(tampered):
    g = _group("geomed", tampered)
    for r in range(ROUNDS):
        assert g.run(1) == 1 and np.isfinite(g.global_flat()).all(), r
    lead = g.clients[0]
    assert lead.robust == 3 and lead.agg_scale == 1.0
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), g.global_flat())
    flats = [init_flat(list(SMALL), 2 * 1000003 + r) for r in range(7)]
    o = Float64GeomedGroupOracle([(c.X.numpy(), c.y.numpy()) for c in g.clients], 3, lead.cfg, flats, lead.participants,
                                 tamper=tamper_two(param_count(list(SMALL)), *BAD) if tampered else None)
    o.run(ROUNDS)
    err = nerr(g.global_flat(), o.x)
    print(f"torch group geomed ({'tampered' if tampered else 'clean'}): vs float64 group oracle {err:.3g}")
    assert err <= 2e-5, err


def test_first_round_survives_a_nan_client_where_the_mean_does_not():
    g = _group("geomed", True)
    g.run(1)
    assert np.isfinite(g.global_flat()).all()
    m = _group("mean", True)
    m.run(1)
    assert not np.isfinite(m.global_flat()).any()


def test_torch_group_composes():
    for kw in (dict(participation=0.6), dict(server_opt="adam", server_lr=1e-2), dict(screen="multi_krum", screen_byzantine=2),
               dict(compress="topk", compress_ratio=0.5), dict(geomed_iters=1, geomed_nu=1e-3)):
        g = _group("geomed", "participation" not in kw, **kw)
        assert g.run(3) == 3 and np.isfinite(g.global_flat()).all(), kw
    h = g.history()
    assert "screen_kept" not in h and set(h) == set(_group("median", False).history())    # no new history key


# ---- the [C] entry point ----
def test_entry_point_flags():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    run = lambda *a: subprocess.run([sys.executable, script, "--device", "cpu", "--backend", "gloo", "--engine", "torch",
                                     "--quiet", *a], cwd=root, capture_output=True, text=True, timeout=300, env=env)
    r = run("--clients", "3", "--rounds", "3", "--aggregator", "geomed", "--geomed-iters", "2", "--geomed-nu", "1e-5")
    assert r.returncode == 0 and "3 simulated clients (torch): 3 rounds" in r.stdout, r.stderr[-2000:]
    for args, msg in ((("--aggregator", "geomed", "--wide"), "--aggregator is not supported with --wide"),
                      (("--aggregator", "geomed", "--geomed-iters", "0"), "geomed_iters"),
                      (("--aggregator", "geomed", "--geomed-nu", "0"), "geomed_nu"),
                      (("--aggregator", "geomed", "--gather-plane", "xgmi"), "gather_plane='host'"),
                      (("--aggregator", "geomed", "--dp-clip", "1.0"), "differential privacy")):
        r = run(*args)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr[-500:])

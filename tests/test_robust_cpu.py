"""Robust aggregation on the CPU: the torch model of the rule against an independent numpy oracle,
the t rule, config validation and refusals, and torch client groups with a Byzantine client.

The oracle sorts along the clients (``np.sort``: NaN last, -0 == +0), keeps ``[t : K_r - t]`` and
takes the mean in float64; ``robust_aggregate_torch`` in float64 sums the same kept values in client
order instead of sorted order, so the two differ by float64 summation order only: with n <= 9 kept
values, at most (n - 1) 2^-53 sum|kept| + 2^-53 |result| (one rounding per addition, one for the
division), asserted with 2x slack for the oracle's own roundings.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.aggregate import AGGREGATORS, robust_aggregate_torch, trim_count
from fedmi.fl.engine import EngineConfig, TorchRoundEngine, aggregator_id
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass

P = 257
KS = (1, 2, 3, 4, 5, 8, 9)
RULES = [("median", 0.0), ("trimmed_mean", 0.0), ("trimmed_mean", 0.1), ("trimmed_mean", 0.25), ("trimmed_mean", 0.49)]


def oracle(stack, mask, kind, beta):
    """(result, sum|kept|, n) of the numpy oracle in float64."""
    v = np.asarray(stack, np.float64)[np.asarray(mask, bool)]
    kr = v.shape[0]
    t = (kr - 1) // 2 if kind == "median" else min(int(np.floor(beta * kr)), (kr - 1) // 2)
    kept = np.sort(v, axis=0)[t:kr - t]
    return kept.mean(axis=0), np.abs(kept).sum(axis=0), kr - 2 * t


def planted(K, seed, bad=None):
    """[K, P] normals with exact ties across clients, +-0 and (``bad``) one NaN / +inf / -inf client."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((K, P))
    a[:, 10:40] = np.round(a[:, 10:40])                 # ties (and zeros) across clients
    a[:, 40:50] = a[0, 40:50]                           # a whole coordinate tied
    a[:, 50:60] = 0.0
    a[::2, 50:60] = -0.0                                # -0 / +0 mixed
    if bad is not None and K > 1:
        a[K // 2] = bad
    return a


def masks(K, seed):
    rng = np.random.default_rng(seed)
    out = [np.ones(K, bool)]
    for kr in range(1, K):
        m = np.zeros(K, bool)
        m[rng.choice(K, size=kr, replace=False)] = True
        out.append(m)
    return out


@pytest.mark.parametrize("K", KS)
def test_float64_model_matches_the_numpy_oracle(K):
    u = 2.0 ** -53
    for bad in (None, np.nan, np.inf, -np.inf):
        a = planted(K, 11 + K, bad)
        for mask in masks(K, K):
            for kind, beta in RULES:
                got = robust_aggregate_torch(torch.as_tensor(a), mask, kind, beta).numpy()
                ref, sabs, n = oracle(a, mask, kind, beta)
                kr = int(mask.sum())
                t = trim_count(kind, beta, kr)
                assert n == kr - 2 * t
                fin = np.isfinite(ref)
                if bad is not None and t >= 1:
                    assert fin.all(), (K, kind, beta, bad)       # one bad client is trimmed away
                if bad is None:
                    assert fin.all()
                np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
                np.testing.assert_array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
                bound = 2.0 * ((n - 1) * u * sabs[fin] + u * np.abs(ref[fin]))
                assert (np.abs(got[fin] - ref[fin]) <= bound).all(), (K, kind, beta, bad, mask)
                # fp32: same selection (the kept set does not depend on the precision of the sum)
                a32 = a.astype(np.float32)
                g32 = robust_aggregate_torch(torch.as_tensor(a32), mask, kind, beta).numpy()
                r32, s32, _ = oracle(a32, mask, kind, beta)
                f = np.isfinite(r32)
                b32 = 1.001 * ((n - 1) * 2.0 ** -24 * s32[f] + 2.0 ** -24 * np.abs(r32[f]))
                assert g32.dtype == np.float32 and (np.abs(g32[f].astype(np.float64) - r32[f]) <= b32).all()


def test_ties_break_by_client_index_and_nan_sorts_above_inf():
    # K = 4, t = 1 (median): keeps ranks 1, 2
    col = lambda *v: torch.tensor([[x] for x in v], dtype=torch.float32)
    act = [True] * 4
    assert float(robust_aggregate_torch(col(1, 1, 1, 5), act, "median", 0)) == 1.0
    assert float(robust_aggregate_torch(col(np.inf, np.nan, 2, 3), act, "median", 0)) == np.inf   # keeps 3, inf
    assert np.isnan(float(robust_aggregate_torch(col(np.nan, np.nan, 2, 3), act, "median", 0)))   # keeps 3, NaN
    neg_nan = float(np.frombuffer(np.uint32(0xFFC00000).tobytes(), np.float32)[0])   # sign bit set: still sorts high
    assert float(robust_aggregate_torch(col(neg_nan, 1, 2, 3), act, "median", 0)) == 2.5
    out = robust_aggregate_torch(col(-0.0, 0.0, -5, 5), act, "median", 0)
    assert float(out) == 0.0 and not np.signbit(out.numpy())[0]    # 0 + -0 + +0 in client order
    # the order treats NaN and +inf alike at the top: trimmed away together with the lowest value
    a = robust_aggregate_torch(col(1, np.nan, 2, 3, 4), [True] * 5, "trimmed_mean", 0.2)
    b = robust_aggregate_torch(col(1, np.inf, 2, 3, 4), [True] * 5, "trimmed_mean", 0.2)
    assert float(a) == float(b) == 3.0
    # unsampled rows are ignored whatever they hold
    c = robust_aggregate_torch(col(1, np.nan, 2, 3, 4), [True, False, True, True, True], "median", 0)
    assert float(c) == 2.5


def test_t_rule():
    for kr in range(1, 65):
        assert trim_count("median", 0.3, kr) == (kr - 1) // 2
        for beta in (0.0, 0.1, 0.2, 0.25, 0.49, np.nextafter(0.5, 0)):
            t = trim_count("trimmed_mean", beta, kr)
            assert 0 <= t and 2 * t < kr and t <= np.floor(beta * kr)
        assert trim_count("trimmed_mean", 0.0, kr) == 0
    assert trim_count("median", 0, 1) == 0 and trim_count("median", 0, 2) == 0
    assert trim_count("trimmed_mean", 0.2, 5) == 1 and trim_count("trimmed_mean", 0.1, 9) == 0
    x = torch.tensor([[1.0], [4.0]])
    assert float(robust_aggregate_torch(x[:1], [True], "median", 0)) == 1.0
    assert float(robust_aggregate_torch(x, [True, True], "median", 0)) == 2.5
    with pytest.raises(ValueError):
        trim_count("median", 0, 0)
    with pytest.raises(ValueError, match="trim_ratio"):
        trim_count("trimmed_mean", 0.5, 4)


def test_config_validation_and_refusals():
    assert [aggregator_id(EngineConfig(aggregator=a)) for a in AGGREGATORS] == [0, 1, 2]
    assert EngineConfig().aggregator == "mean" and EngineConfig().trim_ratio == 0.1
    with pytest.raises(ValueError, match="aggregator must be one of"):
        aggregator_id(EngineConfig(aggregator="krum"))
    for beta in (-0.1, 0.5, 0.7, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="trim_ratio"):
            aggregator_id(EngineConfig(aggregator="trimmed_mean", trim_ratio=beta))
    for agg in ("median", "trimmed_mean"):
        with pytest.raises(ValueError, match="differential privacy"):
            aggregator_id(EngineConfig(aggregator=agg, dp_clip=1.0))
    aggregator_id(EngineConfig(aggregator="mean", dp_clip=1.0))
    X, y = make_multiclass(40, 5, 2, DATA_SEED)
    flat = init_flat([5, 4, 2], 0)
    with pytest.raises(ValueError, match="differential privacy"):
        TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, aggregator="median", dp_clip=0.5, dp_seed=1),
                         None, flat)
    with pytest.raises(ValueError, match="aggregator must be one of"):
        TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, aggregator="mode"), None, flat)
    with pytest.raises(ValueError, match="at most 64 clients"):
        TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, aggregator="median"), SimRank(65, 0, "cpu"),
                         flat, n_total=65 * 40)
    # one client: the aggregate is the identity, the engine runs as under "mean"
    e = TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, aggregator="median"), None, flat)
    assert e.robust == 0 and e.run(2) == 2
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    with pytest.raises(ValueError, match="robust-aggregator"):
        FedTrialGroup(X, y, 2, [FedTrial((4,), 0.01, 1)], None, EngineConfig(max_rounds=2, aggregator="median"),
                      backend="torch")
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="robust aggregator"):
        WideClient(torch.zeros(4, 14), torch.zeros(4, dtype=torch.long), [14, 8, 2], aggregator="median")
    from fedmi.fl.engine import HipRoundEngine
    views = [torch.zeros(8), torch.zeros(8)]
    with pytest.raises(ValueError, match="comm_buffers"):   # refused before anything touches a device
        HipRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, aggregator="median"), None, flat,
                       comm_buffers=views)


# ---- groups ----
ROUNDS = 6
DIMS = [17, 24, 3]


def _group(agg, tamper=None, k=5, **kw):
    X, y = make_multiclass(96, 17, 3, DATA_SEED)
    cfg = EngineConfig(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, aggregator=agg,
                       trim_ratio=0.2, **kw)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, cfg, backend="torch", shard_mode="iid", seed=2, tamper=tamper)
    g.run(ROUNDS)
    return g


def _poison(value, n_img):
    def tamper(r, bufs):
        bufs[2][:n_img] = value
    return tamper


@pytest.mark.parametrize("agg", ["median", "trimmed_mean"])
def test_torch_group_survives_a_nan_client(agg):
    n = param_count(DIMS)
    a = _group(agg, _poison(float("nan"), n))
    b = _group(agg, _poison(float("inf"), n))
    wa, wb = a.global_flat(), b.global_flat()
    assert np.isfinite(wa).all()
    np.testing.assert_array_equal(wa, wb)      # NaN and +inf are trimmed alike at the top
    np.testing.assert_array_equal(a.history()["global"], b.history()["global"])
    clean = _group(agg)
    assert np.abs(wa - clean.global_flat()).max() > 0          # the tamper took effect
    for c in a.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), wa)
        np.testing.assert_array_equal(c.history()["global"], a.history()["global"])


def test_torch_group_mean_is_poisoned_by_the_same_client():
    g = _group("mean", _poison(float("nan"), param_count(DIMS)))
    assert not np.isfinite(g.global_flat()).any()


def test_trimmed_mean_beta_0_is_the_unweighted_mean():
    X, y = make_multiclass(96, 17, 3, DATA_SEED)
    seen = []
    torch.set_num_threads(1)
    cfg0 = EngineConfig(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0,
                        aggregator="trimmed_mean", trim_ratio=0.0)
    z = ClientGroup(X, y, 5, cfg0, backend="torch", shard_mode="iid", seed=2,
                    tamper=lambda r, bufs: seen.append(torch.stack([b[:param_count(DIMS)] for b in bufs]).clone()))
    z.run(1)
    st = seen[-1]
    acc = torch.zeros(st.shape[1])
    for k in range(5):
        acc = acc + st[k]
    np.testing.assert_array_equal(z.global_flat(), (acc / 5.0).numpy())


@pytest.mark.parametrize("participation", [1.0, 0.6])
def test_mean_is_bit_identical_to_the_default(participation):
    X, y = make_multiclass(96, 17, 3, DATA_SEED)
    out = []
    for kw in (dict(), dict(aggregator="mean", trim_ratio=0.3)):
        torch.set_num_threads(1)
        cfg = EngineConfig(hidden=(24,), max_rounds=ROUNDS + 2, graph_rounds=0, participation=participation, **kw)
        g = ClientGroup(X, y, 5, cfg, backend="torch", shard_mode="iid", seed=2)
        g.run(ROUNDS)
        out.append((g.global_flat(), g.history()["global"], g.history()["loss"]))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


def test_participation_excludes_unsampled_clients():
    # 3 of 5 sampled: a NaN client is cut whenever it is sampled (t = 1 for the median of 3)
    g = _group("median", _poison(float("nan"), param_count(DIMS)), participation=0.6)
    assert np.isfinite(g.global_flat()).all()
    lead = g.clients[0]
    assert any(2 in lead.participants(r) for r in range(ROUNDS)) and any(2 not in lead.participants(r) for r in range(ROUNDS))
    s = _group("median", None, participation=0.6, server_opt="adam", server_lr=1e-2)
    assert np.isfinite(s.global_flat()).all() and np.abs(s.clients[0].server_m.numpy()).max() > 0


# ---- three ranks over gloo ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_cfg():
    return EngineConfig(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, aggregator="median")


def _gloo_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    try:
        from fedmi.data.sharding import shard_indices
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="gloo", device="cpu")
        X, y = make_multiclass(96, 17, 3, DATA_SEED)
        idx = [shard_indices(len(X), r, world, mode="iid", seed=2, labels=y, alpha=0.5) for r in range(world)]
        e = TorchRoundEngine(X[idx[rank]], y[idx[rank]], 3, _rank_cfg(), comm, init_flat(DIMS, 2 * 1000003 + rank),
                             n_total=sum(len(i) for i in idx))
        e.run(ROUNDS)
        q.put((rank, (e.global_flat(), np.asarray(e.history()["global"]), np.asarray(e.history()["loss"])), None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_three_ranks_over_gloo_equal_the_torch_group_bitwise():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=120) for _ in range(3)], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    for rank, _, err in res:
        assert err is None, f"rank {rank}:\n{err}"
    X, y = make_multiclass(96, 17, 3, DATA_SEED)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, 3, _rank_cfg(), backend="torch", shard_mode="iid", seed=2)
    g.run(ROUNDS)
    ref = (g.global_flat(), g.history()["global"], g.history()["loss"])
    for rank, out, _ in res:
        for a, b in zip(out, ref):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank}")


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
    r = run("--clients", "3", "--rounds", "3", "--aggregator", "trimmed_mean", "--trim-ratio", "0.34")
    assert r.returncode == 0 and "3 simulated clients (torch): 3 rounds" in r.stdout, r.stderr[-2000:]
    for args, msg in ((("--aggregator", "median", "--wide"), "--aggregator is not supported with --wide"),
                      (("--aggregator", "trimmed_mean", "--trim-ratio", "0.5"), "trim_ratio"),
                      (("--aggregator", "median", "--dp-clip", "1.0"), "differential privacy")):
        r = run(*args)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr[-500:])

"""Differentially private FedAvg on the CPU: the Philox noise stream, the accountant, the torch
oracle's clipped + noised contribution, two ranks over gloo, and the fp32 oracle's own distance
from float64 on the end-to-end cases of tests/test_dp_fedavg.py.

Oracle noise on those cases (6 rounds, data seed 3, init seed 1): ``max|fp32 - fp64| / max|fp64|``
for weights, exp_avg and exp_avg_sq, ``max |fp32 - fp64| / |fp64|`` for the loss and the recorded
update norms.  The GPU test's bounds (2e-5 for weights and moments, 1e-4 for the loss) hold as long
as these stay within a quarter of them (5e-6, 2.5e-5), which this file asserts:

    case     z     weights   exp_avg   exp_avg_sq  loss      norm
    -------  ----  --------  --------  ----------  --------  --------
    income   0     5.6e-07   2.3e-07   2.7e-07     1.5e-07   1.3e-07
    income   0.02  5.4e-07   1.8e-07   2.5e-07     1.0e-07   1.3e-07
    steps2   0     1.2e-06   2.4e-07   3.1e-07     7.2e-08   8.5e-08
    steps2   0.02  7.7e-07   2.6e-07   3.6e-07     1.3e-07   6.1e-08
    small    0     4.0e-07   6.5e-08   2.3e-07     2.4e-08   2.6e-07
    small    0.02  1.9e-07   7.9e-08   9.3e-08     1.1e-07   2.6e-07
"""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.engine import EngineConfig, TorchRoundEngine
from fedmi.models.mlp import init_flat
from fedmi.privacy import accountant
from fedmi.privacy.philox import box_muller, dp_normals, philox4x32_10, u01

from .dp_oracle import (DP_CASES, DP_ROUNDS, DP_SEED, DP_Z, Float64DPOracle, assert_clip_decisions, contribution_f64)
from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr

EPS32 = 2.0 ** -24


# ---- Philox / Box-Muller ----
@pytest.mark.parametrize("ctr,key,out", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, out):
    """Random123's published Philox4x32-10 vectors."""
    got = philox4x32_10(np.asarray(ctr, np.uint32), key)
    assert " ".join(f"{int(x):08x}" for x in got) == out


def test_philox_vectorised_equals_one_by_one():
    ctr = np.stack([np.arange(5), np.full(5, 7), np.full(5, 1), np.full(5, 0x46454450)], 1)
    many = philox4x32_10(ctr, (3, 9))
    for i in range(5):
        np.testing.assert_array_equal(many[i], philox4x32_10(ctr[i], (3, 9)))


def test_u01_is_the_fp32_map_and_stays_positive():
    o = np.asarray([0, 255, 256, 0x7fffffff, 0x80000000, 0xffffffff], np.uint32)
    u = u01(o)
    assert u[0] == u[1] == 0.5 / 2 ** 24 and u[2] == 1.5 / 2 ** 24
    assert (u > 0).all() and (u <= 1).all()
    # below 1/2 the fp32 evaluation is exact; above, (o >> 8) + 0.5 rounds to 24 bits
    assert u[3] == (0x7fffff + 0.5) / 2 ** 24
    assert abs(u[5] - (0xffffff + 0.5) / 2 ** 24) <= 2.0 ** -25
    assert np.isfinite(box_muller(o[:4])).all() and np.isfinite(box_muller(o[2:])).all()


def test_dp_normals_stream_layout_and_moments():
    """Lane p % 4 of block p // 4; a prefix of a longer draw; rank and round change the stream;
    mean, variance and the correlation between two ranks of a standard normal sample."""
    a = dp_normals(4001, 3, 0, DP_SEED)
    np.testing.assert_array_equal(a[:1000], dp_normals(1000, 3, 0, DP_SEED))
    blk = box_muller(philox4x32_10([5, 3, 0, 0x46454450], (DP_SEED & 0xffffffff, DP_SEED >> 32)))
    np.testing.assert_array_equal(a[20:24], blk)
    b = dp_normals(4001, 3, 1, DP_SEED)
    n = a.size
    assert abs(a.mean()) < 5 / math.sqrt(n) and abs(a.var() - 1) < 5 * math.sqrt(2 / n)
    assert abs(np.corrcoef(a, b)[0, 1]) < 5 / math.sqrt(n)
    assert abs(np.corrcoef(a, dp_normals(4001, 4, 0, DP_SEED))[0, 1]) < 5 / math.sqrt(n)
    assert abs(np.corrcoef(a, dp_normals(4001, 3, 0, DP_SEED + 1))[0, 1]) < 5 / math.sqrt(n)


# ---- accountant ----
def test_accountant_grid_minimum_is_the_closed_form():
    """z = 1, T = 60, delta = 1e-5 -> 67.169.  The grid can only sit above the closed-form minimum,
    by at most sqrt(A B) e^2 with A = T / (2 z^2), B = ln(1 / delta) and e the half-step of the
    default geometric grid of alpha - 1 (8 decades over 20000 steps)."""
    z, T, delta = 1.0, 60, 1e-5
    closed = accountant.epsilon_closed_form(z, T, delta)
    grid = accountant.epsilon_rdp(z, T, delta)
    assert abs(closed - 67.169) < 1e-3
    e = 0.5 * (10 ** (8 / 20000) - 1)
    slack = math.sqrt(T / (2 * z * z) * math.log(1 / delta)) * e * e
    print(closed, grid, grid - closed, slack)
    assert 0 <= grid - closed <= 1.01 * slack + 1e-12


def test_accountant_is_monotone():
    eps = [accountant.epsilon_closed_form(1.0, T, 1e-5) for T in (1, 10, 60, 300)]
    assert eps == sorted(eps) and len(set(eps)) == 4
    eps = [accountant.epsilon_closed_form(z, 60, 1e-5) for z in (4.0, 2.0, 1.0, 0.5, 0.1)]
    assert eps == sorted(eps) and len(set(eps)) == 5
    eps = [accountant.epsilon_rdp(z, 60, 1e-5) for z in (4.0, 2.0, 1.0, 0.5)]
    assert eps == sorted(eps)
    assert accountant.epsilon_closed_form(0.0, 5, 1e-5) == math.inf
    assert accountant.epsilon_closed_form(1.0, 0, 1e-5) == 0.0
    with pytest.raises(ValueError):
        accountant.epsilon_closed_form(1.0, 5, 0.0)
    s = accountant.privacy_statement(1.0, 60, 1e-5)
    assert "67.17" in s and "1e-05" in s and "60 rounds" in s
    assert "client-level, no subsampling amplification" in s


# ---- configuration ----
@pytest.mark.parametrize("kw", [dict(dp_noise=0.5), dict(dp_clip=-1.0), dict(dp_clip=1.0, dp_noise=-0.1),
                                dict(dp_clip=float("nan")), dict(dp_clip=1.0, dp_seed=-1),
                                dict(dp_clip=1.0, dp_seed=2 ** 64)])
def test_invalid_dp_config_raises(kw):
    X, y = make_multiclass(40, 5, 2, DATA_SEED)
    with pytest.raises(ValueError):
        TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, **kw), None, init_flat([5, 4, 2], 0))


def test_fed_sweep_refuses_dp():
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    X, y = make_multiclass(40, 5, 2, DATA_SEED)
    with pytest.raises(ValueError, match="differentially private"):
        FedTrialGroup(X, y, 2, [FedTrial((4,), 0.01, 1)], None, EngineConfig(max_rounds=2, dp_clip=0.5),
                      backend="torch")


# ---- torch engine, one client ----
def _income_engine(**kw):
    X, y = make_multiclass(300, 14, 2, DATA_SEED)
    cfg = EngineConfig(max_rounds=6, early_stop=False, **kw)
    return TorchRoundEngine(X, y, 2, cfg, None, init_flat([14, 50, 200, 2], INIT_SEED))


def test_torch_contribution_is_the_formula():
    """Rounds 0 (clipped at S = 0.4) and 1 (not clipped): the contribution is w (x + c D) + sigma n
    recomputed in float64 with the host normals, to a few fp32 roundings of its terms; its length
    is the non-DP length (P weights + the metric tail)."""
    S, z = 0.4, 0.5
    e = _income_engine(dp_clip=S, dp_noise=z, dp_seed=DP_SEED)
    plain = _income_engine()
    clipped = []
    for r in range(2):
        x = e.global_flat()
        e.step_train()
        e.step_eval()
        local = e.local_flat()
        buf = e.fedavg_contribution()
        plain.step_train()
        plain.step_eval()
        assert buf.shape == plain.fedavg_contribution().shape == (e.P + e.tail_stride,)
        nrm = dp_normals(e.P, r, 0, DP_SEED)
        sigma = float(np.float32(z * S))
        assert float(e.dp_sigma[r]) == sigma
        want, norm, c = contribution_f64(local, x, 1.0, S, sigma, nrm)
        clipped.append(c < 1.0)
        tol = 4 * EPS32 * (np.abs(x) + np.abs(local) + np.abs(sigma * nrm)) + 1e-30
        assert np.all(np.abs(buf[:e.P].numpy().astype(np.float64) - want) <= tol)
        e.fedavg_apply(buf)
        plain.step_aggregate()
        assert abs(e.history()["update_norm"][r] - norm) <= 2 * EPS32 * norm
        # the local model is the un-noised, un-clipped one; the global is the contribution
        np.testing.assert_array_equal(e.global_flat(), buf[:e.P].numpy())
    assert clipped == [True, False]


def test_huge_clip_without_noise_is_the_plain_run_bitwise():
    a, b = _income_engine(dp_clip=1e9), _income_engine()
    a.run(4)
    b.run(4)
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    np.testing.assert_array_equal(a.history()["loss"], b.history()["loss"])
    np.testing.assert_array_equal(a.history()["global"], b.history()["global"])
    assert "update_norm" in a.history() and "update_norm" not in b.history()
    assert (a.history()["update_norm"] > 0).all() and a.history()["update_norm"].shape == (4,)


def test_private_seed_is_drawn_and_travels_with_the_state():
    a, b = _income_engine(dp_clip=0.37, dp_noise=0.1), _income_engine(dp_clip=0.37, dp_noise=0.1)
    assert a.dp_seed != b.dp_seed and 0 <= a.dp_seed < 2 ** 64
    a.run(2)
    st = a.portable_state()
    assert st["dp_seed"] == a.dp_seed
    b.load_portable_state(st)
    assert b.dp_seed == a.dp_seed
    a.run(2)
    b.run(2)
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    np.testing.assert_array_equal(a.history()["update_norm"], b.history()["update_norm"])
    assert "dp_seed" not in _income_engine().portable_state()


# ---- two ranks over gloo ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from fedmi.parallel.comm import Comm
    from fedmi.parallel.consistency import check_replicas
    comm = Comm(backend="gloo", device="cpu")
    X, y = make_multiclass(300 + 100 * rank, 14, 2, DATA_SEED + rank)   # unequal shards: max w = 0.5714
    cfg = EngineConfig(max_rounds=4, early_stop=False, dp_clip=0.3, dp_noise=0.5, dp_seed=DP_SEED)
    e = TorchRoundEngine(X, y, 2, cfg, comm, init_flat([14, 50, 200, 2], INIT_SEED + rank))
    x = e.global_flat()
    e.step_train()
    e.step_eval()
    local = e.local_flat()
    buf = e.fedavg_contribution()[:e.P].numpy().copy()
    e.step_aggregate()
    e.run(2)
    ok = check_replicas(comm, [e.global_flat(), np.asarray(e.history()["global"])])
    q.put((rank, len(X), x, local, buf, e.global_flat(), [float(s) for s in e.dp_sigma], ok,
           e.history()["update_norm"]))
    comm.close()


def test_two_ranks_over_gloo_share_one_noised_model():
    """z > 0 over gloo: every rank ends with the same global model (check_replicas), each rank's
    noise vector is its own stream, sigma follows the LARGER client's weight on both ranks, and the
    first global model is the sum of the two contributions."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    sizes = [r[1] for r in res]
    sigma = float(np.float32(0.5 * 0.3 * (max(sizes) / sum(sizes)) / math.sqrt(2)))
    xi = []
    for rank, n, x, local, buf, g, sig, ok, norms in res:
        assert ok is True or ok == True  # noqa: E712 -- check_replicas' verdict
        assert sig == [sigma] * 4
        w = n / sum(sizes)
        clean, norm, c = contribution_f64(local, x, w, 0.3, 0.0, None)
        assert c < 1.0 and abs(norms[0] - norm) <= 2 * EPS32 * norm
        xi.append(buf.astype(np.float64) - clean)
        want = dp_normals(x.size, 0, rank, DP_SEED) * sigma
        assert np.all(np.abs(xi[-1] - want) <= 4 * EPS32 * (np.abs(clean) + np.abs(want)) + 1e-30)
        np.testing.assert_array_equal(g, res[0][5])
    P = xi[0].size
    assert abs(np.corrcoef(xi[0], xi[1])[0, 1]) < 5 / math.sqrt(P)
    assert not np.array_equal(xi[0], xi[1])


# ---- oracle noise on the end-to-end cases ----
def dp_oracle_noise(case, z):
    rows, F, C, hidden, S, kw = DP_CASES[case]
    S = S[z]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    flat = init_flat([F, *hidden, C], INIT_SEED)
    cfg = EngineConfig(hidden=hidden, max_rounds=DP_ROUNDS + 2, graph_rounds=0, early_stop=False, dp_clip=S,
                       dp_noise=z, dp_seed=DP_SEED, **kw)
    ref = TorchRoundEngine(X, y, C, cfg, None, flat)
    ref.run(DP_ROUNDS)
    f64 = Float64DPOracle(X, y, C, cfg, flat, DP_SEED)
    f64.run(DP_ROUNDS)
    w, m, v, loss = f64.result()
    st = ref.portable_state()
    l32 = ref.history()["loss"].astype(np.float64)
    n32 = ref.history()["update_norm"].astype(np.float64)
    n64 = np.asarray(f64.norms)
    return ({"weights": nerr(ref.global_flat(), w), "exp_avg": nerr(st["exp_avg"], m),
             "exp_avg_sq": nerr(st["exp_avg_sq"], v), "loss": float(np.max(np.abs(l32 - loss) / np.abs(loss))),
             "norm": float(np.max(np.abs(n32 - n64) / n64))}, n32, n64, S)


@pytest.mark.parametrize("z", [0.0, DP_Z])
@pytest.mark.parametrize("case", sorted(DP_CASES))
def test_fp32_dp_oracle_is_within_a_quarter_of_the_gpu_bound(case, z):
    e, n32, n64, S = dp_oracle_noise(case, z)
    print(case, z, e, np.round(n32, 4))
    assert_clip_decisions(n32, S)
    assert_clip_decisions(n64, S)
    assert e["weights"] <= 5e-6, e
    assert e["exp_avg"] <= 5e-6, e
    assert e["exp_avg_sq"] <= 5e-6, e
    assert e["loss"] <= 2.5e-5, e
    assert e["norm"] <= 5e-6, e


# ---- checkpoints and the [C] entry point ----
def test_checkpoint_keeps_the_private_seed_and_norms(tmp_path):
    from fedmi.ckpt.checkpoint import resume, save_checkpoint
    a = _income_engine(dp_clip=0.37, dp_noise=0.1)
    a.run(3)
    save_checkpoint(str(tmp_path), a)
    b = _income_engine(dp_clip=0.37, dp_noise=0.1)
    assert resume(str(tmp_path), b) == 3 and b.dp_seed == a.dp_seed
    a.run(2)
    b.run(2)
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    np.testing.assert_array_equal(a.history()["update_norm"], b.history()["update_norm"])


def _run_c(args):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py"),
                        "--device", "cpu", "--backend", "gloo", "--engine", "torch", "--quiet", *args],
                       cwd=root, capture_output=True, text=True, timeout=300, env=env)
    return r


def test_entrypoint_dp_flags(tmp_path):
    import json
    r = _run_c(["--rounds", "3", "--no-early-stop", "--dp-clip", "0.2", "--dp-noise", "1.0", "--dp-seed", "5",
                "--jsonl", str(tmp_path / "m.jsonl")])
    assert r.returncode == 0, r.stderr[-2000:]
    eps = accountant.epsilon_closed_form(1.0, 3, 1e-5)
    last = r.stdout.strip().splitlines()[-1]
    assert f"epsilon = {eps:.4g} at delta = 1e-05 over 3 rounds" in last
    assert "client-level, no subsampling amplification" in last
    rows = [json.loads(l) for l in open(tmp_path / "m.jsonl")]
    assert len(rows) == 3 and all(row["update_norm"] > 0.2 for row in rows)
    r = _run_c(["--clients", "2", "--rounds", "2", "--no-early-stop", "--dp-clip", "0.2", "--dp-noise", "0.5",
                "--dp-delta", "1e-6"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "at delta = 1e-06 over 2 rounds" in r.stdout.strip().splitlines()[-1]
    r = _run_c(["--rounds", "2", "--dp-noise", "0.5"])
    assert r.returncode != 0 and "--dp-noise needs --dp-clip" in r.stderr


def test_api_doc_example():
    """docs/API.md "Differential privacy", one client on the torch engine."""
    from fedmi.data.tabular import load_tabular
    from fedmi.fl.trainer import FederatedMLPLearning
    ds = load_tabular(with_mean=True)
    cfg = EngineConfig(dp_clip=0.2, dp_noise=1.0)
    fl = FederatedMLPLearning(ds.X_train, ds.y_train, 0, 1, comm=None, config=cfg, backend="torch")
    fl.train_and_evaluate(None, rounds=3, verbose=False)
    assert fl.history()["update_norm"].shape == (3,) and (fl.history()["update_norm"] > 0.2).all()
    assert abs(accountant.epsilon_closed_form(1.0, rounds=60, delta=1e-5) - 67.17) < 5e-3

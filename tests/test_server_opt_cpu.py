"""Server optimizers (FedAvgM, FedAdagrad, FedAdam, FedYogi) on the CPU: field validation, the fp32
torch engine against the float64 oracle, two ranks over gloo, client groups, checkpoints, the [C]
entry point, and the untouched defaults.

fp32 torch engine against tests/server_oracle.Float64ServerOracle, six rounds, data seed 3, init seed
1, ``max|fp32 - fp64| / max|fp64|`` (measured):

    shape   opt      weights  server_m  server_v
    income  sgd      4.3e-06  1.2e-05   -
    income  adagrad  6.8e-07  1.5e-05   1.2e-05
    income  adam     1.4e-06  8.5e-06   5.5e-06
    income  yogi     1.4e-06  1.3e-05   5.5e-06
    small   sgd      1.5e-06  5.4e-06   -
    small   adagrad  1.0e-07  2.0e-06   3.5e-06
    small   adam     2.4e-07  2.0e-06   1.3e-06
    small   yogi     3.9e-07  2.1e-06   1.3e-06

Bounds.  Weights: 5e-6, a quarter of the project's 2e-5 for a second fp32 implementation, as in
tests/test_dp_cpu.py.  Server state: the pseudo-gradient d = a - x is the difference of two images
that each carry the weights' error E = 5e-6 max|w|, so |err d| <= 2 E.  m is a combination of the
d's with coefficients that sum to at most 1 / (1 - b1) = 10 (sgd) or 1 (adaptive): err m <= 10 * 2 E
resp. 2 E, asserted relative to max|m|.  v adds (a multiple <= 1 of) d^2 per round, whose error is
<= 2 |d| 2 E + (2 E)^2 with |d| <= dmax = the largest pseudo-gradient component seen; over R rounds
err v <= R (4 dmax E + 4 E^2), asserted relative to max|v|.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.engine import EngineConfig, TorchRoundEngine
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr
from .server_oracle import (OPTS, SERVER_KW, SERVER_ROUNDS, SERVER_SHAPES, Float64ServerOracle, server_cfg,
                            server_step_f64, shape_data)


def _engine(opt, shape="income", **kw):
    X, y, C, flat = shape_data(shape)
    return TorchRoundEngine(X, y, C, server_cfg(opt, shape, **kw), None, flat)


# ---- configuration ----
@pytest.mark.parametrize("kw", [dict(server_opt="fedadam"), dict(server_opt="sgd", server_lr=0.0),
                                dict(server_opt="sgd", server_lr=float("inf")), dict(server_opt="adam", server_lr=-1.0),
                                dict(server_opt="sgd", server_momentum=1.0), dict(server_opt="sgd", server_momentum=-0.1),
                                dict(server_opt="adam", server_beta2=1.0), dict(server_opt="yogi", server_beta2=-0.5),
                                dict(server_opt="adagrad", server_tau=0.0), dict(server_opt="adam", server_tau=-1e-3),
                                dict(server_lr=float("nan"))])
def test_invalid_server_config_raises(kw):
    X, y = make_multiclass(40, 5, 2, DATA_SEED)
    with pytest.raises(ValueError, match="server_"):
        TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, **kw), None, init_flat([5, 4, 2], 0))


def test_sgd_accepts_any_tau_and_refusals_name_the_field():
    X, y = make_multiclass(40, 5, 2, DATA_SEED)
    TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, server_opt="sgd", server_tau=0.0), None,
                     init_flat([5, 4, 2], 0))
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    with pytest.raises(ValueError, match="server-optimizer"):
        FedTrialGroup(X, y, 2, [FedTrial((4,), 0.01, 1)], None, EngineConfig(max_rounds=2, server_opt="adam"),
                      backend="torch")


# ---- fp32 torch engine against the float64 oracle ----
@pytest.mark.parametrize("shape", sorted(SERVER_SHAPES))
@pytest.mark.parametrize("opt", OPTS)
def test_torch_engine_matches_float64_oracle(opt, shape):
    X, y, C, flat = shape_data(shape)
    cfg = server_cfg(opt, shape)
    e = TorchRoundEngine(X, y, C, cfg, None, flat)
    e.run(SERVER_ROUNDS)
    o = Float64ServerOracle(X, y, C, cfg, flat)
    o.run(SERVER_ROUNDS)
    st = e.portable_state()
    err = {"weights": nerr(e.global_flat(), o.weights()), "server_m": nerr(st["server_m"], o.server_m)}
    if opt != "sgd":
        err["server_v"] = nerr(st["server_v"], o.server_v)
    E = 5e-6 * np.abs(o.weights()).max()
    bound = {"weights": 5e-6, "server_m": (20 if opt == "sgd" else 2) * E / np.abs(o.server_m).max()}
    if opt != "sgd":
        bound["server_v"] = SERVER_ROUNDS * (4 * o.dmax * E + 4 * E * E) / np.abs(o.server_v).max()
    print(shape, opt, {k: f"{v:.2g}" for k, v in err.items()}, "bounds", {k: f"{v:.2g}" for k, v in bound.items()})
    for k in err:
        assert err[k] <= bound[k], (k, err, bound)
    # the step did something: the global model is not the local one, the state moved
    assert np.abs(e.global_flat() - e.local_flat()).max() == 0   # (torch: the model adopts the global)
    assert np.abs(st["server_m"]).max() > 0
    plain = TorchRoundEngine(X, y, C, EngineConfig(hidden=cfg.hidden, max_rounds=8, early_stop=False), None, flat)
    plain.run(SERVER_ROUNDS)
    assert nerr(plain.global_flat(), o.weights()) > 1e-3


def test_first_step_is_the_formula():
    """Round 0 from m = 0, v = tau^2, all four optimizers: the new global model is server_step_f64 of
    the engine's own (x, a) to a few fp32 roundings."""
    for opt in OPTS:
        e = _engine(opt)
        x = e.global_flat()
        e.step_train()
        e.step_eval()
        a = e.local_flat()
        e.step_aggregate()
        cfg = e.cfg
        m0 = np.zeros(e.P)
        v0 = None if opt == "sgd" else np.full(e.P, float(cfg.server_tau) ** 2)
        want, m, v = server_step_f64(x, a, m0, v0, cfg)
        got = e.global_flat().astype(np.float64)
        assert np.all(np.abs(got - want) <= 8 * 2.0 ** -24 * (np.abs(want) + np.abs(want - x)) + 1e-30), opt
        np.testing.assert_allclose(e.server_m.numpy(), m, rtol=4 * 2.0 ** -24, atol=1e-30)


def test_sgd_without_momentum_at_lr_1_is_fedavg_up_to_one_rounding():
    a, b = _engine("sgd", server_momentum=0.0), TorchRoundEngine(*shape_data("income")[:3], EngineConfig(
        max_rounds=8, early_stop=False), None, shape_data("income")[3])
    a.run(1)
    b.run(1)
    np.testing.assert_allclose(a.global_flat(), b.global_flat(), rtol=0, atol=2.0 ** -23 * np.abs(b.global_flat()).max())


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
    try:
        from fedmi.parallel.comm import Comm
        from fedmi.parallel.consistency import check_replicas
        comm = Comm(backend="gloo", device="cpu")
        X, y = make_multiclass(300 + 100 * rank, 14, 2, DATA_SEED + rank)
        out = {}
        for opt in ("sgd", "yogi"):
            e = TorchRoundEngine(X, y, 2, server_cfg(opt, max_rounds=4), comm,
                                 init_flat([14, 50, 200, 2], INIT_SEED))   # one common starting model
            e.run(3)
            ok = check_replicas(comm, [e.global_flat(), np.asarray(e.history()["global"])])
            out[opt] = (e.global_flat(), e.server_m.numpy().copy(), e.server_v.numpy().copy(), bool(ok))
        q.put((rank, out, None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_two_ranks_over_gloo_end_bitwise_equal():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    for rank, _, err in res:
        assert err is None, f"rank {rank}:\n{err}"
    for opt in ("sgd", "yogi"):
        (g0, m0, v0, ok0), (g1, m1, v1, ok1) = res[0][1][opt], res[1][1][opt]
        assert ok0 and ok1
        np.testing.assert_array_equal(g0, g1)
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(v0, v1)
        assert np.abs(m0).max() > 0


# ---- client groups ----
@pytest.mark.parametrize("participation", [1.0, 0.5])
def test_torch_client_group_steps_every_client_alike(participation):
    X, y = make_multiclass(1200, 14, 2, DATA_SEED)
    g = ClientGroup(X, y, 4, server_cfg("adam", participation=participation), backend="torch", shard_mode="iid", seed=2)
    g.run(3)
    lead = g.clients[0]
    assert np.abs(lead.server_m.numpy()).max() > 0
    for e in g.clients[1:]:   # sampled or not, every client holds the same server state and model
        np.testing.assert_array_equal(e.server_m.numpy(), lead.server_m.numpy())
        np.testing.assert_array_equal(e.server_v.numpy(), lead.server_v.numpy())
        np.testing.assert_array_equal(e.global_flat(), lead.global_flat())


# ---- checkpoints ----
def test_checkpoint_round_trip_and_mismatch_errors(tmp_path):
    from fedmi.ckpt.checkpoint import resume, save_checkpoint
    a = _engine("yogi")
    a.run(3)
    save_checkpoint(str(tmp_path / "s"), a)
    b = _engine("yogi")
    assert resume(str(tmp_path / "s"), b) == 3
    np.testing.assert_array_equal(b.server_m.numpy(), a.server_m.numpy())
    np.testing.assert_array_equal(b.server_v.numpy(), a.server_v.numpy())
    a.run(3)
    b.run(3)
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    np.testing.assert_array_equal(a.history()["loss"], b.history()["loss"])
    c = _engine("yogi")
    c.run(6)
    np.testing.assert_array_equal(c.global_flat(), b.global_flat())   # ... and equals the uninterrupted run
    X, y, C, flat = shape_data("income")
    plain = lambda: TorchRoundEngine(X, y, C, EngineConfig(max_rounds=8, early_stop=False), None, flat)
    with pytest.raises(ValueError, match="server optimizer"):
        resume(str(tmp_path / "s"), plain())
    p = plain()
    p.run(2)
    save_checkpoint(str(tmp_path / "p"), p)
    with pytest.raises(ValueError, match="server optimizer"):
        resume(str(tmp_path / "p"), _engine("sgd"))
    assert resume(str(tmp_path / "p"), plain()) == 2


# ---- defaults ----
def test_defaults_leave_state_and_history_keys_unchanged():
    cfg = EngineConfig()
    assert (cfg.server_opt, cfg.server_lr, cfg.server_momentum, cfg.server_beta2, cfg.server_tau) == \
        ("none", 1.0, 0.9, 0.99, 1e-3)
    X, y, C, flat = shape_data("small")
    e = TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=4, early_stop=False), None, flat)
    e.run(2)
    assert set(e.portable_state()) == {"rounds", "global", "local", "exp_avg", "exp_avg_sq", "opt_steps", "es",
                                       "history"}
    assert set(e.history()) == {"rounds_run", "stop_round", "stop_trigger", "global", "per_rank", "loss"}
    assert not hasattr(e, "server_m")
    s = _engine("sgd", "small")
    s.run(2)
    assert set(s.portable_state()) - set(e.portable_state()) == {"server_m", "server_v"}
    assert set(s.history()) == set(e.history())
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="server optimizer"):
        WideClient(torch.zeros(4, 14), torch.zeros(4, dtype=torch.long), [14, 8, 2], server_opt="sgd")


# ---- the [C] entry point ----
def _run_c(args):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(root, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py"),
                           "--device", "cpu", "--backend", "gloo", "--engine", "torch", "--quiet", *args],
                          cwd=root, capture_output=True, text=True, timeout=300, env=env)


def test_entrypoint_server_flags(tmp_path):
    import json
    base = ["--rounds", "3", "--no-early-stop"]
    r = _run_c([*base, "--jsonl", str(tmp_path / "plain.jsonl")])
    assert r.returncode == 0, r.stderr[-2000:]
    r = _run_c([*base, "--server-opt", "adam", "--server-lr", "0.01", "--server-momentum", "0.8", "--server-beta2",
                "0.95", "--server-tau", "0.01", "--jsonl", str(tmp_path / "adam.jsonl")])
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {k: [json.loads(l) for l in open(tmp_path / f"{k}.jsonl")] for k in ("plain", "adam")}
    assert len(rows["adam"]) == 3
    # round 0 scores the first local model either way; afterwards the runs differ
    assert rows["adam"][0]["loss"] == rows["plain"][0]["loss"] and rows["adam"][2]["loss"] != rows["plain"][2]["loss"]
    r = _run_c(["--clients", "2", *base, "--server-opt", "sgd", "--server-momentum", "0.5"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "2 simulated clients (torch): 3 rounds" in r.stdout
    r = _run_c([*base, "--wide", "--server-opt", "sgd"])
    assert r.returncode != 0 and "--server-opt is not supported with --wide" in r.stderr
    r = _run_c([*base, "--server-opt", "adam", "--server-tau", "0"])
    assert r.returncode != 0 and "server_tau" in r.stderr

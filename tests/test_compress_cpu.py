"""Update compression with error feedback on the CPU: the config fields and refusals, the host model
``compress_torch`` (selection, ties, NaN, the error-feedback identities), the telescoping sum in
float64, torch client groups at 17-24-3 (client sampling, early stop, checkpoints), the wire-size
accounting, the planner's COMPRESS launch kind and the [C] entry point's flags.
"""
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from fedmi.fl.compress import (COMPRESSORS, compress_id, compress_k, compress_round, compress_torch, sign_scale,
                               topk_count, topk_mask, uplink_bytes)
from fedmi.fl.engine import EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.fl.simulate import ClientGroup

from .server_oracle import shape_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_SMALL = 17 * 24 + 24 + 24 * 3 + 3   # 17-24-3: 507 parameters


def _bits(t):
    return torch.as_tensor(t, dtype=torch.float32).contiguous().numpy().view(np.uint32)


def _rand(P, seed=0):
    return torch.as_tensor(np.random.default_rng(seed).standard_normal(P).astype(np.float32))


# ---- config ----
def test_defaults():
    cfg = EngineConfig()
    assert (cfg.compress, cfg.compress_ratio, cfg.error_feedback) == ("none", 0.1, True)
    assert compress_id(cfg) == 0 and COMPRESSORS == ("none", "topk", "sign")
    assert compress_id(EngineConfig(compress="topk")) == 1 and compress_id(EngineConfig(compress="sign")) == 2
    assert compress_id(EngineConfig(compress="topk", compress_ratio=1.0)) == 1


@pytest.mark.parametrize("kw, field", [
    (dict(compress="top-k"), "compress"), (dict(compress="topk", compress_ratio=0.0), "compress_ratio"),
    (dict(compress="topk", compress_ratio=1.5), "compress_ratio"), (dict(compress_ratio=-0.1), "compress_ratio"),
    (dict(compress="topk", compress_ratio=float("nan")), "compress_ratio"),
    (dict(compress="sign", compress_ratio="a tenth"), "compress_ratio"),
    (dict(compress="sign", error_feedback=1), "error_feedback"),
    (dict(compress="topk", dp_clip=0.5, dp_seed=1), "dp_clip"), (dict(compress="sign", dp_clip=0.5, dp_seed=1), "dp_clip")])
def test_validation_names_the_field(kw, field):
    with pytest.raises(ValueError, match=field):
        compress_id(EngineConfig(**kw))
    X, y, C, flat = shape_data("small")
    with pytest.raises(ValueError, match=field):
        TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=2, **kw), None, flat)


def test_refusals():
    X, y, C, flat = shape_data("small")
    cfg = EngineConfig(hidden=(24,), max_rounds=2, compress="topk")
    bufs = (torch.zeros(8), torch.zeros(8))
    with pytest.raises(ValueError, match="compress"):   # trial batches hand every engine its comm buffers
        HipRoundEngine(X, y, C, cfg, None, flat, comm_buffers=bufs)
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    with pytest.raises(ValueError, match="compress"):
        FedTrialGroup(X, y, C, [FedTrial((4,), 0.01, 1)], None, EngineConfig(max_rounds=2, compress="sign"),
                      backend="torch")
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="compress"):
        WideClient(torch.zeros(4, 14), torch.zeros(4, dtype=torch.long), [14, 8, 2], compress="topk")


def test_k_and_wire_size():
    assert [topk_count(r, 507) for r in (1e-9, 0.001, 0.01, 0.1, 0.5, 1.0)] == [1, 1, 6, 51, 254, 507]
    assert topk_count(0.1, 11352) == 1136 and topk_count(0.01, 11352) == 114 and topk_count(1.0, 34) == 34
    assert compress_k(EngineConfig(compress="topk", compress_ratio=0.01), 11352) == 114
    assert compress_k(EngineConfig(compress="sign"), 11352) == 11352 and compress_k(EngineConfig(), 34) == 34
    assert uplink_bytes("topk", 1136, 11352) == 8 * 1136
    assert uplink_bytes("sign", 11352, 11352) == 4 + 1419 and uplink_bytes("sign", 34, 34) == 4 + 5
    assert uplink_bytes("none", 11352, 11352) == 4 * 11352
    with pytest.raises(ValueError, match="compress"):
        uplink_bytes("dense", 1, 1)
    X, y, C, flat = shape_data("small")
    e = TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=2, compress="topk"), None, flat)
    assert e.P == P_SMALL and e.compress_k == 51 and e.uplink_bytes() == 408
    d = TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=2), None, flat)
    assert d.uplink_bytes() == 4 * P_SMALL


# ---- compress_torch ----
@pytest.mark.parametrize("P", [34, 507, 11352])
@pytest.mark.parametrize("k", ["one", "tenth", "all"])
def test_topk_keeps_exactly_k_and_splits_u(P, k):
    k = {"one": 1, "tenth": topk_count(0.1, P), "all": P}[k]
    u = _rand(P, P)
    c, e, stat = compress_torch(u, "topk", k)
    kept = c != 0
    assert int(kept.sum()) == k and c.dtype == torch.float32
    np.testing.assert_array_equal(_bits(c + e), _bits(u))                  # c + e' == u, bitwise
    np.testing.assert_array_equal(_bits(c)[kept.numpy()], _bits(u)[kept.numpy()])
    assert not e[kept].any() and torch.equal(e[~kept], u[~kept])
    mags = np.sort(np.abs(u.numpy()))[::-1]
    assert stat == float(mags[k - 1]) and float(u[kept].abs().min()) == stat
    if k < P:
        assert float(u[~kept].abs().max()) <= stat
    c0, e0, _ = compress_torch(u, "topk", k, error_feedback=False)
    assert torch.equal(c0, c) and not e0.any()


def test_topk_ties_keep_the_lowest_indices():
    P, k = 507, 100
    u = torch.full((P,), 0.25) * torch.as_tensor(np.where(np.arange(P) % 3 == 0, -1.0, 1.0), dtype=torch.float32)
    kept = topk_mask(u, k)        # all magnitudes equal, mixed signs
    assert kept[:k].all() and not kept[k:].any()
    c, e, stat = compress_torch(u, "topk", k)
    assert torch.equal(c[:k], u[:k]) and not c[k:].any() and torch.equal(e[k:], u[k:]) and stat == 0.25
    # more exact zeros (of both signs) than P - k: the cut falls among the zeros
    u = torch.zeros(P)
    u[1::2] = -0.0
    big = [500, 3, 77]
    u[big] = torch.tensor([2.0, -3.0, 1.0])
    kept = topk_mask(u, 10)
    want = sorted(big + [0, 1, 2, 4, 5, 6, 7])
    assert torch.nonzero(kept).reshape(-1).tolist() == want
    c, e, stat = compress_torch(u, "topk", 10)
    assert stat == 0.0 and int((c != 0).sum()) == 3
    np.testing.assert_array_equal(_bits(c)[want], _bits(u)[want])          # a kept -0 stays -0
    np.testing.assert_array_equal(_bits(c + e)[~kept.numpy()], _bits(u + 0.0)[~kept.numpy()])


def test_nan_ranks_first_and_inf_second():
    u = _rand(507, 3)
    u[400] = float("nan")
    u[17] = float("-inf")
    assert torch.nonzero(topk_mask(u, 1)).reshape(-1).tolist() == [400]
    assert torch.nonzero(topk_mask(u, 2)).reshape(-1).tolist() == [17, 400]
    c, e, stat = compress_torch(u, "topk", 1)
    assert math.isnan(float(c[400])) and e[400] == 0 and math.isnan(stat) and not c[:400].any()
    _, _, stat2 = compress_torch(u, "topk", 2)
    assert stat2 == math.inf


@pytest.mark.parametrize("P", [34, 507, 11352])
def test_sign(P):
    u = _rand(P, P + 1)
    u[0] = 0.0
    u[1] = -0.0
    c, e, s = compress_torch(u, "sign")
    s32 = np.float32(s)
    assert s == float(sign_scale(u)) and (c.abs() == float(s32)).all()
    np.testing.assert_array_equal(_bits(c) >> 31, _bits(u) >> 31)          # copysign, -0 included
    np.testing.assert_array_equal(_bits(e), _bits(u - c))                  # e' == fsub(u, c)
    # the fixed-order fp32 sum against the float64 mean: (ceil(P / 1024) + 6 + 16 + 1) roundings
    ref = float(u.double().abs().sum()) / P
    assert abs(s - ref) <= ((P + 1023) // 1024 + 23) * 2.0 ** -24 * ref
    c2, e2, s2 = compress_torch(u, "sign", s=0.5)
    assert s2 == 0.5 and (c2.abs() == 0.5).all() and torch.equal(e2, u - c2)
    _, e0, _ = compress_torch(u, "sign", error_feedback=False)
    assert not e0.any()


def test_compress_round_is_the_rule():
    P = 507
    local, x, e = _rand(P, 1), _rand(P, 2), 0.01 * _rand(P, 3)
    w = float(np.float32(0.3))
    u = (local - x) + e
    for kind, k in (("topk", 51), ("sign", P)):
        c, en, stat = compress_torch(u, kind, k)
        out, en2, stat2 = compress_round(local, x, e, w, kind, k)
        np.testing.assert_array_equal(_bits(out), _bits(torch.tensor(w) * (x + c)))
        assert torch.equal(en, en2) and stat == stat2


# ---- telescoping in float64 ----
@pytest.mark.parametrize("kind", ["topk", "sign"])
def test_error_feedback_telescopes_in_float64(kind):
    """Along six rounds of a torch client the rule, carried in float64 on the client's own (local, x)
    pairs, loses nothing: sum_r c_r + e_R == sum_r (local_r - x_r) to 1e-12 relative."""
    X, y, C, flat = shape_data("small")
    eng = TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=8, early_stop=False, compress=kind), None, flat)
    k = eng.compress_k
    e = torch.zeros(eng.P, dtype=torch.float64)
    sum_c = torch.zeros(eng.P, dtype=torch.float64)
    sum_d = torch.zeros(eng.P, dtype=torch.float64)
    for r in range(6):
        eng.step_train()
        eng.step_eval()
        local, x = eng.model.flat.detach().double().clone(), eng._dp_input.double()
        eng.step_aggregate()
        d = local - x
        assert d.abs().max() > 0
        c, e, _ = compress_torch(d + e, kind, k)
        assert c.dtype == torch.float64
        sum_c += c
        sum_d += d
    err = float((sum_c + e - sum_d).abs().max()) / float(sum_d.abs().max())
    print(kind, "telescoping error, relative", err, "residual share", float(e.abs().max() / sum_d.abs().max()))
    assert err <= 1e-12
    assert float(e.abs().max()) > 0      # something was carried
    # ... and without error feedback what is dropped is lost
    _, e0, _ = compress_torch(sum_d, kind, k, error_feedback=False)
    assert not e0.any()


# ---- torch engines and groups at 17-24-3 ----
def _group(rounds=6, **kw):
    X, y, _, _ = shape_data("small")
    cfg = EngineConfig(**{**dict(hidden=(24,), max_rounds=rounds + 2, early_stop=False), **kw})
    return ClientGroup(X, y, 4, cfg, backend="torch")


@pytest.mark.parametrize("kind", ["topk", "sign"])
def test_torch_client_follows_the_rule_bitwise(kind):
    """One client of a group, step by step: contribution, residual and statistic are compress_round of
    the engine's own local model, round input and residual (two local steps, weight n_i / N)."""
    g = _group(compress=kind, local_steps=2)
    for r in range(4):
        for e in g.clients:
            e.step_train()
            e.step_eval()
        snap = [(e.model.flat.detach().clone(), e._dp_input.clone(), e.compress_residual.clone()) for e in g.clients]
        bufs = [e.fedavg_contribution() for e in g.clients]
        for e, (local, x, res), buf in zip(g.clients, snap, bufs):
            out, en, stat = compress_round(local, x, res, e.agg_scale, kind, e.compress_k)
            np.testing.assert_array_equal(_bits(buf[:e.P]), _bits(out))
            np.testing.assert_array_equal(_bits(e.compress_residual), _bits(en))
            assert e.hist.cstat[r] == np.float32(stat) and stat > 0
            assert torch.equal(e.fedavg_contribution(), buf)       # asking twice compresses once
            assert torch.equal(e.model.flat.detach(), local)       # the local model is not touched
        tot = bufs[0].clone()
        for b in bufs[1:]:
            tot += b
        for e in g.clients:
            e.fedavg_apply(tot.clone())
    h = g.history()
    assert h["compress_stat"].shape == (4,) and (h["compress_stat"] > 0).all()


def test_unsampled_client_keeps_residual_and_stat():
    g = _group(compress="topk", participation=0.5)
    lead = g.clients[0]
    seen = {True: 0, False: 0}
    for r in range(6):
        before = [e.compress_residual.clone() for e in g.clients]
        g.run(1)
        part = set(lead.participants(r).tolist())
        for e, b in zip(g.clients, before):
            active = e.rank in part
            seen[active] += 1
            if active:
                assert not torch.equal(e.compress_residual, b) and e.hist.cstat[r] > 0
            else:
                np.testing.assert_array_equal(_bits(e.compress_residual), _bits(b))
                assert e.hist.cstat[r] == 0
    assert seen[True] == 12 and seen[False] == 12


@pytest.mark.parametrize("kw", [dict(compress="topk", server_opt="adam", server_lr=1e-2),
                                dict(compress="sign", aggregator="median"),
                                dict(compress="topk", prox_mu=0.1, local_steps=2),
                                dict(compress="sign", error_feedback=False)])
def test_compositions_run_and_stay_replicated(kw):
    g = _group(**kw)
    g.run(6)
    ref = g.clients[0].global_flat()
    assert np.isfinite(ref).all()
    for e in g.clients[1:]:
        np.testing.assert_array_equal(e.global_flat(), ref)
    if kw.get("error_feedback", True):
        assert all(float(e.compress_residual.abs().max()) > 0 for e in g.clients)
    else:
        assert not any(e.compress_residual.any() for e in g.clients)
    dense = _group(**{k: v for k, v in kw.items() if k not in ("compress", "error_feedback")})
    dense.run(6)
    assert np.abs(dense.global_flat() - ref).max() > 0     # the compressor changed the trajectory
    assert "compress_stat" not in dense.history() and "compress_residual" not in dense.clients[0].portable_state()


def test_full_topk_is_dense_up_to_rounding():
    a, b = _group(compress="topk", compress_ratio=1.0), _group()
    a.run(6)
    b.run(6)
    err = np.abs(a.global_flat() - b.global_flat()).max() / np.abs(b.global_flat()).max()
    print("top-k at ratio 1 vs dense, torch group, 6 rounds:", err)
    assert err < 1e-4 and not any(e.compress_residual.any() for e in a.clients)


def test_rounds_past_an_early_stop_change_nothing():
    g = _group(rounds=38, compress="topk", early_stop=True, patience=2, tolerance=0.5)
    ran = g.run(40)
    h = g.history()
    assert g.stopped and ran == h["rounds_run"] == h["stop_round"] < 40
    res = [e.compress_residual.clone() for e in g.clients]
    flat, stat = g.global_flat(), h["compress_stat"].copy()
    assert g.run(5) == 0
    for e, b in zip(g.clients, res):
        np.testing.assert_array_equal(_bits(e.compress_residual), _bits(b))
    np.testing.assert_array_equal(g.global_flat(), flat)
    np.testing.assert_array_equal(g.history()["compress_stat"], stat)


@pytest.mark.parametrize("kind", ["topk", "sign"])
def test_checkpoint_round_trip_and_mismatch_errors(tmp_path, kind):
    from fedmi.ckpt.checkpoint import resume, save_checkpoint
    X, y, C, flat = shape_data("small")
    mk = lambda **kw: TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=8, early_stop=False, **kw), None,
                                       flat)
    a = mk(compress=kind)
    a.run(3)
    save_checkpoint(str(tmp_path / "s"), a)
    b = mk(compress=kind)
    assert resume(str(tmp_path / "s"), b) == 3
    np.testing.assert_array_equal(_bits(b.compress_residual), _bits(a.compress_residual))
    assert float(a.compress_residual.abs().max()) > 0
    a.run(3)
    b.run(3)
    c = mk(compress=kind)
    c.run(6)                                                   # ... and equals the uninterrupted run
    for e in (a, b):
        np.testing.assert_array_equal(e.global_flat(), c.global_flat())
        np.testing.assert_array_equal(_bits(e.compress_residual), _bits(c.compress_residual))
        np.testing.assert_array_equal(e.history()["compress_stat"], c.history()["compress_stat"])
    with pytest.raises(ValueError, match="compress"):
        resume(str(tmp_path / "s"), mk())
    p = mk()
    p.run(2)
    save_checkpoint(str(tmp_path / "p"), p)
    with pytest.raises(ValueError, match="compress"):
        resume(str(tmp_path / "p"), mk(compress=kind))
    assert resume(str(tmp_path / "p"), mk()) == 2
    st = a.portable_state()
    st["compress_residual"] = st["compress_residual"][:-1]
    with pytest.raises(ValueError, match="residual"):
        mk(compress=kind).load_portable_state(st)


# ---- the planner ----
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_compress_plans_under_asan_ubsan(tmp_path):
    """tests/native/test_compress_plan.cpp: with compress_on the plans hold one COMPRESS record per round
    where DP's would sit; with it off they are record for record the golden ones."""
    exe = str(tmp_path / "test_compress_plan")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           "-I" + os.path.join(ROOT, "tests", "native"), os.path.join(ROOT, "tests", "native", "test_compress_plan.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    golden = os.path.join(ROOT, "tests", "golden", "round_plans.json")
    r = subprocess.run([exe, golden], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sequences checked: 86" in r.stdout and "failures: 0" in r.stdout
    assert "compress plan failures: 0\n" in r.stdout


# ---- the [C] entry point ----
def _run_c(args):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py"),
                           "--device", "cpu", "--backend", "gloo", "--engine", "torch", "--quiet", *args],
                          cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)


def test_entry_point_flags(tmp_path):
    out = str(tmp_path / "rows.jsonl")
    r = _run_c(["--clients", "2", "--rounds", "2", "--no-early-stop", "--hidden", "8", "--compress", "topk",
                "--compress-ratio", "0.25", "--no-error-feedback", "--jsonl", out])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [json.loads(line) for line in open(out)]
    P = 14 * 8 + 8 + 8 * 2 + 2
    assert len(rows) == 2 and all(row["uplink_bytes"] == 8 * math.ceil(0.25 * P) for row in rows)
    assert all(row["compress_stat"] > 0 for row in rows)
    r = _run_c(["--wide", "--compress", "sign"])
    assert r.returncode != 0 and "--compress is not supported with --wide" in r.stderr
    r = _run_c(["--compress", "topk", "--compress-ratio", "0"])
    assert r.returncode != 0 and "compress_ratio" in r.stderr

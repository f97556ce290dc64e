"""The stochastic update compressors on the CPU: the config fields, the wire-size accounting, the host
model ``compress_torch`` for ``"qsgd"`` (levels, sign, error bound, unbiasedness over fixed seeds) and
``"randk"`` (selection, gain), the random stream, the telescoping sum in float64, and torch client
groups at 17-24-3 (repeatability, resume, state mismatches), and the [C] entry point's flags.
"""
import math

import numpy as np
import pytest
import torch

from fedmi.fl.compress import (ALL_COMPRESSORS, COMPRESSORS, RANDOM_COMPRESSORS, compress_id, compress_k,
                               compress_round, compress_torch, compress_words, ordered_sum, qsgd_levels, qsgd_norm,
                               randk_keys, randk_mask, sign_scale, topk_count, uplink_bytes)
from fedmi.fl.engine import EngineConfig, TorchRoundEngine
from fedmi.fl.simulate import ClientGroup
from fedmi.privacy import philox

from .server_oracle import shape_data

U = 2.0 ** -24          # unit roundoff of fp32
LEVELS = (1, 2, 127, 32767)


def _bits(t):
    return torch.as_tensor(t, dtype=torch.float32).contiguous().numpy().view(np.uint32)


def _rand(P, seed=0, scale=0.05):
    return torch.as_tensor((scale * np.random.default_rng(seed).standard_normal(P)).astype(np.float32))


# ---- config ----
def test_names_and_defaults():
    assert COMPRESSORS == ("none", "topk", "sign") and RANDOM_COMPRESSORS == ("qsgd", "randk")
    assert ALL_COMPRESSORS == COMPRESSORS + RANDOM_COMPRESSORS
    cfg = EngineConfig()
    assert (cfg.compress_levels, cfg.compress_seed) == (127, None) and compress_id(cfg) == 0
    assert compress_id(EngineConfig(compress="qsgd")) == 3 and compress_id(EngineConfig(compress="randk")) == 4
    assert compress_id(EngineConfig(compress="qsgd", compress_levels=1, compress_seed=0)) == 3
    assert compress_id(EngineConfig(compress="qsgd", compress_levels=32767, compress_seed=2 ** 64 - 1)) == 3
    streams = {philox.DP_STREAM, philox.QSGD_STREAM, philox.RANDK_STREAM}
    from fedmi.fl.secagg import SECAGG_STREAM
    assert len(streams | {SECAGG_STREAM}) == 4


@pytest.mark.parametrize("kw, field", [
    (dict(compress="qsgd", compress_levels=0), "compress_levels"),
    (dict(compress="qsgd", compress_levels=32768), "compress_levels"),
    (dict(compress="qsgd", compress_levels=1.5), "compress_levels"),
    (dict(compress="topk", compress_levels=-3), "compress_levels"),
    (dict(compress="randk", compress_seed=-1), "compress_seed"),
    (dict(compress="qsgd", compress_seed=2 ** 64), "compress_seed"),
    (dict(compress="qsgd", compress_seed="seven"), "compress_seed"),
    (dict(compress="randk", compress_ratio=0.0), "compress_ratio"),
    (dict(compress="randk", error_feedback=1), "error_feedback"),
    (dict(compress="qsgd", dp_clip=0.5, dp_seed=1), "dp_clip"), (dict(compress="randk", dp_clip=0.5, dp_seed=1), "dp_clip")])
def test_validation_names_the_field(kw, field):
    with pytest.raises(ValueError, match=field):
        compress_id(EngineConfig(**kw))
    X, y, C, flat = shape_data("small")
    with pytest.raises(ValueError, match=field):
        TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=2, **kw), None, flat)


def test_refusals_are_those_of_the_old_kinds():
    X, y, C, flat = shape_data("small")
    from fedmi.fl.engine import HipRoundEngine
    from fedmi.fl.wide import WideClient
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    for kind in RANDOM_COMPRESSORS:
        with pytest.raises(ValueError, match="compress"):
            HipRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=2, compress=kind), None, flat,
                           comm_buffers=(torch.zeros(8), torch.zeros(8)))
        with pytest.raises(ValueError, match="compress"):
            FedTrialGroup(X, y, C, [FedTrial((4,), 0.01, 1)], None, EngineConfig(max_rounds=2, compress=kind),
                          backend="torch")
        with pytest.raises(ValueError, match="compress"):
            WideClient(torch.zeros(4, 14), torch.zeros(4, dtype=torch.long), [14, 8, 2], compress=kind)


def test_k_and_wire_size():
    P = 11352
    assert uplink_bytes("qsgd", P, P, 127) == 4 + 11352 == uplink_bytes("qsgd", P, P)
    assert uplink_bytes("qsgd", P, P, 1) == 4 + math.ceil(11352 * 2 / 8)
    assert uplink_bytes("qsgd", P, P, 2) == 4 + math.ceil(11352 * 3 / 8)
    assert uplink_bytes("qsgd", 34, 34, 32767) == 4 + 68
    assert topk_count(0.01, P) == 114 and uplink_bytes("randk", 114, P) == 4 * 114
    assert uplink_bytes("topk", 114, P) == 8 * 114 and uplink_bytes("none", P, P) == 4 * P    # as before
    with pytest.raises(ValueError, match="compress"):
        uplink_bytes("rand-k", 1, 1)
    assert compress_k(EngineConfig(compress="randk", compress_ratio=0.01), P) == 114
    assert compress_k(EngineConfig(compress="qsgd", compress_ratio=0.01), P) == P
    X, y, C, flat = shape_data("small")
    mk = lambda **kw: TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=2, **kw), None, flat)
    assert mk(compress="randk").uplink_bytes() == 4 * 51
    assert mk(compress="qsgd", compress_levels=1).uplink_bytes() == 4 + math.ceil(507 * 2 / 8)


# ---- the stream ----
def test_words_follow_round_client_and_seed():
    for kind in RANDOM_COMPRESSORS:
        base = compress_words(kind, 507, 7, 3, 2)
        assert base.dtype == np.uint32 and base.shape == (507,)
        np.testing.assert_array_equal(base, compress_words(kind, 507, 7, 3, 2))
        for other in ((8, 3, 2), (7, 4, 2), (7, 3, 1)):
            assert (compress_words(kind, 507, *other) != base).mean() > 0.99
        np.testing.assert_array_equal(compress_words(kind, 34, 7, 3, 2), base[:34])     # a prefix: counter = quad
    assert (compress_words("qsgd", 507, 7, 3, 2) != compress_words("randk", 507, 7, 3, 2)).mean() > 0.99
    # the layout: word p % 4 of the block at counter (p // 4, round, client, stream) under seed_key(seed)
    seed = 0x0123456789ABCDEF
    blk = philox.philox4x32_10(np.array([[5, 3, 2, philox.QSGD_STREAM]], np.uint64), philox.seed_key(seed))
    np.testing.assert_array_equal(compress_words("qsgd", 507, seed, 3, 2)[20:24], blk[0])


def test_ordered_sum_is_the_sign_scale_sum():
    u = _rand(11352, 1)
    a = np.abs(u.numpy())
    assert sign_scale(u) == np.float32(ordered_sum(a) / np.float32(11352))
    assert qsgd_norm(u) == np.float32(np.sqrt(ordered_sum(u.numpy() * u.numpy())))
    assert abs(float(qsgd_norm(u)) - float(u.double().norm())) <= 40 * U * float(u.double().norm())
    assert qsgd_norm(u.double()).dtype == np.float64


# ---- qsgd ----
@pytest.mark.parametrize("P", [34, 507, 11352])
@pytest.mark.parametrize("s", LEVELS)
def test_qsgd_levels_sign_and_error_bound(P, s):
    u = _rand(P, P + s)
    norm = qsgd_norm(u)
    words = compress_words("qsgd", P, 11, 2, 1)
    lv = qsgd_levels(u, s, norm, words)
    assert lv.dtype == np.float32 and (lv == np.floor(lv)).all() and lv.min() >= 0 and lv.max() <= s
    c, e, stat = compress_torch(u, "qsgd", levels=s, seed=11, round=2, client=1)
    assert c.dtype == torch.float32 and stat == float(norm) > 0
    np.testing.assert_array_equal(_bits(c.abs()), _bits((norm * lv) / np.float32(s)))
    nz = c != 0
    assert (torch.signbit(c) == torch.signbit(u)).all() and (torch.sign(c[nz]) == torch.sign(u[nz])).all()
    err = float((c.double() - u.double()).abs().max())
    assert err <= float(norm) / s * (1 + 4 * U), (err, float(norm) / s)
    np.testing.assert_array_equal(_bits(e), _bits(u - c))
    c0, e0, _ = compress_torch(u, "qsgd", error_feedback=False, levels=s, seed=11, round=2, client=1)
    assert torch.equal(c0, c) and not e0.any()
    # the same triple reproduces the draw; another round, client or seed changes it
    again, _, _ = compress_torch(u, "qsgd", levels=s, seed=11, round=2, client=1)
    assert torch.equal(again, c)
    if P > 34:
        for kw in (dict(seed=12, round=2, client=1), dict(seed=11, round=3, client=1), dict(seed=11, round=2, client=0)):
            assert not torch.equal(compress_torch(u, "qsgd", levels=s, **kw)[0], c)
    # given the norm
    cn, _, sn = compress_torch(u, "qsgd", levels=s, seed=11, round=2, client=1, norm=float(norm) * 2)
    assert sn == float(norm) * 2 and not torch.equal(cn, c)


def test_qsgd_zero_and_non_finite_norms_travel_as_they_are():
    z = torch.zeros(34)
    z[1::2] = -0.0
    c, e, stat = compress_torch(z, "qsgd", levels=2, seed=1)
    np.testing.assert_array_equal(_bits(c), _bits(z))
    assert stat == 0 and not e.any()
    u = _rand(507, 3)
    u[100] = math.nan
    c, e, stat = compress_torch(u, "qsgd", levels=127, seed=1)
    np.testing.assert_array_equal(_bits(c), _bits(u))
    assert math.isnan(stat) and not e.any()
    u[100] = 3e30                                          # the square overflows: norm = inf
    c, e, stat = compress_torch(u, "qsgd", levels=127, seed=1)
    np.testing.assert_array_equal(_bits(c), _bits(u))
    assert stat == math.inf and not e.any()


@pytest.mark.parametrize("P", [34, 507])
@pytest.mark.parametrize("s", LEVELS)
def test_qsgd_is_unbiased_over_fixed_seeds(P, s):
    """An entry's c takes two values norm / s apart, so its standard deviation is at most (norm / s) / 2 and
    that of the mean over n = 1024 independent seeds at most (norm / s) / (2 sqrt(n)); six of those."""
    u = _rand(P, 100 + P)
    norm = float(qsgd_norm(u))
    mean = torch.zeros(P, dtype=torch.float64)
    for seed in range(1, 1025):
        mean += compress_torch(u, "qsgd", levels=s, seed=seed, round=0, client=0, norm=norm)[0].double()
    mean /= 1024
    bound = 6 * (norm / s) / (2 * math.sqrt(1024))
    worst = float((mean - u.double()).abs().max())
    print(f"qsgd P={P} s={s}: max |mean c - u| / bound = {worst / bound:.3f}")
    assert worst <= bound


# ---- randk ----
@pytest.mark.parametrize("P", [34, 507, 11352])
@pytest.mark.parametrize("k", ["one", "hundredth", "half", "all"])
def test_randk_keeps_exactly_k_by_key(P, k):
    k = {"one": 1, "hundredth": topk_count(0.01, P), "half": P // 2, "all": P}[k]
    u = _rand(P, P)
    key = randk_keys(P, 5, 4, 3)
    assert key.min() >= 0 and key.max() < 2 ** 31
    np.testing.assert_array_equal(key, (compress_words("randk", P, 5, 4, 3) >> 1).astype(np.int64))
    kept = randk_mask(P, k, 5, 4, 3).numpy()
    order = np.argsort(-key, kind="stable")
    want = np.zeros(P, bool)
    want[order[:k]] = True
    np.testing.assert_array_equal(kept, want)
    assert kept.sum() == k
    c, e, stat = compress_torch(u, "randk", k, seed=5, round=4, client=3)
    np.testing.assert_array_equal(_bits(c), _bits(torch.where(torch.as_tensor(kept), u, torch.zeros(P))))
    np.testing.assert_array_equal(_bits(e), _bits(torch.where(torch.as_tensor(kept), torch.zeros(P), u)))
    assert stat == float(np.float32(key[order[k - 1]]) * np.float32(2.0 ** -31)) and 0 <= stat < 1
    # the gain is P / k only without error feedback
    c0, e0, stat0 = compress_torch(u, "randk", k, error_feedback=False, seed=5, round=4, client=3)
    gain = np.float32(np.float32(P) / np.float32(k))
    np.testing.assert_array_equal(_bits(c0), _bits(torch.where(torch.as_tensor(kept), u * float(gain), torch.zeros(P))))
    assert not e0.any() and stat0 == stat
    if k < P:
        assert not torch.equal(c0, c)
        assert not np.array_equal(randk_mask(P, k, 5, 5, 3).numpy(), kept)      # another round, another set
    # the selection does not look at u
    np.testing.assert_array_equal(compress_torch(-7 * u, "randk", k, seed=5, round=4, client=3)[0].numpy() != 0, kept)


def test_randk_ties_keep_the_lower_index(monkeypatch):
    import fedmi.fl.compress as cp
    keys = np.array([5, 9, 5, 5, 1, 9], np.int64)
    monkeypatch.setattr(cp, "randk_keys", lambda P, seed, round, client: keys)
    u = torch.arange(1.0, 7.0)
    for k, want in ((1, [1]), (2, [1, 5]), (3, [0, 1, 5]), (4, [0, 1, 2, 5]), (5, [0, 1, 2, 3, 5])):
        c, _, stat = cp.compress_torch(u, "randk", k)
        assert np.flatnonzero(c.numpy()).tolist() == want
        assert stat == float(np.float32(keys[want].min()) * np.float32(2.0 ** -31))


def test_randk_without_error_feedback_is_unbiased_over_fixed_seeds():
    """Every entry is kept with probability k / P and then scaled by P / k: the mean over n seeds has
    standard deviation |u| sqrt((P / k - 1) / n); six of those."""
    P, k, n = 34, 9, 1024
    u = _rand(P, 9)
    mean = torch.zeros(P, dtype=torch.float64)
    for seed in range(1, n + 1):
        mean += compress_torch(u, "randk", k, error_feedback=False, seed=seed)[0].double()
    mean /= n
    bound = 6 * u.double().abs() * math.sqrt((P / k - 1) / n)
    assert ((mean - u.double()).abs() <= bound).all()


def test_compress_round_is_the_rule():
    local, x, e = _rand(507, 1, 1.0), _rand(507, 2, 1.0), _rand(507, 3, 0.02)
    for kind, kw in (("qsgd", dict(levels=2)), ("randk", dict(k=51))):
        kw = dict(seed=4, round=1, client=2, **kw)
        u = (local - x) + e
        c, en, stat = compress_torch(u, kind, **kw)
        out, en2, stat2 = compress_round(local, x, e, 0.25, kind, **kw)
        np.testing.assert_array_equal(_bits(out), _bits(torch.tensor(0.25) * (x + c)))
        assert torch.equal(en, en2) and stat == stat2
    with pytest.raises(ValueError, match="kind"):
        compress_torch(local, "dense")
    with pytest.raises(TypeError):
        compress_torch(local, "qsgd", 0, True, None, 127)      # the new arguments are keyword-only


# ---- telescoping in float64 ----
@pytest.mark.parametrize("kind", RANDOM_COMPRESSORS)
def test_error_feedback_telescopes_in_float64(kind):
    """Along six rounds of a torch client the rule, carried in float64 on the client's own (local, x)
    pairs, loses nothing: sum_r c_r + e_R == sum_r (local_r - x_r) to 1e-12 relative."""
    X, y, C, flat = shape_data("small")
    eng = TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=8, early_stop=False, compress=kind,
                                                 compress_levels=2, compress_seed=5), None, flat)
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
        c, e, _ = compress_torch(d + e, kind, k, levels=2, seed=5, round=r, client=0)
        assert c.dtype == torch.float64
        sum_c += c
        sum_d += d
    err = float((sum_c + e - sum_d).abs().max()) / float(sum_d.abs().max())
    print(kind, "telescoping error, relative", err, "residual share", float(e.abs().max() / sum_d.abs().max()))
    assert err <= 1e-12
    assert float(e.abs().max()) > 0      # something was carried
    _, e0, _ = compress_torch(sum_d, kind, k, error_feedback=False, levels=2, seed=5)
    assert not e0.any()


# ---- torch engines and groups at 17-24-3 ----
def _group(rounds=6, **kw):
    X, y, _, _ = shape_data("small")
    cfg = EngineConfig(**{**dict(hidden=(24,), max_rounds=rounds + 2, early_stop=False, compress_levels=4), **kw})
    return ClientGroup(X, y, 4, cfg, backend="torch")


def _state(g):
    return [np.concatenate([e.global_flat(), e.local_flat(), e.compress_residual.numpy(),
                            e.history()["compress_stat"]]) for e in g.clients]


@pytest.mark.parametrize("kind", RANDOM_COMPRESSORS)
def test_torch_client_follows_the_rule_bitwise(kind):
    g = _group(compress=kind, compress_seed=21, local_steps=2, participation=0.75)
    seen = 0
    for r in range(4):
        for e in g.clients:
            e.step_train()
            e.step_eval()
        snap = [(e.model.flat.detach().clone(), e._dp_input.clone(), e.compress_residual.clone()) for e in g.clients]
        bufs = [e.fedavg_contribution() for e in g.clients]
        part = set(g.clients[0].participants(r).tolist())
        for e, (local, x, res) in zip(g.clients, snap):
            if e.rank not in part:
                assert e.hist.cstat[r] == 0 and torch.equal(e.compress_residual, res)
                continue
            seen += 1
            _, en, stat = compress_round(local, x, res, 1.0, kind, e.compress_k, levels=4, seed=21, round=r,
                                         client=e.rank)
            np.testing.assert_array_equal(_bits(e.compress_residual), _bits(en))
            assert e.hist.cstat[r] == np.float32(stat) and stat > 0
        tot = bufs[0].clone()
        for b in bufs[1:]:
            tot += b
        for e in g.clients:
            e.fedavg_apply(tot.clone())
    assert seen == 12


@pytest.mark.parametrize("kind", RANDOM_COMPRESSORS)
def test_same_seed_runs_are_bitwise_equal_and_seeds_matter(kind):
    runs = []
    for seed in (3, 3, 4):
        g = _group(compress=kind, compress_seed=seed)
        g.run(5)
        assert all(e.compress_seed == seed for e in g.clients)
        runs.append(_state(g))
    for a, b, c in zip(*runs):
        np.testing.assert_array_equal(_bits(a), _bits(b))
        assert not np.array_equal(_bits(a), _bits(c))
    p = _group(compress=kind)                               # no seed: a private draw per client
    assert len({e.compress_seed for e in p.clients}) == 4
    dense = _group()
    assert not hasattr(dense.clients[0], "compress_seed") and "compress_seed" not in dense.clients[0].portable_state()
    assert "compress_seed" not in _group(compress="topk").clients[0].portable_state()


@pytest.mark.parametrize("kind", RANDOM_COMPRESSORS)
@pytest.mark.parametrize("seed", [17, None])
def test_group_resume_mid_run_is_bitwise(kind, seed):
    a = _group(compress=kind, compress_seed=seed)
    a.run(3)
    states = [e.portable_state() for e in a.clients]
    assert all(st["compress_seed"] == e.compress_seed for st, e in zip(states, a.clients))
    b = _group(compress=kind, compress_seed=seed)
    for e, st in zip(b.clients, states):
        e.load_portable_state(st)
    b.rounds = 3
    a.run(3)
    b.run(3)
    for x, y in zip(_state(a), _state(b)):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    if seed is not None:
        c = _group(compress=kind, compress_seed=seed)
        c.run(6)
        for x, y in zip(_state(a), _state(c)):
            np.testing.assert_array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("kind", RANDOM_COMPRESSORS)
def test_checkpoint_round_trip_and_mismatch_errors(tmp_path, kind):
    from fedmi.ckpt.checkpoint import load_checkpoint, resume, save_checkpoint
    X, y, C, flat = shape_data("small")
    mk = lambda **kw: TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=8, early_stop=False, **kw), None,
                                       flat)
    a = mk(compress=kind)                                   # a private 64-bit seed
    a.run(3)
    save_checkpoint(str(tmp_path / "s"), a)
    lo, hi = (int(v) for v in load_checkpoint(str(tmp_path / "s"), rank=0)["client"]["compress_seed"])
    assert lo | (hi << 32) == a.compress_seed and 0 <= lo < 2 ** 32 and 0 <= hi < 2 ** 32
    b = mk(compress=kind)
    assert b.compress_seed != a.compress_seed
    assert resume(str(tmp_path / "s"), b) == 3 and b.compress_seed == a.compress_seed
    a.run(3)
    b.run(3)
    np.testing.assert_array_equal(_bits(a.global_flat()), _bits(b.global_flat()))
    np.testing.assert_array_equal(_bits(a.compress_residual), _bits(b.compress_residual))
    np.testing.assert_array_equal(a.history()["compress_stat"], b.history()["compress_stat"])
    # a state without compress_seed does not load into a random-compressor engine, nor the reverse
    det = mk(compress="topk")
    det.run(2)
    with pytest.raises(ValueError, match="compress_seed"):
        mk(compress=kind).load_portable_state(det.portable_state())
    with pytest.raises(ValueError, match="compress_seed"):
        mk(compress="sign").load_portable_state(a.portable_state())
    with pytest.raises(ValueError, match="compress"):
        mk().load_portable_state(a.portable_state())
    with pytest.raises(ValueError, match="compress"):
        resume(str(tmp_path / "s"), mk())
    save_checkpoint(str(tmp_path / "d"), det)
    assert "compress_seed" not in load_checkpoint(str(tmp_path / "d"), rank=0)["client"]
    assert resume(str(tmp_path / "d"), mk(compress="topk")) == 2      # a deterministic state loads as before


# ---- the [C] entry point ----
def _run_c(args):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(root, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py"),
                           "--device", "cpu", "--backend", "gloo", "--engine", "torch", "--quiet", *args],
                          cwd=root, capture_output=True, text=True, timeout=300, env=env)


def test_entry_point_flags(tmp_path):
    import json
    P = 14 * 8 + 8 + 8 * 2 + 2
    rows = {}
    for name, args, want in (
            ("qsgd", ["--compress", "qsgd", "--compress-levels", "2", "--compress-seed", "5"], 4 + math.ceil(P * 3 / 8)),
            ("randk", ["--compress", "randk", "--compress-ratio", "0.25", "--compress-seed", "5", "--no-error-feedback"],
             4 * math.ceil(0.25 * P))):
        out = str(tmp_path / f"{name}.jsonl")
        r = _run_c(["--clients", "2", "--rounds", "2", "--no-early-stop", "--hidden", "8", *args, "--jsonl", out])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows[name] = [json.loads(line) for line in open(out)]
        assert len(rows[name]) == 2 and all(row["uplink_bytes"] == want for row in rows[name])
        assert all(row["compress_stat"] > 0 for row in rows[name])
    r = _run_c(["--wide", "--compress", "qsgd"])
    assert r.returncode != 0 and "--compress is not supported with --wide" in r.stderr
    r = _run_c(["--compress", "qsgd", "--compress-levels", "0"])
    assert r.returncode != 0 and "compress_levels" in r.stderr
    r = _run_c(["--compress", "randk", "--compress-seed", "-1"])
    assert r.returncode != 0 and "compress_seed" in r.stderr

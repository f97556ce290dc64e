"""Secure aggregation on the CPU: the host model of fedmi/fl/secagg.py (quantise, pair masks, open), the
config validation and refusals, torch client groups with secagg on against off, checkpoints, the [C]
entry point's flags.

Bound.  K_r contributions are each rounded once to the 2^-F grid (<= 2^-(F+1) each) and the integer sum
is rounded once to fp32 (<= 2^-24 of its magnitude), so against the float64 sum ``ref`` of the fp32
contributions |opened - ref| <= K_r 2^-(F+1) + 2^-24 |ref| up to a factor 1 + 2^-24; asserted as 1.001 x.
"""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.engine import EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.fl.secagg import (SECAGG_STREAM, pair_mask, secagg_id, secagg_limit, secagg_mask, secagg_open,
                             secagg_quantize, secagg_round)
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.privacy.philox import DP_STREAM, philox4x32_10, seed_key

from .server_oracle import shape_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_SMALL = 17 * 24 + 24 + 24 * 3 + 3   # 17-24-3: 507 parameters, the last quad is partial
SEED = 0x0123456789ABCDEF


def _bound(kr, bits, ref):
    return 1.001 * (kr * 2.0 ** -(bits + 1) + 2.0 ** -24 * np.abs(ref))


def _contribs(K, kr, seed):
    """K weighted contributions: normals scaled like w_i * model (the sum stays O(1))."""
    return (np.random.default_rng(seed).standard_normal((K, P_SMALL)) / kr).astype(np.float32)


CASES = [(2, [0, 1]), (5, [0, 2, 4]), (8, list(range(8))), (64, list(range(64)))]


# ---- 1. cancellation, 2. seed independence ----
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("K, part", CASES, ids=["2", "3of5", "8", "64"])
def test_masks_cancel_and_the_sum_opens_within_the_bound(K, part, bits):
    cs = _contribs(K, len(part), 10 * K + bits)
    opened, ys, counts = secagg_round(cs, part, 3, bits, SEED)
    qs = np.stack([secagg_quantize(cs[i], bits, len(part))[0] for i in part])
    with np.errstate(over="ignore"):
        sy = np.stack([ys[i] for i in part]).sum(axis=0, dtype=np.uint32)
        sq = qs.view(np.uint32).sum(axis=0, dtype=np.uint32)
    np.testing.assert_array_equal(sy, sq)                               # mod 2^32, exactly
    np.testing.assert_array_equal(sq.view(np.int32).astype(np.int64), qs.astype(np.int64).sum(axis=0))   # no wrap
    assert sum(counts.values()) == 0
    ref = cs[part].astype(np.float64).sum(axis=0)
    ratio = np.abs(opened.astype(np.float64) - ref) / _bound(len(part), bits, ref)
    print(f"K_r={len(part)} F={bits}: worst error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    # another seed: other words on the wire, the same opened bits
    other, ys2, _ = secagg_round(cs, part, 3, bits, SEED + 1)
    np.testing.assert_array_equal(other.view(np.int32), opened.view(np.int32))
    assert all((ys2[i] != ys[i]).mean() > 0.99 for i in part)


# ---- 3. clamp ----
@pytest.mark.parametrize("kr", [1, 3, 64])
def test_clamp_inf_and_nan(kr):
    L = secagg_limit(kr)
    assert L == (2 ** 31 - 1) // kr
    c = np.array([1e9, -1e9, np.inf, -np.inf, np.nan, 2.0 ** -6, -0.0, 0.0], np.float32)
    for bits in (8, 24, 30):
        q, n = secagg_quantize(c, bits, kr)
        assert q.dtype == np.int32 and n == 5
        np.testing.assert_array_equal(q, [L, -L, L, -L, 0, 2 ** (bits - 6), 0, 0])
    # exactly +-L is kept and not counted; one more is clamped; ties round to even
    q, n = secagg_quantize(np.array([L, -L, L + 1, 2.5, 3.5, -2.5], np.float64).astype(np.float32) / 256, 8, kr)
    if L < 2 ** 24:   # (L itself is an fp32 value)
        assert n == 1 and q[:3].tolist() == [L, -L, L]
    assert q[3:].tolist() == [2, 4, -2]
    # K_r clamped maxima do not wrap
    ys = np.stack([secagg_mask(secagg_quantize(np.full(5, np.inf, np.float32), 24, kr)[0], i, range(kr), 0, SEED)
                   for i in range(kr)])
    np.testing.assert_array_equal(secagg_open(ys, 24), np.float32(kr * L) * np.float32(2.0 ** -24))
    assert kr * L <= 2 ** 31 - 1


# ---- 4. masking sanity (not a security proof) ----
def test_masked_words_look_uniform_and_depend_on_round_client_and_seed():
    K, bits = 8, 24
    part = list(range(K))
    cs = _contribs(K, K, 5)
    _, ys, _ = secagg_round(cs, part, 2, bits, SEED)
    tol = 5.0 / (2.0 * np.sqrt(32.0 * P_SMALL))
    assert abs(tol - 0.0196) < 1e-4
    worst = 0.0
    for i in part:
        q = secagg_quantize(cs[i], bits, K)[0].view(np.uint32)
        assert not (ys[i] == q).any()                                   # expected rate 2^-32
        ones = np.unpackbits(ys[i].view(np.uint8)).mean()
        worst = max(worst, abs(ones - 0.5))
    print(f"worst one-bit fraction off 0.5: {worst:.4f} (tolerance {tol:.4f})")
    assert worst <= tol
    q0 = secagg_quantize(cs[0], bits, K)[0]
    base = secagg_mask(q0, 0, part, 2, SEED)
    assert (secagg_mask(q0, 0, part, 3, SEED) != base).mean() > 0.99    # round
    assert (secagg_mask(q0, 1, part, 2, SEED) != base).mean() > 0.99    # client
    assert (secagg_mask(q0, 0, part, 2, SEED ^ 1) != base).mean() > 0.99   # seed
    assert (secagg_mask(q0, 0, part[:-1], 2, SEED) != base).mean() > 0.99  # sampled set
    # a lone sampled client has no pair: its quantised value travels unmasked
    np.testing.assert_array_equal(secagg_mask(q0, 0, [0], 2, SEED), q0.view(np.uint32))


def test_pair_mask_is_the_documented_philox_stream():
    assert SECAGG_STREAM != DP_STREAM
    a, b, r = 3, 41, 7
    m = pair_mask(a, b, r, P_SMALL, SEED)
    assert m.dtype == np.uint32 and m.shape == (P_SMALL,)
    for p in (0, 1, 5, 254, 506):
        word = philox4x32_10(np.array([[p // 4, r, 64 * a + b, SECAGG_STREAM]], np.uint64), seed_key(SEED))[0, p % 4]
        assert m[p] == word
    with pytest.raises(ValueError, match="sampled"):
        secagg_mask(np.zeros(4, np.int32), 2, [0, 1], 0, SEED)
    with pytest.raises(ValueError, match="int32"):
        secagg_mask(np.zeros(4, np.float32), 0, [0, 1], 0, SEED)


# ---- 5. config ----
def test_defaults():
    cfg = EngineConfig()
    assert (cfg.secagg, cfg.secagg_bits, cfg.secagg_seed) == (False, 24, None)
    assert secagg_id(cfg) == 0 and secagg_id(EngineConfig(secagg=True)) == 1
    assert secagg_id(EngineConfig(secagg=True, secagg_bits=8, secagg_seed=2 ** 64 - 1)) == 1
    assert secagg_id(EngineConfig(secagg=True, secagg_bits=30, secagg_seed=0)) == 1
    assert {"secagg", "secagg_bits", "secagg_seed"} <= set(cfg.to_dict())


@pytest.mark.parametrize("kw, field", [
    (dict(secagg=1), "secagg"), (dict(secagg="yes"), "secagg"), (dict(secagg=True, secagg_bits=7), "secagg_bits"),
    (dict(secagg_bits=31), "secagg_bits"), (dict(secagg=True, secagg_bits=24.0), "secagg_bits"),
    (dict(secagg=True, secagg_seed=-1), "secagg_seed"), (dict(secagg=True, secagg_seed=2 ** 64), "secagg_seed"),
    (dict(secagg=True, secagg_seed=1.5), "secagg_seed")])
def test_validation_names_the_field(kw, field):
    with pytest.raises(ValueError, match=field):
        secagg_id(EngineConfig(**kw))
    X, y, C, flat = shape_data("small")
    with pytest.raises(ValueError, match=field):
        TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=2, **kw), None, flat)


def test_refusals_and_the_single_client():
    X, y, C, flat = shape_data("small")
    base = dict(hidden=(24,), max_rounds=2, secagg=True, secagg_seed=SEED)
    mk = lambda world, **kw: TorchRoundEngine(X, y, C, EngineConfig(**{**base, **kw}), SimRank(world, 0, "cpu"), flat,
                                              n_total=world * len(X), client_sizes=[len(X)] * world)
    for agg in ("median", "trimmed_mean"):
        with pytest.raises(ValueError, match="aggregator"):
            mk(3, aggregator=agg)
    with pytest.raises(ValueError, match="secagg takes at most 64 clients"):
        mk(65)
    assert mk(64).secagg == 1
    with pytest.raises(ValueError, match="secagg_seed"):   # nobody to agree on a drawn seed with
        mk(3, secagg_seed=None)
    with pytest.raises(ValueError, match="secagg"):   # trial batches hand every engine its comm buffers
        HipRoundEngine(X, y, C, EngineConfig(**base), None, flat, comm_buffers=(torch.zeros(8), torch.zeros(8)))
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    with pytest.raises(ValueError, match="secagg"):
        FedTrialGroup(X, y, C, [FedTrial((4,), 0.01, 1)], None, EngineConfig(max_rounds=2, secagg=True), backend="torch")
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="secagg"):
        WideClient(torch.zeros(4, 14), torch.zeros(4, dtype=torch.long), [14, 8, 2], secagg=True)
    # one client: the identity, nothing runs and nothing is reported
    one = TorchRoundEngine(X, y, C, EngineConfig(**base), None, flat)
    ref = TorchRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=2), None, flat)
    assert one.secagg == 0 and one.run(2) == 2 and ref.run(2) == 2
    np.testing.assert_array_equal(one.global_flat(), ref.global_flat())
    assert "secagg_clamped" not in one.history()


# ---- 6. torch groups, secagg on against off ----
ROUNDS, BITS = 6, 24


def _group(rounds=ROUNDS, wire=None, k=5, **kw):
    X, y, _, _ = shape_data("small")
    torch.set_num_threads(1)
    cfg = EngineConfig(**{**dict(hidden=(24,), max_rounds=rounds + 2, early_stop=False, eps=1e-4), **kw})
    return ClientGroup(X, y, k, cfg, backend="torch", shard_mode="iid", seed=2, wire=wire)


@pytest.mark.parametrize("kw", [dict(), dict(participation=0.6), dict(dp_clip=0.5, dp_noise=0.5, dp_seed=7),
                                dict(server_opt="adam", server_lr=1e-2)],
                         ids=["plain", "3of5", "dp", "server"])
def test_torch_group_with_secagg_against_without(kw):
    clear = {}
    on, off = _group(secagg=True, secagg_seed=SEED, **kw), _group(**kw)
    on.tamper = lambda r, bufs: clear.setdefault(r, [b[:P_SMALL].numpy().copy() for b in bufs])
    on.run(1)
    off.run(1)
    lead = on.clients[0]
    part = [int(k) for k in lead.participants(0)]
    assert len(part) == (3 if "participation" in kw else 5)
    for key in ("global", "per_rank", "loss"):   # round 0 scores the local models: untouched by the aggregation
        np.testing.assert_array_equal(on.history()[key], off.history()[key])
    if "server_opt" not in kw:
        # the opened round-0 image against the float64 sum of the clients' own clear fp32 contributions
        # (with a server optimizer the global weights are a step from that sum, not the sum)
        ref = np.stack(clear[0])[part].astype(np.float64).sum(axis=0)
        err = np.abs(on.global_flat().astype(np.float64) - ref)
        assert (err <= _bound(len(part), BITS, ref)).all(), float((err / _bound(len(part), BITS, ref)).max())
    e0 = float(np.abs(on.global_flat() - off.global_flat()).max() / np.abs(off.global_flat()).max())
    on.run(ROUNDS - 1)
    off.run(ROUNDS - 1)
    a, b = on.global_flat(), off.global_flat()
    e = float(np.abs(a - b).max() / np.abs(b).max())
    print(f"{kw}: secagg on vs off, max|err| / max|ref|: round 0 {e0:.3g}, after {ROUNDS} rounds {e:.3g}")
    assert e0 < 2e-5 and e < 2e-5
    for c in on.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), a)
    h = on.history()
    assert h["secagg_clamped"].shape == (ROUNDS,) and not h["secagg_clamped"].any()
    assert "secagg_clamped" not in off.history()
    # the seed is not part of the result
    again = _group(secagg=True, secagg_seed=SEED + 99, **kw)
    again.run(ROUNDS)
    np.testing.assert_array_equal(again.global_flat(), a)
    drawn = _group(secagg=True, **kw)   # secagg_seed=None: one draw for the whole group
    assert len({c.secagg_seed for c in drawn.clients}) == 1
    drawn.run(ROUNDS)
    np.testing.assert_array_equal(drawn.global_flat(), a)


def test_clamped_coordinates_are_counted():
    def tamper(r, bufs):
        bufs[1][:3] = torch.tensor([float("nan"), float("inf"), -1e9])
    g = _group(secagg=True, secagg_seed=SEED, k=3)
    g.tamper = tamper
    g.run(2)
    assert [c.history()["secagg_clamped"].tolist() for c in g.clients] == [[0, 0], [3, 3], [0, 0]]
    L = secagg_limit(3)
    w = g.global_flat()
    assert np.isfinite(w).all() and abs(w[1]) > 0.5 * L * 2.0 ** -BITS and abs(w[2]) > 0.5 * L * 2.0 ** -BITS


# ---- 7. checkpoints and the wire ----
def test_wire_hook_sees_the_host_model():
    clear, wire = {}, {}
    g = _group(secagg=True, secagg_seed=SEED, participation=0.6,
               wire=lambda r, bufs: wire.setdefault(r, [b.clone() for b in bufs]))
    g.tamper = lambda r, bufs: clear.setdefault(r, [b.clone() for b in bufs])
    g.run(1)
    part = [int(k) for k in g.clients[0].participants(0)]
    assert len(part) == 3
    for i in range(5):
        c, w = clear[0][i], wire[0][i]
        assert torch.equal(c[P_SMALL:], w[P_SMALL:])                     # tails stay clear floats
        if i in part:
            q, n = secagg_quantize(c[:P_SMALL].numpy(), BITS, 3)
            np.testing.assert_array_equal(w[:P_SMALL].view(torch.int32).numpy().view(np.uint32),
                                          secagg_mask(q, i, part, 0, SEED))
        else:
            assert not c[:P_SMALL].any() and not w[:P_SMALL].view(torch.int32).any()   # untouched zeros


def test_checkpoint_round_trip_and_resume(tmp_path):
    """Every client of a group saves after 3 rounds; a group with ANOTHER mask seed resumes and continues
    bit for bit with the uninterrupted run.  The checkpoint carries the three config fields and no seed."""
    from fedmi.ckpt.checkpoint import load_checkpoint, resume, save_checkpoint
    kw = dict(secagg=True, participation=0.6, k=3)
    a = _group(secagg_seed=5, **kw)
    a.run(3)
    for c in a.clients:
        save_checkpoint(str(tmp_path / "s"), c)
    ck = load_checkpoint(str(tmp_path / "s"), rank=1)
    cfg = ck["meta"]["config"]
    assert (cfg["secagg"], cfg["secagg_bits"], cfg["secagg_seed"]) == (True, 24, 5)
    assert not any("seed" in k for k in ck["client"])                   # the mask seed is config, never state
    b = _group(secagg_seed=6, **kw)
    for c in b.clients:
        assert resume(str(tmp_path / "s"), c) == 3
    b.rounds = 3
    for c, d in zip(a.clients, b.clients):
        np.testing.assert_array_equal(c.global_flat(), d.global_flat())
        np.testing.assert_array_equal(c.local_flat(), d.local_flat())
    a.run(3)
    b.run(3)
    c = _group(secagg_seed=7, **kw)
    c.run(6)
    for g in (a, b):
        for e, ref in zip(g.clients, c.clients):
            np.testing.assert_array_equal(e.global_flat(), ref.global_flat())
            for key in ("secagg_clamped", "global", "loss", "per_rank"):
                np.testing.assert_array_equal(e.history()[key], ref.history()[key])
    # a checkpoint without secagg loads into an engine with it and back: the fields are config only
    p = _group(k=3)
    p.run(2)
    for e in p.clients:
        save_checkpoint(str(tmp_path / "p"), e)
    assert resume(str(tmp_path / "p"), _group(secagg=True, k=3).clients[0]) == 2


# ---- three ranks over gloo ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_cfg(**kw):
    # secagg_seed=None: every rank takes rank 0's draw over the control plane
    return EngineConfig(**{**dict(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, secagg=True,
                                  participation=0.67, dp_clip=0.5, dp_noise=0.5, dp_seed=7), **kw})


def _gloo_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    try:
        from fedmi.data.sharding import shard_indices
        from fedmi.models.mlp import init_flat
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="gloo", device="cpu")
        X, y, _, _ = shape_data("small")
        idx = [shard_indices(len(X), r, world, mode="iid", seed=2, labels=y, alpha=0.5) for r in range(world)]
        e = TorchRoundEngine(X[idx[rank]], y[idx[rank]], 3, _rank_cfg(), comm, init_flat([17, 24, 3], 2 * 1000003 + rank),
                             n_total=sum(len(i) for i in idx))
        e.run(ROUNDS)
        h = e.history()
        q.put((rank, (e.secagg_seed, e.global_flat(), np.asarray(h["global"]), np.asarray(h["loss"])), None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_three_ranks_over_gloo_equal_the_torch_group_bitwise():
    """Sampling 2 of 3, DP noise, a drawn seed: every rank gathers the masked rows, opens the same sum."""
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
    assert len({out[0] for _, out, _ in res}) == 1                      # one seed for the job
    g = _group(k=3, **{k: v for k, v in _rank_cfg().to_dict().items() if k in ("secagg", "participation", "dp_clip",
                                                                               "dp_noise", "dp_seed")}, eps=1e-8)
    g.run(ROUNDS)
    assert len(g.clients[0].participants(0)) == 2
    ref = (g.global_flat(), g.history()["global"], g.history()["loss"])
    for rank, out, _ in res:
        for a, b in zip(out[1:], ref):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank}")


def test_trainer_warns_once_when_a_coordinate_clamped():
    from fedmi.fl.trainer import FederatedMLPLearning
    X, y, _, _ = shape_data("small")
    cfg = EngineConfig(hidden=(24,), max_rounds=4, early_stop=False, secagg=True, secagg_seed=SEED)
    fl = FederatedMLPLearning(X, y, 0, 1, comm=None, hidden_sizes=[24], config=cfg, backend="torch")
    fl.train_and_evaluate(None, rounds=2, verbose=False)                # one client: the identity, no history, no warning
    assert fl.engine.secagg == 0 and "secagg_clamped" not in fl.history()
    # what a multi-client engine that clamped reports, with no round left to run
    fl.engine.secagg = 1
    fl.engine.hist.clamped = np.array([0, 4, 0, 0])
    with pytest.warns(RuntimeWarning, match="secure aggregation clamped 4 coordinates"):
        fl.train_and_evaluate(None, rounds=2, verbose=False)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fl.train_and_evaluate(None, rounds=2, verbose=False)            # once per trainer


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
    r = _run_c(["--clients", "2", "--rounds", "2", "--no-early-stop", "--hidden", "8", "--secagg", "--secagg-bits", "20",
                "--secagg-seed", "11", "--jsonl", out])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [json.loads(line) for line in open(out)]
    assert len(rows) == 2 and all(row["secagg_clamped"] == 0 for row in rows)
    # the refusals are decided before a communicator exists: in process
    sys.path.insert(0, ROOT)
    try:
        import FL_CustomMLPCLassifierImplementation_Multiple_Rounds as entry
    finally:
        sys.path.remove(ROOT)
    a = entry.parse_args(["--secagg", "--secagg-bits", "12", "--secagg-seed", "3"])
    assert (a.secagg, a.secagg_bits, a.secagg_seed) == (True, 12, 3)
    a = entry.parse_args([])
    assert (a.secagg, a.secagg_bits, a.secagg_seed) == (False, 24, None)
    for args, msg in ((["--wide", "--secagg"], "--secagg is not supported with --wide"),
                      (["--secagg", "--secagg-bits", "31"], "secagg_bits"),
                      (["--secagg", "--aggregator", "median"], "aggregator")):
        with pytest.raises(SystemExit, match=msg):
            entry.main(["--device", "cpu", "--backend", "gloo", "--engine", "torch", "--quiet", *args])

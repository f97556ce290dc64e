"""Differentially private FedAvg on the GPU: the clip + noise kernel (fl_dp.hip) against a float64
host model of its own inputs, DP rounds against the torch oracle, and the engine paths around it
(client groups, client sampling, early stop, resume, graphs, the xGMI plane, trial batches).

Shapes: ``income`` = make_multiclass(300, 14, 2) with 14-50-200-2 (P = 11 352 dense parameters = 2 838
noise blocks = three 1024-thread workgroups, image of 19 104 floats with real padding) and ``small`` =
(96, 17, 3) with 17-24-3 (one workgroup, F off the income shape).  Clipping bounds and the norms they
were placed between: tests/dp_oracle.py.  The oracle's own float64 distance on the end-to-end cases is
at most 1.2e-6 (tests/test_dp_cpu.py), under a quarter of the bounds used here, so those stay at
the project's 2e-5 (weights, moments) and rtol 1e-4 (loss).
"""
import functools
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.engine import EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_to_dense, init_flat
from fedmi.privacy.philox import dp_normals

from .dp_oracle import DP_CASES, DP_ROUNDS, DP_SEED, DP_Z, assert_clip_decisions, contribution_f64
from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
KERNEL_Z = 0.5          # kernel tests: noise large enough that xi / sigma resolves the normals' own error


def norm_chain(Pimg):
    """Longest sequential chain of the kernel's ||D||^2 reduction: 4 fused multiply-adds per float4
    a thread owns (float4s t, t + 1024, ...), 6 levels of the wave's xor tree, 16 wave sums."""
    return 4 * math.ceil(Pimg / 4 / 1024) + 6 + 16


def _case_engine(cls, case, z, **kw):
    rows, F, C, hidden, S, extra = DP_CASES[case]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    cfg = EngineConfig(hidden=hidden, max_rounds=DP_ROUNDS + 2, early_stop=False, dp_clip=S[z], dp_noise=z,
                       dp_seed=DP_SEED, **{"graph_rounds": 0, **extra, **kw})
    return cls(X, y, C, cfg, None, init_flat([F, *hidden, C], INIT_SEED))


@functools.lru_cache(maxsize=None)
def _oracle(case, z):
    """DP_ROUNDS rounds of the fp32 torch oracle, once per case (read-only)."""
    ref = _case_engine(TorchRoundEngine, case, z)
    ref.run(DP_ROUNDS)
    st, h = ref.portable_state(), ref.history()
    out = {"w": ref.global_flat(), "m": st["exp_avg"], "v": st["exp_avg_sq"], "loss": h["loss"],
           "norm": h["update_norm"].astype(np.float64)}
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- 1: the kernel against its own inputs ----
def _check_contribution(e, r, w, rank, S, z, tag):
    """Round r's contribution in e's comm buffer vs the float64 model of (local, input image)."""
    e.stream.synchronize()
    dims, Pimg = e.dims, e.Pimg
    x_img = e.params[r & 1][:Pimg].cpu().numpy()
    out_img = e.params[(r + 1) & 1][:Pimg].cpu().numpy()
    loc_img = e.local.cpu().numpy()
    pad = dense_to_image(np.ones(e.P, np.float32), dims) == 0
    assert pad.sum() == Pimg - e.P and pad.any()
    assert not out_img[pad].any() and not loc_img[pad].any(), f"{tag}: padding written"
    x, out, loc = (image_to_dense(a, dims).astype(np.float64) for a in (x_img, out_img, loc_img))
    sigma = float(e.dp_sigma[r])
    nrm = dp_normals(e.P, r, rank, DP_SEED) if z else None
    want, norm, c = contribution_f64(loc, x, w, S, sigma, nrm)
    L = norm_chain(Pimg)
    got_norm = float(e.dp_norm[r].item())
    print(tag, "round", r, "norm", got_norm, "rel err", abs(got_norm - norm) / norm, "bound", L * U, "c", c)
    assert abs(got_norm - norm) <= L * U * norm, (tag, r, got_norm, norm)
    # elementwise: c carries the norm's error + its division's rounding; then fl(a - x), the fma into
    # t = x + c D, the fma w t + noise, and the noise's own roundings (sigma * (rad * trig))
    eps_c = (L + 1) * U if c < 1.0 else 0.0
    t = x + c * (loc - x)
    bound = w * (np.abs(c * (loc - x)) * (eps_c + 2 * U) + U * np.abs(t)) + U * np.abs(want)
    if z:
        rad = np.repeat(np.hypot(np.pad(nrm, (0, -e.P % 4))[0::2], np.pad(nrm, (0, -e.P % 4))[1::2]), 2)[:e.P]
        tol_n = rad * 9e-7 + 4 * U * np.abs(nrm)
        bound = bound + sigma * (tol_n + 2 * U * np.abs(nrm))
    assert bound.max() <= 1e-4 * np.abs(want).max(), (tag, bound.max(), np.abs(want).max())
    err = np.abs(out - want)
    print(tag, "max err / bound", float(np.max(err / np.maximum(bound, 1e-300))), "max err", err.max())
    assert np.all(err <= bound), (tag, r, float(np.max(err / np.maximum(bound, 1e-300))))
    if z:
        xi = (out - w * t) / sigma
        assert np.all(np.abs(xi - nrm) <= bound / sigma), (tag, r)
        return c, xi
    return c, None


@pytest.mark.parametrize("R", [16, 32])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("z", [0.0, KERNEL_Z])
def test_kernel_matches_float64_model_of_its_inputs(dtype, R, z):
    """Three step-API rounds on the income shape (rounds 0, 1 clipped at S = 0.37 without noise; with
    z = 0.5 whatever the noised trajectory gives -- both decisions are covered by the z = 0 runs).

    Norm: the kernel's sum of squares runs through a chain of L = 4 ceil(Pimg / 4096) + 6 + 16 = 42
    fp32 operations (norm_chain), each of relative error <= u = 2^-24 on a sum of non-negative
    terms, over squares of fl(a - x) (2 u each): ||D||^2 is off by <= (L + 2) u, the norm by
    <= ((L + 2) / 2 + 1) u with sqrtf's rounding, which is below the L u = 2.5e-6 asserted here.
    Elementwise: see _check_contribution; the bound comes out near 1e-6 of max|contribution|.
    Normals: 2 pi u1 is off by <= 5.5e-7 (the fp32 constant and the product's rounding), sincosf by
    <= 2 ulp, so cos / sin by <= 9e-7 absolute, times the radius; logf (2 ulp), sqrtf and the
    product add <= 4 u relative.  The host model evaluates u01 in fp32 like the device, so nothing
    else separates the two streams."""
    S = DP_CASES["income"][4][0.0]
    X, y = make_multiclass(300, 14, 2, DATA_SEED)
    flat = init_flat([14, 50, 200, 2], INIT_SEED)
    mk = lambda: HipRoundEngine(X, y, 2, EngineConfig(max_rounds=6, early_stop=False, graph_rounds=0, dtype=dtype,
                                                      rows_per_block=R, dp_clip=S, dp_noise=z, dp_seed=DP_SEED),
                                None, flat)
    outs, cs = [], []
    for run in range(2):
        e = mk()
        assert e.R == R and e.layout["dp"] is True and not e.engine.fused and not e.engine.lagged
        for r in range(3):
            e.step_train()
            c, _ = _check_contribution(e, r, 1.0, 0, S, z, f"{dtype} R{R} z{z}")
            cs.append(c)
            e.step_eval()
            e.step_aggregate()
        e.sync_history()
        outs.append((e.global_flat(), e.history()["update_norm"].copy(), e.local_flat()))
    if z == 0.0 and dtype == "fp32":
        assert cs[0] < 1.0 and cs[2] == 1.0, cs   # both branches of the kernel ran
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)     # two runs are bitwise equal
    assert outs[0][1].shape == (3,) and (outs[0][1] > 0).all()


def test_kernel_rank_streams_are_uncorrelated_and_weights_apply():
    """Ranks 0 and 1 of a two-client federation (w = 0.5, sigma = z S 0.5 / sqrt 2) on the same
    shard: each contribution matches the model with ITS rank's normals; the two noise vectors have
    |correlation| < 5 / sqrt P."""
    S = 0.37
    X, y = make_multiclass(300, 14, 2, DATA_SEED)
    flat = init_flat([14, 50, 200, 2], INIT_SEED)
    cfg = EngineConfig(max_rounds=4, early_stop=False, graph_rounds=0, dp_clip=S, dp_noise=KERNEL_Z, dp_seed=DP_SEED,
                       lagged_eval=False)
    xi = []
    for rank in (0, 1):
        e = HipRoundEngine(X, y, 2, cfg, SimRank(2, rank, "cuda"), flat, n_total=600, client_sizes=[300, 300])
        assert float(e.dp_sigma[0]) == float(np.float32(KERNEL_Z * S * 0.5 / math.sqrt(2)))
        e.engine.run_local(0, e.stream.cuda_stream)
        c, x = _check_contribution(e, 0, 0.5, rank, S, KERNEL_Z, f"rank {rank}")
        assert c < 1.0
        xi.append(x)
    P = xi[0].size
    rho = float(np.corrcoef(xi[0], xi[1])[0, 1])
    print("rank streams: correlation", rho, "bound", 5 / math.sqrt(P))
    assert abs(rho) < 5 / math.sqrt(P)
    assert abs(xi[0].std() - 1) < 5 / math.sqrt(2 * P) and abs(xi[0].mean()) < 5 / math.sqrt(P)


def test_small_shape_kernel_single_workgroup():
    """17-24-3 (507 parameters: 127 noise blocks, the last one partial; one workgroup)."""
    rows, F, C, hidden, S, _ = DP_CASES["small"]
    for z in (0.0, KERNEL_Z):
        X, y = make_multiclass(rows, F, C, DATA_SEED)
        e = HipRoundEngine(X, y, C, EngineConfig(hidden=hidden, max_rounds=4, early_stop=False, graph_rounds=0,
                                                 dp_clip=S[0.0], dp_noise=z, dp_seed=DP_SEED), None,
                           init_flat([F, *hidden, C], INIT_SEED))
        assert e.P % 4 == 3
        for r in range(3):
            e.step_train()
            _check_contribution(e, r, 1.0, 0, S[0.0], z, f"small z{z}")
            e.step_eval()
            e.step_aggregate()


def test_bf16_round_trains_from_the_contribution_not_the_local_model():
    """One bf16 client: without DP round r + 1 stages the Adam-packed LOCAL image.  With DP the
    round's output is the clipped, noised contribution, which must be packed afresh: round 1's
    gradient partials equal those of a fresh engine started from that contribution, bit for bit."""
    X, y = make_multiclass(300, 14, 2, DATA_SEED)
    mk = lambda flat, **kw: HipRoundEngine(X, y, 2, EngineConfig(max_rounds=4, early_stop=False, graph_rounds=0,
                                                                 dtype="bf16", **kw), None, flat)
    e = mk(init_flat([14, 50, 200, 2], INIT_SEED), dp_clip=0.2, dp_noise=KERNEL_Z, dp_seed=DP_SEED)
    e.run(1)
    g1 = e.global_flat()
    assert np.abs(g1 - e.local_flat()).max() > 1e-3
    e.step_train()
    e.stream.synchronize()
    f = mk(g1)
    f.step_train()
    f.stream.synchronize()
    assert torch.equal(e.slab_partials(), f.slab_partials())


# ---- 2, 3: six rounds against the torch oracle ----
@pytest.mark.parametrize("z", [0.0, DP_Z])
@pytest.mark.parametrize("case", sorted(DP_CASES))
def test_dp_rounds_match_torch_oracle(case, z):
    """Weights, Adam moments (nerr < 2e-5) and loss (rtol 1e-4) after six fp32 DP rounds, clipping
    only and with z = 0.02; the recorded update norms equal the oracle's to the kernel's norm bound
    (norm_chain(Pimg) u, test_kernel_matches_float64_model_of_its_inputs).  The clip decisions are
    asserted on the oracle's norms: >= 2 clipped, >= 2 not, none within 1 % of S."""
    S = DP_CASES[case][4][z]
    ref = _oracle(case, z)
    assert_clip_decisions(ref["norm"], S)
    hip = _case_engine(HipRoundEngine, case, z)
    hip.run(DP_ROUNDS)
    st, h = hip.portable_state(), hip.history()
    err = {"weights": nerr(hip.global_flat(), ref["w"]), "exp_avg": nerr(st["exp_avg"], ref["m"]),
           "exp_avg_sq": nerr(st["exp_avg_sq"], ref["v"]),
           "loss": float(np.max(np.abs(h["loss"].astype(np.float64) - ref["loss"]) / np.abs(ref["loss"]))),
           "norm": float(np.max(np.abs(h["update_norm"].astype(np.float64) - ref["norm"]) / ref["norm"]))}
    print(case, z, err, "norm bound", norm_chain(hip.Pimg) * U)
    assert err["weights"] < 2e-5, err
    assert err["exp_avg"] < 2e-5, err
    assert err["exp_avg_sq"] < 2e-5, err
    np.testing.assert_allclose(h["loss"], ref["loss"], rtol=1e-4)
    assert h["update_norm"].shape == (DP_ROUNDS,)
    np.testing.assert_allclose(h["update_norm"], ref["norm"], rtol=norm_chain(hip.Pimg) * U)
    assert "update_norm" not in _plain_engine().history()


@functools.lru_cache(maxsize=None)
def _plain_engine():
    X, y = make_multiclass(96, 17, 3, DATA_SEED)
    e = HipRoundEngine(X, y, 3, EngineConfig(hidden=(24,), max_rounds=4, early_stop=False, graph_rounds=0), None,
                       init_flat([17, 24, 3], INIT_SEED))
    e.run(2)
    return e


def test_defaults_launch_nothing_new():
    e = _plain_engine()
    assert e.layout["dp"] is False and bool(e.engine.fused)
    tr = e.trace(1)
    assert "dp" not in tr and "dp" not in tr["launches"]
    d = _case_engine(HipRoundEngine, "small", DP_Z)
    tr = d.trace(2, close=True)
    assert tr["launches"]["dp"] == 2 and tr["dp"] > 0, tr
    # the profiling re-launchers would republish the un-noised contribution
    with pytest.raises(RuntimeError, match="not on a DP engine"):
        d.engine.time_kernels(d.rounds_issued - 1, 1, d.stream.cuda_stream)
    with pytest.raises(RuntimeError, match="not on a DP engine"):
        d.engine.launch_one(d.rounds_issued - 1, 1, d.stream.cuda_stream)


# ---- 3, 6: client groups ----
# Four IID shards of 300 rows (seed 2), z = 0.02; the torch group's norms per client:
#   all clients sampled:  0.42 in round 0, 0.2985 .. 0.3019 in round 1, 0.246 .. 0.279 afterwards -> S = 0.285
#   participation 0.5:    0.42 / 0.35 .. 0.37 (clients 0, 1) and 0.295 .. 0.32 (clients 2, 3)       -> S = 0.34
GROUP_S = {1.0: 0.285, 0.5: 0.34}


def _group(backend, participation=1.0):
    X, y = make_multiclass(1200, 14, 2, DATA_SEED)
    cfg = EngineConfig(max_rounds=8, early_stop=False, dp_clip=GROUP_S[participation], dp_noise=DP_Z,
                       dp_seed=DP_SEED, participation=participation)
    return ClientGroup(X, y, 4, cfg, backend=backend, shard_mode="iid", seed=2)


@functools.lru_cache(maxsize=None)
def _group_oracle(participation):
    g = _group("torch", participation=participation)
    g.run(DP_ROUNDS)
    return g


def test_client_group_hip_matches_torch():
    """Four clients, z = 0.02, six rounds: global weights, every client's moments and the loss
    within the bounds of test_dp_rounds_match_torch_oracle; every client's update norms too."""
    ref = _group_oracle(1.0)
    hip = _group("hip")
    hip.run(DP_ROUNDS)
    L = norm_chain(hip.clients[0].Pimg)
    print("group weights", nerr(hip.global_flat(), ref.global_flat()))
    assert nerr(hip.global_flat(), ref.global_flat()) < 2e-5
    np.testing.assert_allclose(hip.history()["loss"], ref.history()["loss"], rtol=1e-4)
    for a, b in zip(hip.clients, ref.clients):
        sa, sb = a.portable_state(), b.portable_state()
        assert nerr(sa["exp_avg"], sb["exp_avg"]) < 2e-5 and nerr(sa["exp_avg_sq"], sb["exp_avg_sq"]) < 2e-5
        nb = b.history()["update_norm"].astype(np.float64)
        assert np.min(np.abs(nb - GROUP_S[1.0])) >= 0.01 * GROUP_S[1.0], nb
        print("client", a.rank, "norms", nb, "err", np.max(np.abs(a.history()["update_norm"] - nb) / nb))
        np.testing.assert_allclose(a.history()["update_norm"], nb, rtol=L * U)
    nall = np.stack([c.history()["update_norm"] for c in ref.clients])
    assert (nall > GROUP_S[1.0]).sum() >= 8 and (nall < GROUP_S[1.0]).sum() >= 8


def test_unsampled_clients_record_zero_and_contribute_zeros():
    """participation = 0.5 of four clients: a client that sits a round out records norm 0 and its
    contribution image is exactly zero (no noise); the sampled ones' norms equal the oracle's."""
    ref = _group_oracle(0.5)
    g = _group("hip", participation=0.5)
    s = g.stream.cuda_stream
    seen = set()
    for r in range(4):
        part = set(int(k) for k in g.clients[0].participants(r))
        assert len(part) == 2
        for e in g.clients:
            e.engine.run_local(r, s)
        g.stream.synchronize()
        bufs = [e.params[(r + 1) & 1] for e in g.clients]
        for e, b in zip(g.clients, bufs):
            img = b[:e.Pimg]
            if e.rank in part:
                assert float(img.abs().max()) > 0
            else:
                assert not bool(img.any()), (r, e.rank)
                seen.add(e.rank)
        with torch.cuda.stream(g.stream):       # the group's rank-order sum (ClientGroup._round_hip)
            tot = bufs[0].clone()
            for b in bufs[1:]:
                tot += b
            for b in bufs:
                b.copy_(tot)
        for e in g.clients:
            e.rounds_issued = r + 1
    g.sync_history()
    assert len(seen) >= 2
    L = norm_chain(g.clients[0].Pimg)
    for e, o in zip(g.clients, ref.clients):
        n, no = e.history()["update_norm"], o.history()["update_norm"][:4]
        for r in range(4):
            sampled = e.rank in e.participants(r)
            assert (n[r] > 0) == sampled and (no[r] > 0) == sampled, (e.rank, r, n, no)
        assert np.min(np.abs(no[no > 0] - GROUP_S[0.5])) >= 0.01 * GROUP_S[0.5], no
        np.testing.assert_allclose(n, no, rtol=L * U)


# ---- 4: early stop ----
def test_rounds_past_an_early_stop_leave_the_global_image_alone():
    """Patience 1 with a loose tolerance stops after round 1; a 4-round graph and eager rounds issued
    past the stop (12 in all) leave the model of a run that issued exactly two rounds, bit for bit,
    and spend no history slots."""
    X, y = make_multiclass(300, 14, 2, DATA_SEED)
    flat = init_flat([14, 50, 200, 2], INIT_SEED)
    mk = lambda g: HipRoundEngine(X, y, 2, EngineConfig(max_rounds=16, patience=1, tolerance=0.5, graph_rounds=g,
                                                        dp_clip=0.37, dp_noise=KERNEL_Z, dp_seed=DP_SEED), None, flat)
    a, b = mk(4), mk(0)
    a.run(12)
    b.run(2, check_every=2)
    assert a.rounds_issued == 12 and b.rounds_issued == 2
    ha, hb = a.history(), b.history()
    assert ha["stop_round"] == hb["stop_round"] == 2 and ha["rounds_run"] == hb["rounds_run"] == 2
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    np.testing.assert_array_equal(ha["update_norm"], hb["update_norm"])
    assert not a.dp_norm[2:].any()


# ---- 5: stateless resume ----
@pytest.mark.parametrize("seed", [DP_SEED, None], ids=["int-seed", "private-seed"])
def test_resume_continues_the_noise_stream(seed):
    X, y = make_multiclass(300, 14, 2, DATA_SEED)
    flat = init_flat([14, 50, 200, 2], INIT_SEED)
    mk = lambda: HipRoundEngine(X, y, 2, EngineConfig(max_rounds=8, early_stop=False, graph_rounds=0, dp_clip=0.37,
                                                      dp_noise=DP_Z, dp_seed=seed), None, flat)
    a = mk()
    a.run(3)
    st = a.portable_state()
    assert st["dp_seed"] == a.dp_seed
    b = mk()
    if seed is None:
        assert b.dp_seed != a.dp_seed
    b.load_portable_state(st)
    assert b.dp_seed == a.dp_seed
    a.run(3)
    b.run(3)
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    np.testing.assert_array_equal(a.local_flat(), b.local_flat())
    ha, hb = a.history(), b.history()
    assert ha["rounds_run"] == hb["rounds_run"] == 6
    np.testing.assert_array_equal(ha["update_norm"], hb["update_norm"])
    np.testing.assert_array_equal(ha["loss"], hb["loss"])
    if seed is not None:   # ... and equals the uninterrupted run of a third engine
        c = mk()
        c.run(6)
        np.testing.assert_array_equal(c.global_flat(), b.global_flat())


# ---- 8: trial batches ----
def test_trial_batch_and_fed_sweep_refuse_dp():
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    from fedmi.ops import native
    X, y = make_multiclass(96, 17, 3, DATA_SEED)
    base = EngineConfig(hidden=(24,), max_rounds=4, early_stop=False, dp_clip=0.0863, dp_noise=DP_Z, dp_seed=DP_SEED)
    with pytest.raises(ValueError, match="differentially private"):
        FedTrialGroup(X, y, 3, [FedTrial((24,), 0.004, 1)], None, base, backend="hip")
    e = HipRoundEngine(X, y, 3, base, None, init_flat([17, 24, 3], INIT_SEED))
    tb = native().TrialBatch([e.engine])
    with pytest.raises(RuntimeError, match="trial batch: no DP"):
        tb.run(0, 1, e.stream.cuda_stream, True)
    e.run(2)   # the refused batch left the engine's bookkeeping as it was
    assert e.history()["rounds_run"] == 2


# ---- 9: graph replay ----
def test_graph_replay_equals_eager_bitwise():
    """The noise counter takes the DEVICE's round index: a 4-round graph replayed twice draws the
    noise of rounds 0..7, like eager launches."""
    out = []
    for g in (0, 4):
        e = _case_engine(HipRoundEngine, "income", DP_Z, graph_rounds=g)
        e.run(8)
        if g:
            assert e.engine.graph_captures >= 1
        out.append((e.global_flat(), e.history()))
    assert out[0][1]["rounds_run"] == out[1][1]["rounds_run"] == 8
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1]["update_norm"], out[1][1]["update_norm"])
    np.testing.assert_array_equal(out[0][1]["loss"], out[1][1]["loss"])
    assert len(set(out[0][1]["update_norm"].tolist())) == 8


# ---- 7: two ranks on the xGMI plane ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_xgmi(comm, peer, dtype, X, y, flat):
    comm.peer_allreduce = peer
    cfg = EngineConfig(max_rounds=16, early_stop=False, dtype=dtype, graph_rounds=4, dp_clip=0.37, dp_noise=DP_Z,
                       dp_seed=DP_SEED)
    e = HipRoundEngine(X, y, 2, cfg, comm, flat)
    assert e.aggregation == ("xgmi-oneshot" if peer else "host"), e.aggregation
    assert e.layout["dp"] and not e.engine.lagged and not e.engine.adam_exchange
    e.run(3)
    e.step_train()
    e.step_eval()
    e.step_aggregate()
    e.run(6)
    e.sync_history()
    return e.global_flat(), e.history()


def _xgmi_worker(rank, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    try:
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="xgmi", device="cuda:0", rccl=False)
        X, y = make_multiclass(300 + 100 * rank, 14, 2, DATA_SEED + rank)
        flat = init_flat([14, 50, 200, 2], INIT_SEED)
        res = {d: (_run_xgmi(comm, True, d, X, y, flat), _run_xgmi(comm, False, d, X, y, flat))
               for d in ("fp32", "bf16")}
        torch.cuda.synchronize()
        comm.Barrier()
        q.put((rank, res, None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_two_ranks_xgmi_plane_equals_host_aggregation_bitwise():
    """Two ranks sharing one GPU: DP rounds (eager, step API, 4-round graphs) through the one-shot
    xGMI all-reduce equal the same engines aggregating through the host, bit for bit; both ranks hold
    one model."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_xgmi_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=110) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=30)
    for rank, res, err in out:
        assert err is None, f"rank {rank}:\n{err}"
        for dtype in ("fp32", "bf16"):
            (wa, ha), (wb, hb) = res[dtype]
            assert ha["rounds_run"] == hb["rounds_run"] == 10
            np.testing.assert_array_equal(wa, wb, err_msg=f"{dtype} weights")
            np.testing.assert_array_equal(ha["global"], hb["global"])
            np.testing.assert_array_equal(ha["loss"], hb["loss"])
            np.testing.assert_array_equal(ha["update_norm"], hb["update_norm"])
            assert (ha["update_norm"] > 0).all()
    for dtype in ("fp32", "bf16"):
        np.testing.assert_array_equal(out[0][1][dtype][0][0], out[1][1][dtype][0][0])
    for p in procs:
        assert p.exitcode == 0

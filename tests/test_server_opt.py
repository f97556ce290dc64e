"""Server optimizers on the GPU: the server-step kernel (fl_server.hip) against a float64 model of its
own inputs, its packed bf16 image against the stand-alone pack, rounds against the float64 and torch
oracles, and the engine paths around it (client groups, client sampling, DP, early stop, graphs,
resume, the xGMI plane, the refusals).  Shapes and settings: tests/server_oracle.py.
"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.engine import EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, image_to_dense, init_flat

from .dp_oracle import DP_SEED, DP_Z
from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr
from .server_oracle import (OPTS, SERVER_ROUNDS, SERVER_SHAPES, Float64GroupOracle, Float64ServerOracle, server_cfg,
                            server_scalars, server_step_f64, shape_data)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


def _hip(opt, shape="income", **kw):
    X, y, C, flat = shape_data(shape)
    return HipRoundEngine(X, y, C, server_cfg(opt, shape, **kw), None, flat)


def _dense(e, img):
    return image_to_dense(np.asarray(img.cpu().numpy() if isinstance(img, torch.Tensor) else img), e.dims)


def _server_state(e):
    e.stream.synchronize()
    return _dense(e, e.server_m), _dense(e, e.server_v)


# ---- 1: the kernel against its own inputs ----
def step_bounds(x, a, m, v, cfg):
    """float64 step of the fp32 inputs with the kernel's fp32 scalars, and the elementwise bounds of
    the kernel's operation chain (fl_server.hip; every operation is one correctly rounded fp32
    operation of relative error <= u = 2^-24; second-order terms are covered by the factor 1.001).

      d  = sub(a, x):                          |err d| <= u |d|
      sgd      m' = fma(b1, m, d):             |err m'| <= u |d| + u |m'|
               new = fma(lr, m', x):           |err new| <= lr |err m'| + u |new|
      adaptive m' = fma(b1, m, mul(c1, d)):    |err m'| <= 2 u c1 |d| + u |m'|          (c1 = 1 - b1)
      adagrad  v' = fma(d, d, v):              |err v'| <= 2 u d^2 + u v'
      adam     v' = fma(b2, v, mul(c2, mul(d, d))): |err v'| <= 4 u c2 d^2 + u v'       (c2 = 1 - b2)
      yogi     v' = v -/+ mul(c2, mul(d, d)):  |err v'| <= 4 u c2 d^2 + u v'  where the sign of
               sub(v, mul(d, d)) is that of v - d^2, i.e. where |v - d^2| > 3 u d^2 (4 u d^2 excluded)
      s = sqrt(v'):  |err s| <= s (|err v'| / (2 v') + u);   den = add(s, tau): |err den| <= |err s| + u den
      q = div(m', den): |err q| <= |q| (|err den| / den + u) + |err m'| / den
      new = fma(lr, q, x): |err new| <= lr |err q| + u |new|

    Returns (new, m', v', bound_new, bound_m, bound_v, undecidable-sign mask)."""
    lr, b1, c1, b2, c2, tau = server_scalars(cfg, fp32=True)
    x, a, m = (np.asarray(t, np.float64) for t in (x, a, m))
    new, mn, vn = server_step_f64(x, a, m, v, cfg, fp32_scalars=True)
    d = a - x
    skip = np.zeros(x.shape, bool)
    if cfg.server_opt == "sgd":
        bm = U * np.abs(d) + U * np.abs(mn)
        bn = lr * bm + U * np.abs(new)
        return new, mn, None, 1.001 * bn, 1.001 * bm, None, skip
    bm = 2 * U * c1 * np.abs(d) + U * np.abs(mn)
    d2 = d * d
    if cfg.server_opt == "adagrad":
        bv = 2 * U * d2 + U * vn
    else:
        bv = 4 * U * c2 * d2 + U * vn
    if cfg.server_opt == "yogi":
        skip = np.abs(np.asarray(v, np.float64) - d2) <= 4 * U * d2
    s = np.sqrt(vn)
    bs = s * (bv / (2 * vn) + U)
    den = s + tau
    bden = bs + U * den
    q = mn / den
    bq = np.abs(q) * (bden / den + U) + bm / den
    bn = lr * bq + U * np.abs(new)
    return new, mn, vn, 1.001 * bn, 1.001 * bm, 1.001 * bv, skip


def _check_step(e, r, tag, worst):
    """Round r's server step through the step API: snapshot (x, a, m, v), step, compare."""
    cfg, Pimg = e.cfg, e.Pimg
    e.stream.synchronize()
    x_img = e.params[r & 1][:Pimg].cpu().numpy()
    a_buf = e.params[(r + 1) & 1].cpu().numpy()
    m_img, v_img = e.server_m.cpu().numpy(), e.server_v.cpu().numpy()
    e.step_aggregate()
    e.stream.synchronize()
    out_buf = e.params[(r + 1) & 1].cpu().numpy()
    m_out, v_out = e.server_m.cpu().numpy(), e.server_v.cpu().numpy()
    # padding exact, tails untouched
    pad = dense_to_image(np.ones(e.P, np.float32), e.dims) == 0
    assert pad.sum() == Pimg - e.P and pad.any()
    tau2 = np.float32(float(np.float32(cfg.server_tau)) ** 2)
    assert not out_buf[:Pimg][pad].any() and not m_out[pad].any(), f"{tag}: padding written"
    assert (v_out[pad] == tau2).all(), f"{tag}: v padding changed"
    np.testing.assert_array_equal(out_buf[Pimg:], a_buf[Pimg:], err_msg=f"{tag}: tails written")
    assert out_buf.size > Pimg and a_buf[Pimg:].any()
    if cfg.server_opt == "sgd":
        np.testing.assert_array_equal(v_out, v_img)
    x, a, m, v, out, mo, vo = (_dense(e, t).astype(np.float64) for t in (x_img, a_buf[:Pimg], m_img, v_img,
                                                                          out_buf[:Pimg], m_out, v_out))
    new, mn, vn, bn, bm, bv, skip = step_bounds(x, a, m, v, cfg)
    n_skip = int(skip.sum())
    print(tag, "round", r, "excluded (yogi sign)", n_skip, "of", e.P)
    assert n_skip <= e.P // 1000, (tag, n_skip)
    assert bn.max() <= 1e-5 * np.abs(new).max(), (tag, bn.max(), np.abs(new).max())   # not vacuous
    keep = ~skip
    tiny = 1e-300   # (an exact zero against a zero bound, e.g. a dead unit's d = m = 0, is ratio 0)
    ratios = {"new": np.abs(out - new)[keep] / np.maximum(bn[keep], tiny),
              "m": np.abs(mo - mn)[keep] / np.maximum(bm[keep], tiny)}
    if vn is not None:
        ratios["v"] = np.abs(vo - vn)[keep] / np.maximum(bv[keep], tiny)
    ratios = {k: float(t.max()) for k, t in ratios.items()}
    print(tag, "round", r, "max err / bound", ratios, "max err", float(np.abs(out - new).max()))
    worst.append(max(ratios.values()))
    assert all(t <= 1.0 for t in ratios.values()), (tag, r, ratios)
    assert np.abs(out - a).max() > 0   # the step changed the image


@pytest.mark.parametrize("shape", sorted(SERVER_SHAPES))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("opt", OPTS)
def test_kernel_matches_float64_model_of_its_inputs(opt, dtype, shape):
    """Three step-API rounds (so m and v are non-trivial from round 1 on): the new image, m and v
    against server_step_f64 of the fp32 inputs within the elementwise bounds derived in step_bounds,
    which must stay below 1e-5 of max|new| (they come out near 1e-7).  Padding exact (image and m 0,
    v tau^2), tails untouched, two runs bitwise equal.  Worst measured err / bound over all cases:
    0.98 (income, sgd, fp32; docs/ARCHITECTURE.md)."""
    outs, worst = [], []
    for run in range(2):
        e = _hip(opt, shape, dtype=dtype)
        assert e.layout["server_opt"] == opt and not e.engine.fused and not e.engine.lagged
        for r in range(3):
            e.step_train()
            e.step_eval()
            _check_step(e, r, f"{shape} {opt} {dtype}", worst)
        outs.append((e.global_flat(), *_server_state(e), e.local_flat()))
    print(shape, opt, dtype, "worst err / bound", max(worst))
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


# ---- 2: the packed bf16 image ----
@pytest.mark.parametrize("shape", sorted(SERVER_SHAPES))
def test_bf16_server_step_packs_what_the_pack_kernel_packs(shape):
    e = _hip("adam", shape, dtype="bf16")
    e.run(1)
    pk = e.engine.packed_global(e.stream.cuda_stream)
    g = e.global_flat()
    assert np.abs(g - e.local_flat()).max() > 1e-4   # the new global model is not the Adam-packed local one
    X, y, C, _ = shape_data(shape)
    f = HipRoundEngine(X, y, C, EngineConfig(hidden=e.cfg.hidden, max_rounds=4, early_stop=False, graph_rounds=0,
                                             dtype="bf16"), None, g)
    f.run(1)   # its first round runs the stand-alone pack of the image it was initialised from
    want = f.engine.packed_global(f.stream.cuda_stream)
    assert len(pk) == len(want) > 0 and any(want)
    assert pk == want
    tr = e.trace(2, close=True)
    assert tr["launches"]["server"] == 2 and "pack" not in tr["launches"], tr
    # ... and the round after trains from it: bitwise the gradient partials of a fresh engine
    h = _hip("adam", shape, dtype="bf16")
    h.run(1)
    h.step_train()
    h.stream.synchronize()
    f2 = HipRoundEngine(X, y, C, EngineConfig(hidden=e.cfg.hidden, max_rounds=4, early_stop=False, graph_rounds=0,
                                              dtype="bf16"), None, g)
    f2.step_train()
    f2.stream.synchronize()
    assert torch.equal(h.slab_partials(), f2.slab_partials())


# ---- 3: rounds against the oracles ----
@functools.lru_cache(maxsize=None)
def _oracles(opt, shape):
    """Six rounds of the fp32 torch engine and of the float64 oracle, once per case (read-only)."""
    X, y, C, flat = shape_data(shape)
    cfg = server_cfg(opt, shape)
    t = TorchRoundEngine(X, y, C, cfg, None, flat)
    t.run(SERVER_ROUNDS)
    o = Float64ServerOracle(X, y, C, cfg, flat)
    o.run(SERVER_ROUNDS)
    st = t.portable_state()
    out = {"t_w": t.global_flat(), "t_m": st["exp_avg"], "t_v": st["exp_avg_sq"], "t_loss": t.history()["loss"],
           "t_sm": st["server_m"], "t_sv": st["server_v"], "o_w": o.weights(), "o_sm": o.server_m,
           "o_sv": o.server_v if o.server_v is not None else np.zeros(0)}
    for a in out.values():
        a.setflags(write=False)
    return out


def _assert_rule(opt, tag, hip, ref, moments=True, state=("w", "sm", "sv")):
    """sgd: the project's bounds against the torch engine (weights and client moments nerr < 2e-5,
    loss rtol 1e-4).  Adaptive: HIP-to-float64 nerr of weights, server m and v at most 4 times the
    fp32 torch engine's own error against the same float64 oracle."""
    if opt == "sgd":
        err = {k: nerr(hip[k], ref["t_" + k]) for k in (("w", "m", "v") if moments else ("w",))}
        print(tag, "HIP vs torch", {k: f"{v:.2g}" for k, v in err.items()})
        assert max(err.values()) < 2e-5, (tag, err)
        np.testing.assert_allclose(hip["loss"], ref["t_loss"], rtol=1e-4)
        return
    for k in state:
        eh, et = nerr(hip[k], ref["o_" + k]), nerr(ref["t_" + k], ref["o_" + k])
        print(tag, k, f"HIP vs float64 {eh:.3g}  torch vs float64 {et:.3g}  ratio {eh / et:.2f}")
        assert eh <= 4 * et, (tag, k, eh, et)


@pytest.mark.parametrize("shape", sorted(SERVER_SHAPES))
@pytest.mark.parametrize("opt", OPTS)
def test_rounds_match_the_oracles(opt, shape):
    ref = _oracles(opt, shape)
    e = _hip(opt, shape)
    e.run(SERVER_ROUNDS)
    st = e.portable_state()
    assert st["server_m"].shape == (e.P,) and st["server_v"].shape == (e.P,)
    hip = {"w": e.global_flat(), "m": st["exp_avg"], "v": st["exp_avg_sq"], "loss": e.history()["loss"],
           "sm": st["server_m"], "sv": st["server_v"]}
    _assert_rule(opt, f"{shape} {opt}", hip, ref)


# ---- 4: client groups ----
# name -> (optimizer, settings off tests/server_oracle.py's, rule)
GROUP_EPS = 1e-4   # the clients' Adam eps of the case held to the torch group (see the test's docstring)
GROUP_CASES = {"sgd": ("sgd", dict(eps=GROUP_EPS), "torch"), "sgd-eps-1e-8": ("sgd", {}, "float64"),
               "adam": ("adam", {}, "float64")}


def _group(backend, case, participation):
    opt, kw, _ = GROUP_CASES[case]
    X, y = make_multiclass(1200, 14, 2, DATA_SEED)
    return ClientGroup(X, y, 4, server_cfg(opt, participation=participation, **kw), backend=backend, shard_mode="iid",
                       seed=2)


@functools.lru_cache(maxsize=None)
def _group_oracles(case, participation):
    torch.set_num_threads(1)   # the torch group's roundings depend on the thread count (as tests/test_simulate.py pins it)
    g = _group("torch", case, participation)
    g.run(SERVER_ROUNDS)
    lead = g.clients[0]
    shards = [(c.X.numpy(), c.y.numpy()) for c in g.clients]
    flat = init_flat([14, 50, 200, 2], 2 * 1000003)   # the group's common starting model (seed 2)
    o = Float64GroupOracle(shards, 2, lead.cfg, flat, lead.participants)
    o.run(SERVER_ROUNDS)
    return g, {"t_w": g.global_flat(), "t_loss": g.history()["loss"], "t_sm": lead.server_m.numpy(),
               "t_sv": lead.server_v.numpy(), "o_w": o.x, "o_sm": o.server_m,
               "o_sv": o.server_v if o.server_v is not None else np.zeros(0)}


@pytest.mark.parametrize("participation", [1.0, 0.5])
@pytest.mark.parametrize("case", sorted(GROUP_CASES))
def test_client_group_hip_matches_torch(case, participation):
    """Four IID clients, six rounds, all sampled / two of four per round, under the rule of
    test_rounds_match_the_oracles; every client, sampled or not, steps the same server state.

    FedAvgM (lr 1, momentum 0.9) is held to the project's 2e-5 against the torch group, with the
    clients' Adam eps at 1e-4.  Reasoning: a client's early Adam steps are lr m^ / (sqrt(v^) + eps),
    about lr g / (|g| + eps) in its first step, whose sensitivity to the gradient's own fp32 rounding
    grows like lr / eps where |g| is small.  In a group that happens in every round in which a
    client takes its first steps (with two of four sampled: rounds 0, 1 and 2), each sampled client
    counts 1/2 instead of 1/4, and server momentum re-applies what entered the global model up to
    1 / (1 - b1) = 10 times.  With the default eps = 1e-8 the fp32 TORCH group is therefore 2.4e-5 (all
    sampled) and 4.7e-5 (two of four) from the float64 group oracle after six rounds -- one coordinate
    (dense index 5330) is 1.2e-5 off after round 0 alone -- and 1.4e-5 .. 5.9e-5 over shard / init seeds
    2..7 at momentum 0.5: the reference's own error exceeds the bound, whatever is compared with it.
    At eps = 1e-6 / 1e-4 / 1e-3 it is 1.1e-6 / 5.8e-7 / 6.5e-7 (all sampled) and 3.3e-6 / 1.0e-6 /
    8.2e-7 (two of four); the case runs at 1e-4 and asserts, on the two references alone, that the
    torch group is within a quarter of the bound (5e-6) of the float64 oracle, the project's
    convention for a reference (tests/test_dp_cpu.py).  The same groups at the default eps
    ('sgd-eps-1e-8') and FedAdam are held to the float64 rule (HIP error <= 4 x the torch group's own)."""
    opt, _, rule = GROUP_CASES[case]
    tg, ref = _group_oracles(case, participation)
    g = _group("hip", case, participation)
    g.run(SERVER_ROUNDS)
    lead = g.clients[0]
    sm, sv = _server_state(lead)
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), lead.global_flat())
        for a, b in zip(_server_state(c), (sm, sv)):
            np.testing.assert_array_equal(a, b)
    hip = {"w": g.global_flat(), "loss": g.history()["loss"], "sm": sm, "sv": sv}
    if rule == "torch":
        cond = nerr(ref["t_w"], ref["o_w"])
        print(f"group {case} p{participation}: torch group vs float64 oracle {cond:.3g}")
        assert cond <= 5e-6, cond   # the reference is well conditioned (no HIP result enters here)
        for a, b in zip(g.clients, tg.clients):
            sa, sb = a.portable_state(), b.portable_state()
            err = (nerr(sa["exp_avg"], sb["exp_avg"]), nerr(sa["exp_avg_sq"], sb["exp_avg_sq"]))
            print("client", a.rank, "moments", err)
            assert max(err) < 2e-5, (a.rank, err)
    _assert_rule(opt if rule == "torch" else "adaptive", f"group {case} p{participation}", hip, ref, moments=False,
                 state=("w", "sm") if opt == "sgd" else ("w", "sm", "sv"))


# ---- 5: server momentum with DP ----
def test_server_momentum_consumes_the_noised_sum():
    """sgd + DP (S = 0.37, z = 0.02, the DP tests' seed): through the step API the server step's
    input `a` is the clipped, noised contribution fl_dp.hip left in the buffer (it differs from the
    local model), and its output follows step_bounds; six rounds against the torch engine within the
    sgd rule."""
    kw = dict(dp_clip=0.37, dp_noise=DP_Z, dp_seed=DP_SEED)
    e = _hip("sgd", **kw)
    worst = []
    for r in range(2):
        e.step_train()
        e.step_eval()
        e.stream.synchronize()
        a = _dense(e, e.params[(r + 1) & 1][:e.Pimg])
        assert np.abs(a - e.local_flat()).max() > 1e-4   # noised (and in round 0 clipped)
        _check_step(e, r, "sgd+dp", worst)
    X, y, C, flat = shape_data("income")
    t = TorchRoundEngine(X, y, C, server_cfg("sgd", **kw), None, flat)
    t.run(SERVER_ROUNDS)
    h = _hip("sgd", **kw)
    h.run(SERVER_ROUNDS)
    st, ts = h.portable_state(), t.portable_state()
    ref = {"t_w": t.global_flat(), "t_m": ts["exp_avg"], "t_v": ts["exp_avg_sq"], "t_loss": t.history()["loss"]}
    hip = {"w": h.global_flat(), "m": st["exp_avg"], "v": st["exp_avg_sq"], "loss": h.history()["loss"]}
    _assert_rule("sgd", "sgd+dp", hip, ref)
    np.testing.assert_allclose(h.history()["update_norm"], t.history()["update_norm"], rtol=1e-5)


# ---- 6: early stop ----
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rounds_past_an_early_stop_change_nothing(dtype):
    """Patience 1 with a loose tolerance stops after round 1; ten more rounds (a 4-round graph and
    eager ones) leave the global image and m / v of a run that issued exactly two rounds."""
    mk = lambda g: _hip("yogi", max_rounds=16, early_stop=True, patience=1, tolerance=0.5, graph_rounds=g, dtype=dtype)
    a, b = mk(4), mk(0)
    b.run(2, check_every=2)
    snap = (b.global_flat(), *_server_state(b))
    a.run(12)
    assert a.rounds_issued == 12 and b.rounds_issued == 2
    ha, hb = a.history(), b.history()
    assert ha["stop_round"] == hb["stop_round"] == 2 and ha["rounds_run"] == hb["rounds_run"] == 2
    for x, y in zip((a.global_flat(), *_server_state(a)), snap):
        np.testing.assert_array_equal(x, y)
    assert np.abs(snap[1]).max() > 0


# ---- 7: graphs and resume ----
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_graph_replay_equals_eager_bitwise(opt, dtype):
    out = []
    for g in (0, 4):
        e = _hip(opt, max_rounds=10, graph_rounds=g, dtype=dtype)
        e.run(8)
        if g:
            assert e.engine.graph_captures >= 1
        out.append((e.global_flat(), *_server_state(e), e.history()["loss"]))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_resume_from_a_checkpoint_continues_bitwise(dtype, tmp_path):
    from fedmi.ckpt.checkpoint import resume, save_checkpoint
    a = _hip("yogi", dtype=dtype)
    a.run(3)
    save_checkpoint(str(tmp_path), a)
    b = _hip("yogi", dtype=dtype)
    assert resume(str(tmp_path), b) == 3
    for x, y in zip(_server_state(a), _server_state(b)):
        np.testing.assert_array_equal(x, y)
    b.run(3)
    c = _hip("yogi", dtype=dtype)
    c.run(6)
    for x, y in zip((b.global_flat(), b.local_flat(), *_server_state(b), b.history()["loss"]),
                    (c.global_flat(), c.local_flat(), *_server_state(c), c.history()["loss"])):
        np.testing.assert_array_equal(x, y)
    X, y, C, flat = shape_data("income")
    plain = HipRoundEngine(X, y, C, EngineConfig(max_rounds=8, early_stop=False, graph_rounds=0, dtype=dtype), None, flat)
    with pytest.raises(ValueError, match="server optimizer"):
        resume(str(tmp_path), plain)
    with pytest.raises(ValueError, match="server optimizer"):
        _hip("sgd", dtype=dtype).load_portable_state(plain.portable_state())


# ---- 8: two ranks on the xGMI plane ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_xgmi(comm, peer, dtype, X, y, flat):
    comm.peer_allreduce = peer
    e = HipRoundEngine(X, y, 2, server_cfg("adam", max_rounds=16, dtype=dtype, graph_rounds=4), comm, flat)
    assert e.aggregation == ("xgmi-oneshot" if peer else "host"), e.aggregation
    assert e.layout["server_opt"] == "adam" and not e.engine.lagged and not e.engine.adam_exchange
    e.run(3)
    e.step_train()
    e.step_eval()
    e.step_aggregate()
    e.run(6)
    e.sync_history()
    return (e.global_flat(), *_server_state(e)), e.history()


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
    """Two ranks sharing one GPU: server-optimizer rounds (eager, step API, 4-round graphs) through
    the one-shot xGMI all-reduce equal the same engines aggregating through the host, bit for bit;
    both ranks hold one model and one server state."""
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
            (sa, ha), (sb, hb) = res[dtype]
            assert ha["rounds_run"] == hb["rounds_run"] == 10
            for a, b in zip(sa, sb):
                np.testing.assert_array_equal(a, b, err_msg=f"{dtype}: xGMI plane != host plane")
            np.testing.assert_array_equal(ha["global"], hb["global"])
            np.testing.assert_array_equal(ha["loss"], hb["loss"])
            assert np.abs(sa[1]).max() > 0
    for dtype in ("fp32", "bf16"):
        for a, b in zip(out[0][1][dtype][0][0], out[1][1][dtype][0][0]):
            np.testing.assert_array_equal(a, b, err_msg=f"{dtype}: ranks differ")
    for p in procs:
        assert p.exitcode == 0


# ---- 9: defaults and refusals ----
def test_defaults_launch_nothing_new_and_refusals():
    X, y, C, flat = shape_data("small")
    e = HipRoundEngine(X, y, C, EngineConfig(hidden=(24,), max_rounds=6, early_stop=False, graph_rounds=0), None, flat)
    e.run(2)
    assert e.layout["server_opt"] == "none" and bool(e.engine.fused)
    tr = e.trace(1)
    assert "server" not in tr and "server" not in tr["launches"]
    assert not hasattr(e, "server_m") and "server_m" not in e.portable_state()
    with pytest.raises(RuntimeError, match="no server optimizer"):
        e.engine.phase(e.rounds_issued, 3, e.stream.cuda_stream, None)
    d = _hip("adam", "small")
    tr = d.trace(2, close=True)
    assert tr["launches"]["server"] == 2 and tr["server"] > 0, tr
    # the profiling re-launchers would overwrite the new global image
    with pytest.raises(RuntimeError, match="not on a server-optimizer engine"):
        d.engine.time_kernels(d.rounds_issued - 1, 1, d.stream.cuda_stream)
    with pytest.raises(RuntimeError, match="not on a server-optimizer engine"):
        d.engine.launch_one(d.rounds_issued - 1, 1, d.stream.cuda_stream)
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    from fedmi.ops import native
    with pytest.raises(ValueError, match="server-optimizer"):
        FedTrialGroup(X, y, C, [FedTrial((24,), 0.004, 1)], None, server_cfg("adam", "small"), backend="hip")
    with pytest.raises(RuntimeError, match="no server optimizer"):
        native().TrialBatch([d.engine])
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="server optimizer"):
        WideClient(torch.zeros(4, 14, device="cuda"), torch.zeros(4, dtype=torch.long, device="cuda"), [14, 8, 2],
                   server_opt="adam")
    d.run(2)   # the refusals left the engine as it was
    assert d.history()["rounds_run"] == 4

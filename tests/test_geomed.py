"""Geometric-median aggregation on the GPU: the fl_geomed launches alone on synthetic buffers (bitwise
the numpy model ``geomed_model``), a captured graph of the launch sequence, client groups with two
Byzantine clients against the torch group and a float64 group oracle, three ranks gathering over the
host plane, and the refusals.

Accuracy measured on the MI355X (six fp32 rounds, k = 7, two tamperers, clients' Adam eps 1e-4; nerr =
max|a - b| / max|b|):

    small  17-24-3       torch vs float64 2.41e-07   HIP vs torch 3.43e-07   HIP vs float64 2.65e-07
    income 14-50-200-2   torch vs float64 3.16e-07   HIP vs torch 3.59e-07   HIP vs float64 3.23e-07
    small + server adam  torch vs float64 5.00e-07   HIP vs torch 8.86e-07   HIP vs float64 5.37e-07
    small behind multi_krum (f = 2)                  HIP vs torch 3.88e-07

Every case met the direct 2e-5 bound against the torch group; none needed the comparison through the
float64 oracle.
"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.aggregate import GEOMED_SLOT, geomed_model, geomed_scratch_floats, mask_bits
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .geomed_oracle import Float64GeomedGroupOracle, tamper_two
from .reference_oracle import DATA_SEED, make_multiclass, nerr

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL, INCOME = [17, 24, 3], [14, 50, 200, 2]
TAILS = 7
NU = 1e-6
SENTINEL = -77.0


def _same_bits(a, b, msg=""):
    """Equal bit for bit, any NaN matching any NaN (payloads are not part of the rule)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, msg
    na, nb = np.isnan(a), np.isnan(b)
    np.testing.assert_array_equal(na, nb, err_msg=msg)
    np.testing.assert_array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb], err_msg=msg)


def _state(live, r):
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"], rec["next_round"], rec["stop_round"] = int(live), r, r + 1, -1
    return torch.as_tensor(rec.view(np.uint8).copy()).to(DEV)


def _masks(K, seed):
    """Full, with holes, K_r = 1, K_r = 2 (as far as K allows)."""
    rng = np.random.default_rng(seed)
    pick = lambda n: np.isin(np.arange(K), rng.choice(K, size=n, replace=False))
    return [np.ones(K, bool), pick(max(1, (2 * K + 2) // 3)), pick(1), pick(min(2, K))]


def _rtab(masks):
    t = np.zeros((len(masks), 4), np.uint32)
    for r, m in enumerate(masks):
        bits = sum(1 << int(k) for k in np.flatnonzero(m))
        t[r, 0] = np.float32(1.0).view(np.uint32)
        t[r, 1] = np.float32(m.sum()).view(np.uint32)
        t[r, 2], t[r, 3] = bits & 0xFFFFFFFF, bits >> 32
    return torch.as_tensor(t.reshape(-1).view(np.int32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _real(dims):
    return dense_to_image(np.ones(param_count(list(dims)), np.float32), list(dims)) != 0


def _inputs(dims, K, seed):
    """[K, Pimg + TAILS]: honest clients c + 0.01 N(0, I) on the real parameters, clients 0 and K - 2 (K >= 4;
    below: 0 and K - 1) identical, a NaN client (K >= 3), a +inf and a -inf client (K >= 5), a 1e12 sign
    client (K >= 8); sentinels in the image padding of every source: NaN in client 0's, 1e30 in client 1's,
    7 in the others'."""
    pimg = image_layout(dims)[2]
    real = _real(tuple(dims))
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(pimg).astype(np.float32)
    a = np.empty((K, pimg + TAILS), np.float32)
    a[:, :pimg] = c + np.float32(0.01) * rng.standard_normal((K, pimg)).astype(np.float32)
    a[:, pimg:] = rng.standard_normal((K, TAILS)).astype(np.float32)
    a[K - 2 if K >= 4 else K - 1, :pimg] = a[0, :pimg]
    if K >= 3:
        a[K // 2, :pimg] = np.nan
    if K >= 5:
        a[1, :pimg], a[K - 1, :pimg] = np.inf, -np.inf
    if K >= 8:
        a[2, :pimg] = np.float32(1e12) * np.sign(a[2, :pimg])
    a[:, :pimg][:, ~real] = 7.0
    a[0, :pimg][~real] = np.nan
    if K >= 2:
        a[1, :pimg][~real] = 1e30
    return a, real, pimg


def _tab(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


def _launch(m, dims, T, src, dst, state, rtab, rounds, scratch, keep=None, stream=None, tabs=None):
    st, dt = tabs if tabs is not None else (_tab(src), _tab(dst))
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    m.geomed_aggregate(dims, T, NU, st.data_ptr(), len(src), dt.data_ptr(), len(dst), state.data_ptr(), rtab.data_ptr(),
                       TAILS, rounds, scratch.data_ptr(), s, *(() if keep is None else (keep.data_ptr(),)))
    if stream is None:
        torch.cuda.synchronize()


def _scratch(pimg, T):
    return torch.full((geomed_scratch_floats(pimg, T),), SENTINEL, dtype=torch.float32, device=DEV)


def _record(scratch, pimg, T, t, K):
    """(d [K], b [K], mask) of iteration t as the launches left them."""
    base = geomed_scratch_floats(pimg, T) - (T - t) * GEOMED_SLOT
    slot = scratch[base:base + GEOMED_SLOT].cpu().numpy()
    word = slot[128:130].view(np.uint32)
    return slot[64:64 + K], slot[:K], int(word[0]) | (int(word[1]) << 32)


def _fold(a):
    acc = torch.as_tensor(a[0]).clone()
    for row in a[1:]:
        acc += torch.as_tensor(row)
    return acc.numpy()


def _check_kernel(dims, K, seed):
    from fedmi.ops import native
    m = native()
    a, real, pimg = _inputs(dims, K, seed)
    assert geomed_scratch_floats(pimg, 3) == m.geomed_scratch_floats(dims, 3) and GEOMED_SLOT == m.GEOMED_SLOT
    masks = _masks(K, seed)
    rtab = _rtab(masks)
    tails = _fold(a[:, pimg:])
    finite = 0
    for T in (1, 3):
        for r, mask in enumerate(masks):
            tag = f"K={K} T={T} mask={np.flatnonzero(mask).tolist()}"
            rec = []
            model = geomed_model(a[:, :pimg], mask, real, T, NU, records=rec)
            finite += int(np.isfinite(model).all())
            if r == 0:
                assert np.isfinite(model).all(), tag   # all sampled: the bad clients are a minority at every K
            # separate buffers, one destination
            src = [torch.as_tensor(row).to(DEV) for row in a]
            dst = [torch.full((pimg + TAILS,), 7.0, device=DEV)]
            scratch = _scratch(pimg, T)
            _launch(m, dims, T, src, dst, _state(1, r), rtab, len(masks), scratch)
            out = dst[0].cpu().numpy()
            for s, row in zip(src, a):
                _same_bits(s.cpu().numpy(), row, tag + ": a source changed")
            _same_bits(out[:pimg][real], model[real], tag + ": image")
            assert (out[:pimg][~real].view(np.int32) == 0).all(), tag + ": padding"   # sentinels in every source's
            _same_bits(out[pimg:], tails, tag + ": tails")
            for t in range(T):
                d, b, word = _record(scratch, pimg, T, t, K)
                _same_bits(d, rec[t]["d"], tag + f": d of iteration {t}")
                _same_bits(b, rec[t]["b"], tag + f": b of iteration {t}")
                assert word == rec[t]["mask"], (tag, t, word, rec[t]["mask"])
            if r == 0:
                # rows of a gathered stack, Pimg + TAILS floats apart (dword-aligned only), into K destinations
                assert (pimg + TAILS) % 4 != 0
                stack = torch.as_tensor(a).to(DEV)
                many = [torch.full((pimg + TAILS,), 7.0, device=DEV) for _ in range(K)]
                _launch(m, dims, T, [stack[k] for k in range(K)], many, _state(1, r), rtab, len(masks), _scratch(pimg, T))
                for q in many:
                    _same_bits(q.cpu().numpy(), out, tag + ": stack rows, K destinations")
            if r == 1:
                # in place: every source is a destination
                _launch(m, dims, T, src, src, _state(1, r), rtab, len(masks), _scratch(pimg, T))
                for s in src:
                    _same_bits(s.cpu().numpy(), out, tag + ": in place")
    assert finite >= 2, finite   # (all clients sampled: the bad ones are a minority at every K; K_r = 1, 2 may pick them alone)
    # behind a screen: the rule runs over mask & keep
    keep_mask = np.ones(K, bool)
    if K >= 3:
        keep_mask[[K // 2, 1]] = False
    bits = mask_bits(keep_mask)
    keep = torch.tensor([bits - (1 << 64) if bits >= 1 << 63 else bits], dtype=torch.int64, device=DEV)
    both = masks[0] & keep_mask
    src = [torch.as_tensor(row).to(DEV) for row in a]
    dst = [torch.full((pimg + TAILS,), 7.0, device=DEV)]
    _launch(m, dims, 3, src, dst, _state(1, 0), rtab, len(masks), _scratch(pimg, 3), keep=keep)
    out = dst[0].cpu().numpy()
    _same_bits(out[:pimg][real], geomed_model(a[:, :pimg], both, real, 3, NU)[real], f"K={K}: keep word")
    _same_bits(out[pimg:], tails, f"K={K}: keep word, tails")
    # a state that is not live (stopped, or a round past max_rounds): the rank-order sum of the whole
    # buffer, padding included, and no scratch written
    whole = _fold(a)
    for state, rounds in ((_state(0, 0), len(masks)), (_state(1, len(masks)), len(masks)), (_state(1, -1), len(masks))):
        src = [torch.as_tensor(row).to(DEV) for row in a]
        dst = [torch.full((pimg + TAILS,), 7.0, device=DEV)]
        scratch = _scratch(pimg, 3)
        _launch(m, dims, 3, src, dst, state, rtab, rounds, scratch)
        _same_bits(dst[0].cpu().numpy(), whole, f"K={K}: not live")
        assert (scratch.cpu().numpy() == np.float32(SENTINEL)).all(), f"K={K}: not live, scratch written"


KS = [2, 3, 4, 5, 8, 9, 16, 33, 64]


@pytest.mark.parametrize("K", KS)
def test_kernel_small_image(K):
    _check_kernel(SMALL, K, 100 + K)


@pytest.mark.parametrize("K", KS)
def test_kernel_income_image(K):
    pimg = image_layout(INCOME)[2]
    assert pimg % 256 != 0      # a partial last block
    _check_kernel(INCOME, K, 7 + K)


@pytest.mark.parametrize("K", [5, 16])
def test_nobody_at_a_finite_distance_keeps_the_median(K):
    """Every client holds a NaN at one real position (and one client is +inf): the median is NaN there, no
    distance is finite, every iteration keeps z_0 -- the bits of the median launch."""
    from fedmi.ops import native
    m = native()
    a, real, pimg = _inputs(SMALL, K, 31)
    first = int(np.flatnonzero(real)[3])
    a[:, first] = np.nan
    mask = np.ones(K, bool)
    rtab = _rtab([mask])
    src = [torch.as_tensor(row).to(DEV) for row in a]
    med = [torch.zeros(pimg + TAILS, device=DEV)]
    st, dt, state = _tab(src), _tab(med), _state(1, 0)   # (named: the launch reads them after the call returns)
    m.robust_aggregate(SMALL, 1, 0.0, st.data_ptr(), K, dt.data_ptr(), 1, state.data_ptr(), rtab.data_ptr(), TAILS, 1,
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del st, dt, state
    for T in (1, 3):
        rec, tr = [], []
        model = geomed_model(a[:, :pimg], mask, real, T, NU, trace=tr, records=rec)
        assert tr == [[]] * T
        dst = [torch.full((pimg + TAILS,), 7.0, device=DEV)]
        scratch = _scratch(pimg, T)
        _launch(m, SMALL, T, src, dst, _state(1, 0), rtab, 1, scratch)
        _same_bits(dst[0].cpu().numpy(), med[0].cpu().numpy(), f"K={K} T={T}: the median")
        _same_bits(dst[0].cpu().numpy()[:pimg][real], model[real], f"K={K} T={T}: the model")
        for t in range(T):
            d, b, word = _record(scratch, pimg, T, t, K)
            assert word == 0 and np.isinf(d).all() and (b == 0).all(), (K, T, t)


@pytest.mark.parametrize("K", [4, 9])
def test_an_empty_iteration_repeats_the_last_combine(K):
    """K identical clients with 1e35 at one real position: d = 0, b = 1 / nu = 1e6, and b v overflows there, so
    z_1 holds +inf, no distance to it is finite, and iterations 1 and 2 include nobody: they must produce z_1
    again from iteration 0's weights (z_1 itself was never stored)."""
    from fedmi.ops import native
    m = native()
    a, real, pimg = _inputs(SMALL, 2, 77)
    a = np.repeat(a[:1], K, axis=0)
    a[:, :pimg][:, ~real] = 7.0
    big = int(np.flatnonzero(real)[11])
    a[:, big] = 1e35
    mask = np.ones(K, bool)
    rtab = _rtab([mask])
    rec, tr = [], []
    model = geomed_model(a[:, :pimg], mask, real, 3, NU, trace=tr, records=rec)
    assert tr == [list(range(K)), [], []] and np.isposinf(model[big]) and np.isfinite(np.delete(model, big)).all()
    assert [q["mask"] for q in rec] == [2 ** K - 1] * 3 and np.isinf(rec[2]["d"]).all()
    src = [torch.as_tensor(row).to(DEV) for row in a]
    dst = [torch.full((pimg + TAILS,), 7.0, device=DEV)]
    scratch = _scratch(pimg, 3)
    _launch(m, SMALL, 3, src, dst, _state(1, 0), rtab, 1, scratch)
    out = dst[0].cpu().numpy()
    _same_bits(out[:pimg][real], model[real], f"K={K}: image")
    assert (out[:pimg][~real].view(np.int32) == 0).all()
    for t in range(3):
        d, b, word = _record(scratch, pimg, 3, t, K)
        _same_bits(d, rec[t]["d"], f"K={K}: d of iteration {t}")
        _same_bits(b, rec[t]["b"], f"K={K}: b of iteration {t}")
        assert word == rec[t]["mask"]


def test_graph_replay_equals_eager_launches():
    """One captured graph of the T + 1 launches, replayed over four rounds whose rtab rows differ: the round
    comes from the state the launches read."""
    from fedmi.ops import native
    m = native()
    K, T = 9, 3
    a, real, pimg = _inputs(SMALL, K, 5)
    masks = _masks(K, 5)
    rtab = _rtab(masks)
    src = [torch.as_tensor(row).to(DEV) for row in a]
    eager = []
    for r in range(len(masks)):
        dst = [torch.zeros(pimg + TAILS, device=DEV)]
        _launch(m, SMALL, T, src, dst, _state(1, r), rtab, len(masks), _scratch(pimg, T))
        eager.append(dst[0].cpu().numpy())
        _same_bits(eager[-1][:pimg][real], geomed_model(a[:, :pimg], masks[r], real, T, NU)[real], f"eager round {r}")
    assert len({e.tobytes() for e in eager}) == len(masks)
    state = _state(1, 0)
    dst = [torch.zeros(pimg + TAILS, device=DEV)]
    tabs = (_tab(src), _tab(dst))
    scratch = _scratch(pimg, T)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        _launch(m, SMALL, T, src, dst, state, rtab, len(masks), scratch, stream=torch.cuda.current_stream().cuda_stream,
                tabs=tabs)
    torch.cuda.synchronize()
    for r in list(range(len(masks))) + [0]:
        state.copy_(_state(1, r))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _same_bits(dst[0].cpu().numpy(), eager[r], f"replay of round {r}")
    del tabs


# ---- groups ----
ROUNDS = 6
GROUP_EPS = 1e-4   # the clients' Adam eps of the groups held to the torch group (tests/test_server_opt.py)
SHAPES = {"small": (240, 17, 3, (24,)), "income": (1200, 14, 2, (50, 200))}
BAD = (1, 4)


def _dims(shape):
    return [SHAPES[shape][1], *SHAPES[shape][3], SHAPES[shape][2]]


def _cfg(shape, agg="geomed", **kw):
    base = dict(hidden=SHAPES[shape][3], max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, aggregator=agg,
                eps=GROUP_EPS)
    return EngineConfig(**{**base, **kw})


def _data(shape):
    rows, F, C, _ = SHAPES[shape]
    return make_multiclass(rows, F, C, DATA_SEED)


def _tamper(shape, backend):
    dims = _dims(shape)
    return tamper_two(image_layout(dims)[2] if backend == "hip" else param_count(dims), *BAD)


def _group(backend, shape, agg="geomed", k=7, rounds=ROUNDS, tampered=True, heldout=None, **kw):
    X, y = _data(shape)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, _cfg(shape, agg, **kw), backend=backend, shard_mode="iid", seed=2,
                    tamper=_tamper(shape, backend) if tampered else None, heldout=heldout)
    g.run(rounds)
    return g


@functools.lru_cache(maxsize=None)
def _references(shape, server):
    kw = dict(server_opt="adam", server_lr=1e-2) if server else {}
    g = _group("torch", shape, **kw)
    lead = g.clients[0]
    flats = [init_flat(_dims(shape), 2 * 1000003 + (0 if server else r)) for r in range(7)]
    o = Float64GeomedGroupOracle([(c.X.numpy(), c.y.numpy()) for c in g.clients], SHAPES[shape][2], lead.cfg, flats,
                                 lead.participants, tamper=tamper_two(param_count(_dims(shape)), *BAD))
    o.run(ROUNDS)
    out = {"t_w": g.global_flat(), "t_loss": g.history()["loss"].copy(), "o_w": o.x}
    for a in out.values():
        a.setflags(write=False)
    return out


def _assert_clients_agree(g):
    lead = g.clients[0]
    h = lead.history()
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), lead.global_flat())
        hc = c.history()
        for key in ("global", "loss", "per_rank"):
            np.testing.assert_array_equal(hc[key], h[key])


def _assert_weights_rule(tag, w, ref):
    """fp32 weights within the project's 2e-5 of the torch group; where the torch group is itself
    further than that from the float64 group oracle, within 4x its error of the oracle."""
    cond, et, eo = nerr(ref["t_w"], ref["o_w"]), nerr(w, ref["t_w"]), nerr(w, ref["o_w"])
    print(f"{tag}: torch vs float64 {cond:.3g}  HIP vs torch {et:.3g}  HIP vs float64 {eo:.3g}")
    if cond <= 2e-5:
        assert et <= 2e-5, (tag, et)
    else:
        assert eo <= 4 * cond, (tag, eo, cond)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_hip_group_with_two_byzantine_clients(shape):
    X, y = _data(shape)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, 7, _cfg(shape), backend="hip", shard_mode="iid", seed=2, tamper=_tamper(shape, "hip"))
    for r in range(ROUNDS):
        assert g.run(1) == 1
        assert np.isfinite(g.global_flat()).all(), r        # the global model stays finite every round
    lead = g.clients[0]
    assert lead.layout["aggregator"] == "geomed" and lead.agg_scale == 1.0
    assert lead.layout["geomed"] == {"iters": 3, "nu": float(np.float32(1e-6)), "launches": 4}
    _assert_clients_agree(g)
    ref = _references(shape, False)
    _assert_weights_rule(f"group {shape} geomed", g.global_flat(), ref)
    np.testing.assert_allclose(g.history()["loss"], ref["t_loss"], rtol=1e-4)
    # the zero-padding invariant survived a client whose whole image (padding included) was NaN
    img = lead.params[g.rounds & 1][:lead.Pimg].cpu().numpy()
    real = _real(tuple(lead.dims))
    assert (img[~real].view(np.int32) == 0).all()


def test_heldout_loss_is_finite_where_the_mean_is_poisoned():
    X, y = _data("small")
    Xv, yv = make_multiclass(64, 17, 3, DATA_SEED + 1)
    geo = _group("hip", "small", heldout=(Xv, yv))
    mean = _group("hip", "small", agg="mean", heldout=(Xv, yv))
    assert np.isfinite(geo.history()["heldout_loss"][-1])
    assert not np.isfinite(mean.history()["heldout_loss"][-1])
    assert not np.isfinite(mean.global_flat()).any()


def test_hip_group_bf16():
    a = _group("hip", "small", dtype="bf16")
    assert np.isfinite(a.global_flat()).all() and a.history()["rounds_run"] == ROUNDS
    _assert_clients_agree(a)


def test_hip_group_behind_multi_krum():
    kw = dict(screen="multi_krum", screen_byzantine=2)
    hip, ref = _group("hip", "small", **kw), _group("torch", "small", **kw)
    h = hip.history()
    np.testing.assert_array_equal(h["screen_kept"], ref.history()["screen_kept"])
    for w in h["screen_kept"]:
        assert bin(int(w)).count("1") == 5 and not any((int(w) >> k) & 1 for k in BAD)
    _assert_clients_agree(hip)
    w = hip.global_flat()
    err = nerr(w, ref.global_flat())
    print(f"group small geomed behind multi_krum: HIP vs torch {err:.3g}")
    assert np.isfinite(w).all() and err <= 2e-5, err


def test_hip_group_composes_with_a_server_optimizer():
    g = _group("hip", "small", server_opt="adam", server_lr=1e-2)
    _assert_clients_agree(g)
    assert np.isfinite(g.global_flat()).all() and np.abs(g.clients[0].server_m.cpu().numpy()).max() > 0
    ref = _references("small", True)
    _assert_weights_rule("group small geomed + server adam", g.global_flat(), ref)
    np.testing.assert_allclose(g.history()["loss"], ref["t_loss"], rtol=1e-4)


# ---- three ranks sharing one GPU ----
RANK_ROUNDS = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    try:
        from fedmi.data.sharding import shard_indices
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="xgmi", device="cuda:0", rccl=False)
        X, y = _data("small")
        idx = [shard_indices(len(X), r, world, mode="iid", seed=2, labels=y, alpha=0.5) for r in range(world)]
        e = HipRoundEngine(X[idx[rank]], y[idx[rank]], 3, _cfg("small"), comm, init_flat(SMALL, 2 * 1000003 + rank),
                           n_total=sum(len(i) for i in idx))
        agg, lay = e.aggregation, e.layout["aggregator"]
        e.run(RANK_ROUNDS)
        h = e.history()
        torch.cuda.synchronize()
        img = e.params[RANK_ROUNDS & 1][:e.Pimg].cpu().numpy()
        comm.Barrier()
        q.put((rank, (agg, lay, img, e.global_flat(), h["global"], h["loss"], h["rounds_run"]), None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_three_ranks_host_gather_equal_the_group_bitwise():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    out, failed = [], None
    try:
        for _ in range(3):
            out.append(q.get(timeout=110))
    except Exception as e:  # noqa: BLE001 -- a child hung or died: reported below, nothing more runs
        failed = repr(e)
    for p in procs:
        p.join(timeout=5 if failed else 30)
        if p.is_alive():
            p.terminate()
            p.join(timeout=10)
            failed = failed or "a rank did not exit"
    assert failed is None, failed
    out.sort(key=lambda t: t[0])
    for rank, _, err in out:
        assert err is None, f"rank {rank}:\n{err}"
    assert all(p.exitcode == 0 for p in procs)
    # (only now, with every child done and clean, the reference group runs on the GPU)
    g = _group("hip", "small", k=3, rounds=RANK_ROUNDS, tampered=False)
    lead, h = g.clients[0], g.history()
    ref = (lead.params[RANK_ROUNDS & 1][:lead.Pimg].cpu().numpy(), g.global_flat(), h["global"], h["loss"], h["rounds_run"])
    for rank, res, _ in out:
        assert res[0] == "host-gather" and res[1] == "geomed"
        for a, b in zip(res[2:], ref):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank}")


# ---- refusals ----
def test_refusals():
    from fedmi.ops import native
    X, y = _data("small")
    flat = init_flat(SMALL, 0)
    mk = lambda cfg, **kw: HipRoundEngine(X, y, 3, cfg, SimRank(3, 0, DEV), flat, n_total=3 * len(X),
                                          client_sizes=[len(X)] * 3, **kw)
    e = mk(_cfg("small"))
    assert e.aggregation == "host-gather" and e.layout["aggregator"] == "geomed" and not e.engine.lagged
    with pytest.raises(ValueError, match="gather_plane='host'"):
        mk(_cfg("small", gather_plane="xgmi"))
    one = HipRoundEngine(X, y, 3, _cfg("small", gather_plane="xgmi"), None, flat)   # one client: the identity
    assert one.aggregation == "none" and one.layout["aggregator"] == "mean" and one.robust == 0
    assert "geomed" not in one.layout
    m = native()
    pimg = image_layout(SMALL)[2]
    t = torch.zeros(pimg + TAILS, device=DEV)
    tab = _tab([t] * 65)
    args = lambda K, T, nu: (SMALL, T, nu, tab.data_ptr(), K, tab.data_ptr(), 1, _state(1, 0).data_ptr(),
                             _rtab([np.ones(min(K, 64), bool)]).data_ptr(), TAILS, 1, _scratch(pimg, 32).data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match="1..64 clients"):
        m.geomed_aggregate(*args(65, 3, NU))
    for T in (0, 33):
        with pytest.raises(RuntimeError, match="iters"):
            m.geomed_aggregate(*args(4, T, NU))
    for nu in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(RuntimeError, match="nu"):
            m.geomed_aggregate(*args(4, 3, nu))

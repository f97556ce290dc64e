"""Secure aggregation on the GPU: the fl_secagg_mask and fl_secagg_open kernels alone on synthetic
buffers against the host model (fedmi/fl/secagg.py), bit for bit; the pair against the float64 sum;
HIP client groups against the torch group; three ranks gathering over the host plane.

Bound (tests/test_secagg_cpu.py): |opened - ref| <= 1.001 (K_r 2^-(F+1) + 2^-24 |ref|) against the
float64 sum ``ref`` of the fp32 contributions, where nothing clamped.
"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine
from fedmi.fl.secagg import SECAGG_STREAM, secagg_limit, secagg_mask, secagg_open, secagg_quantize
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass, nerr

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL, INCOME = [17, 24, 3], [14, 50, 200, 2]
TAILS = 7
SEED = 0x0123456789ABCDEF
ROUNDS_TAB = 3   # rounds of the synthetic per-round table: round 1 holds the case's sampled set


def _state(live, r):
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"], rec["next_round"], rec["stop_round"] = int(live), r, r + 1, -1
    return torch.as_tensor(rec.view(np.uint8).copy()).to(DEV)


def _rtab(K, part):
    """Round 0: everyone; round 1: the case's sampled set; round 2: client 0 alone."""
    t = np.zeros((ROUNDS_TAB, 4), np.uint32)
    for r, m in enumerate((range(K), part, [0])):
        bits = sum(1 << int(k) for k in m)
        t[r, 0] = np.float32(1.0).view(np.uint32)
        t[r, 1] = np.float32(len(list(m))).view(np.uint32)
        t[r, 2], t[r, 3] = bits & 0xFFFFFFFF, bits >> 32
    return torch.as_tensor(t.reshape(-1).view(np.int32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _positions(dims):
    """Image position of every dense parameter, and the mask of real image entries."""
    dims = list(dims)
    P, pimg = param_count(dims), image_layout(dims)[2]
    img = dense_to_image(np.arange(1, P + 1, dtype=np.float32), dims)   # (P < 2^24: exact)
    real = img != 0
    pos = np.zeros(P, np.int64)
    pos[img[real].astype(np.int64) - 1] = np.flatnonzero(real)
    pos.setflags(write=False)
    real.setflags(write=False)
    return pos, real, pimg


def _inputs(dims, K, kr, seed):
    """[K, Pimg + TAILS] fp32: the images hold normals / K_r at the real parameters (+-0, values that
    clamp, NaN and +-inf planted, the last -- partial -- quad included) and +0 padding; the tails normals.
    Returns the buffers, the dense contributions and how many planted values clamp per client."""
    pos, real, pimg = _positions(tuple(dims))
    P = pos.size
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((K, P)) / kr).astype(np.float32)
    c[:, 10:14] = 0.0
    c[::2, 10:14] = -0.0
    c[:, 20] = 2.0 ** -24 * 0.5          # a tie at F = 24: rounds to even (0)
    c[:, 21] = 2.0 ** -24 * 1.5          # ... to 2
    c[0, 30], c[0, 31], c[0, P - 1] = 1e9, -1e9, np.nan
    c[K - 1, 40], c[K - 1, 41], c[K - 1, P - 2] = np.inf, -np.inf, 3e38
    a = np.zeros((K, pimg + TAILS), np.float32)
    a[:, pos] = c
    a[:, pimg:] = rng.standard_normal((K, TAILS)).astype(np.float32)
    return a, c


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _tab(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


def _mask_launch(m, dims, bits, bufs, first, state, rtab, clamps):
    bt, ct = _tab(bufs), _tab(clamps)
    m.secagg_mask(dims, bits, SEED, bt.data_ptr(), len(bufs), first, state.data_ptr(), rtab.data_ptr(), ct.data_ptr(),
                  ROUNDS_TAB, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _open_launch(m, dims, bits, src, dst, state, rtab):
    st, dt = _tab(src), _tab(dst)
    m.secagg_open(dims, bits, st.data_ptr(), len(src), dt.data_ptr(), len(dst), state.data_ptr(), rtab.data_ptr(), TAILS,
                  ROUNDS_TAB, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _fold(a):
    acc = torch.as_tensor(a[0]).clone()
    for row in a[1:]:
        acc += torch.as_tensor(row)
    return acc.numpy()


def _host_rows(c, part, r, bits):
    """The host model's masked words and clamp counts of the sampled clients."""
    ys, counts = {}, {}
    for i in part:
        q, counts[i] = secagg_quantize(c[i], bits, len(part))
        ys[i] = secagg_mask(q, i, part, r, SEED)
    return ys, counts


KERNEL_CASES = [(SMALL, 2, [0, 1]), (SMALL, 5, [0, 2, 4]), (SMALL, 8, list(range(8))), (SMALL, 64, list(range(64))),
                (INCOME, 8, list(range(8))), (SMALL, 9, [0, 2, 4, 6, 8])]
KERNEL_IDS = ["small-2", "small-3of5", "small-8", "small-64", "income-8", "small-5of9"]


# ---- 1. the mask kernel ----
@pytest.mark.parametrize("dims, K, part", KERNEL_CASES, ids=KERNEL_IDS)
def test_mask_kernel_equals_the_host_model(dims, K, part):
    from fedmi.ops import native
    m = native()
    pos, real, pimg = _positions(tuple(dims))
    assert pos.size % 4 != 0 or dims is INCOME          # 17-24-3: the last quad is partial
    rtab = _rtab(K, part)
    for bits in (24, 16):
        a, c = _inputs(dims, K, len(part), 100 + K)
        ys, counts = _host_rows(c, part, 1, bits)
        assert counts[part[0]] == 3 and counts[part[-1]] == 3 and sum(counts.values()) == 6
        bufs = [torch.as_tensor(row).to(DEV) for row in a]
        clamps = [torch.zeros(ROUNDS_TAB, dtype=torch.int32, device=DEV) for _ in range(K)]
        _mask_launch(m, dims, bits, bufs, 0, _state(1, 1), rtab, clamps)
        for i in range(K):
            out, tag = _u32(bufs[i]), f"K={K} F={bits} client {i}"
            np.testing.assert_array_equal(out[pimg:], a[i, pimg:].view(np.uint32), err_msg=tag + ": tails")
            if i in part:
                np.testing.assert_array_equal(out[pos], ys[i], err_msg=tag)        # word for word
                assert not out[:pimg][~real].any(), tag                             # padding keeps the bits of +0
                assert clamps[i].cpu().tolist() == [0, counts[i], 0], tag
            else:
                np.testing.assert_array_equal(out, a[i].view(np.uint32), err_msg=tag + ": unsampled")
                assert not clamps[i].any()
        # n = 1 with first_client = i reproduces row i of the n = K launch (a rank masking its own buffer)
        for i in (part[0], part[-1], (set(range(K)) - set(part) or {part[0]}).pop()):
            own = torch.as_tensor(a[i]).to(DEV)
            cl = torch.zeros(ROUNDS_TAB, dtype=torch.int32, device=DEV)
            _mask_launch(m, dims, bits, [own], i, _state(1, 1), rtab, [cl])
            np.testing.assert_array_equal(_u32(own), _u32(bufs[i]), err_msg=f"K={K} n=1 first_client={i}")
            assert torch.equal(cl, clamps[i])
    # round 2 samples client 0 alone: no pair, its quantised value travels unmasked
    bufs = [torch.as_tensor(row).to(DEV) for row in a]
    clamps = [torch.zeros(ROUNDS_TAB, dtype=torch.int32, device=DEV) for _ in range(K)]
    _mask_launch(m, dims, 16, bufs, 0, _state(1, 2), rtab, clamps)
    q, n = secagg_quantize(c[0], 16, 1)
    np.testing.assert_array_equal(_u32(bufs[0])[pos], q.view(np.uint32))
    assert clamps[0].cpu().tolist() == [0, 0, n]
    for i in range(1, K):
        np.testing.assert_array_equal(_u32(bufs[i]), a[i].view(np.uint32))
    # a round that is not live, or outside [0, max_rounds): nothing is touched, nothing counted
    for state in (_state(0, 1), _state(1, ROUNDS_TAB), _state(1, -1)):
        bufs = [torch.as_tensor(row).to(DEV) for row in a]
        clamps = [torch.zeros(ROUNDS_TAB, dtype=torch.int32, device=DEV) for _ in range(K)]
        _mask_launch(m, dims, 24, bufs, 0, state, rtab, clamps)
        for i in range(K):
            np.testing.assert_array_equal(_u32(bufs[i]), a[i].view(np.uint32))
            assert not clamps[i].any()


# ---- 2. the open kernel, 3. the pair against the float64 sum ----
@pytest.mark.parametrize("dims, K, part", KERNEL_CASES, ids=KERNEL_IDS)
def test_open_kernel_equals_the_host_model_and_the_pair_holds_the_bound(dims, K, part):
    from fedmi.ops import native
    m = native()
    pos, real, pimg = _positions(tuple(dims))
    rtab = _rtab(K, part)
    for bits in (24, 16):
        a, c = _inputs(dims, K, len(part), 200 + K)
        bufs = [torch.as_tensor(row).to(DEV) for row in a]
        clamps = [torch.zeros(ROUNDS_TAB, dtype=torch.int32, device=DEV) for _ in range(K)]
        _mask_launch(m, dims, bits, bufs, 0, _state(1, 1), rtab, clamps)
        masked = np.stack([b.cpu().numpy() for b in bufs])
        # NaN planted in the sources' padding (the mask kernel left +0 there) still opens to exact 0
        planted = masked.copy()
        planted[part[0], :pimg][~real] = np.nan
        src = [torch.as_tensor(row).to(DEV) for row in planted]
        dst = [torch.full((pimg + TAILS,), 7.0, device=DEV) for _ in range(2)]
        _open_launch(m, dims, bits, src, dst, _state(1, 1), rtab)
        out, tag = dst[0].cpu().numpy(), f"K={K} F={bits}"
        for s, row in zip(src, planted):
            np.testing.assert_array_equal(_u32(s), row.view(np.uint32), err_msg=tag + ": a source changed")
        np.testing.assert_array_equal(_u32(dst[1]), out.view(np.uint32), err_msg=tag + ": destinations differ")
        assert not out[:pimg][~real].view(np.uint32).any(), tag
        model = secagg_open(np.stack([masked[i].view(np.uint32)[pos] for i in part]), bits)
        np.testing.assert_array_equal(out[pos].view(np.uint32), model.view(np.uint32), err_msg=tag + ": image")
        np.testing.assert_array_equal(out[pimg:].view(np.uint32), _fold(a[:, pimg:]).view(np.uint32), err_msg=tag + ": tails")
        # in place: every source is a destination
        _open_launch(m, dims, bits, src, src, _state(1, 1), rtab)
        for s in src:
            np.testing.assert_array_equal(_u32(s), out.view(np.uint32), err_msg=tag + ": in place")
        # the pair against the float64 sum of the fp32 contributions, where nothing clamped
        ok = np.isfinite(c[part]).all(axis=0) & (np.abs(c[part]) < 1e3).all(axis=0)
        assert ok.sum() == pos.size - (6 if part[0] != part[-1] else 3)
        ref = c[part].astype(np.float64).sum(axis=0)
        bound = 1.001 * (len(part) * 2.0 ** -(bits + 1) + 2.0 ** -24 * np.abs(ref))
        err = np.abs(out[pos].astype(np.float64) - ref)
        print(f"{tag}: worst error / bound {float((err[ok] / bound[ok]).max()):.3f}")
        assert (err[ok] <= bound[ok]).all(), tag
        # the clamped coordinates entered at +-L, NaN at 0: the sum did not wrap
        L = secagg_limit(len(part))
        rest = np.rint(c[part][1:, 30].astype(np.float64) * 2.0 ** bits).sum()
        assert out[pos[30]] == np.float32(L + rest) * np.float32(2.0 ** -bits), tag
    # a state that is not live: the rank-order sum of the whole (clear: the mask step did not run) buffers,
    # padding included
    planted = a.copy()
    planted[part[0], :pimg][~real] = np.nan
    whole = _fold(planted)
    for state in (_state(0, 1), _state(1, ROUNDS_TAB), _state(1, -1)):
        src = [torch.as_tensor(row).to(DEV) for row in planted]
        dst = [torch.full((pimg + TAILS,), 7.0, device=DEV)]
        _open_launch(m, dims, 24, src, dst, state, rtab)
        got = dst[0].cpu().numpy()
        nan = np.isnan(whole)
        np.testing.assert_array_equal(np.isnan(got), nan)
        np.testing.assert_array_equal(got[~nan].view(np.uint32), whole[~nan].view(np.uint32), err_msg=f"K={K}: not live")


# ---- 4. groups ----
ROUNDS = 6
GROUP_EPS = 1e-4   # the clients' Adam eps of the groups held to the torch group (tests/test_server_opt.py)
SHAPES = {"small": (240, 17, 3, (24,)), "income": (1200, 14, 2, (50, 200))}
GROUP_CASES = {"plain": dict(), "3of5": dict(participation=0.6), "dp": dict(dp_clip=0.5, dp_noise=0.5, dp_seed=7),
               "server": dict(server_opt="adam", server_lr=1e-2)}


def _cfg(shape, **kw):
    base = dict(hidden=SHAPES[shape][3], max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, eps=GROUP_EPS,
                secagg=True, secagg_seed=SEED)
    return EngineConfig(**{**base, **kw})


def _data(shape):
    rows, F, C, _ = SHAPES[shape]
    return make_multiclass(rows, F, C, DATA_SEED)


def _group(backend, shape, k=5, rounds=ROUNDS, tamper=None, wire=None, **kw):
    X, y = _data(shape)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, _cfg(shape, **kw), backend=backend, shard_mode="iid", seed=2, tamper=tamper, wire=wire)
    g.run(rounds)
    return g


@functools.lru_cache(maxsize=None)
def _torch_reference(shape, case):
    g = _group("torch", shape, **GROUP_CASES[case])
    out = {"w": g.global_flat(), "glob": g.history()["global"].copy(), "loss": g.history()["loss"].copy()}
    for a in out.values():
        a.setflags(write=False)
    return out


def _assert_clients_agree(g):
    lead = g.clients[0]
    h = lead.history()
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), lead.global_flat())
        for key in ("global", "loss", "per_rank"):
            np.testing.assert_array_equal(c.history()[key], h[key])


@pytest.mark.parametrize("shape, case", [("small", "plain"), ("small", "3of5"), ("small", "dp"), ("small", "server"),
                                         ("income", "plain")])
def test_hip_group_against_the_torch_group(shape, case):
    g = _group("hip", shape, **GROUP_CASES[case])
    _assert_clients_agree(g)
    lead = g.clients[0]
    assert lead.layout["secagg"] == {"bits": 24, "stream": SECAGG_STREAM} and lead.aggregation == "host-gather"
    h = g.history()
    assert h["rounds_run"] == ROUNDS and h["secagg_clamped"].shape == (ROUNDS,) and not h["secagg_clamped"].any()
    ref = _torch_reference(shape, case)
    e = nerr(g.global_flat(), ref["w"])
    print(f"group {shape} {case}: HIP vs torch, max|err| / max|ref| = {e:.3g}")
    assert e < 2e-5, (shape, case, e)
    np.testing.assert_allclose(h["loss"], ref["loss"], rtol=1e-4)
    # the zero-padding invariant of the global image
    img = lead.params[g.rounds & 1][:lead.Pimg].cpu().numpy()
    assert not img[~_positions(tuple(lead.dims))[1]].view(np.uint32).any()


def test_hip_group_bf16_against_secagg_off():
    """bf16 at the bf16 engines' 5-round tolerance (tests/test_hip_engine.py BF16_DRIFT_TOL: relative L2
    5e-3), against the HIP group without secure aggregation."""
    on = _group("hip", "small", rounds=5, dtype="bf16")
    off = _group("hip", "small", rounds=5, dtype="bf16", secagg=False)
    _assert_clients_agree(on)
    assert "secagg" not in off.clients[0].layout and "secagg_clamped" not in off.history()
    w, wr = on.global_flat(), off.global_flat()
    d = float(np.linalg.norm(w - wr) / np.linalg.norm(wr))
    print(f"bf16 group, secagg on vs off, 5 rounds: relative L2 {d:.3g}")
    assert d < 5e-3


def test_wire_view_equals_the_host_model_and_the_seed_is_not_in_the_result():
    clear, wire = {}, {}
    g = _group("hip", "small", participation=0.6,
               tamper=lambda r, bufs: clear.setdefault(r, [b.cpu().numpy().copy() for b in bufs]),
               wire=lambda r, bufs: wire.setdefault(r, [b.cpu().numpy().copy() for b in bufs]))
    lead = g.clients[0]
    pos, real, pimg = _positions(tuple(lead.dims))
    part = [int(k) for k in lead.participants(0)]
    assert len(part) == 3
    for i in range(5):
        c, w = clear[0][i], wire[0][i]
        np.testing.assert_array_equal(c[pimg:].view(np.uint32), w[pimg:].view(np.uint32))    # tails stay clear
        if i in part:
            q, n = secagg_quantize(c[pos], 24, 3)
            np.testing.assert_array_equal(w.view(np.uint32)[pos], secagg_mask(q, i, part, 0, SEED))
            assert n == 0 and not w[:pimg][~real].view(np.uint32).any()
        else:
            np.testing.assert_array_equal(c.view(np.uint32), w.view(np.uint32))
    other = _group("hip", "small", participation=0.6, secagg_seed=SEED + 1)
    np.testing.assert_array_equal(other.global_flat(), g.global_flat())
    np.testing.assert_array_equal(other.history()["global"], g.history()["global"])


def test_rounds_past_an_early_stop_change_nothing():
    kw = dict(early_stop=True, patience=1, tolerance=0.5, max_rounds=16)
    a = _group("hip", "small", rounds=2, **kw)
    b = _group("hip", "small", rounds=8, **kw)
    assert a.history()["stop_round"] == b.history()["stop_round"] == 2 and b.history()["rounds_run"] == 2
    for ca, cb in zip(a.clients, b.clients):
        np.testing.assert_array_equal(ca.global_flat(), cb.global_flat())
    np.testing.assert_array_equal(a.history()["secagg_clamped"], b.history()["secagg_clamped"])


def test_clamp_counts_and_resume_continue_bit_for_bit():
    """Client 1 publishes NaN, +inf and -1e9 every round: counted on its own history, the sum stays finite.
    A group under ANOTHER mask seed that loads the clients' portable states after 3 rounds ends where the
    uninterrupted one does (the seed is config, never state), clamp history included."""
    def tamper(r, bufs):
        bufs[1][:3] = torch.tensor([float("nan"), float("inf"), -1e9], device=DEV)
    a = _group("hip", "small", k=3, rounds=3, tamper=tamper)
    assert [c.history()["secagg_clamped"].tolist() for c in a.clients] == [[0] * 3, [3] * 3, [0] * 3]
    assert np.isfinite(a.global_flat()).all()
    states = [c.portable_state() for c in a.clients]
    assert not any("seed" in k for k in states[0])
    b = _group("hip", "small", k=3, rounds=0, tamper=tamper, secagg_seed=SEED + 5)
    for c, st in zip(b.clients, states):
        c.load_portable_state(st)
    b.rounds = 3
    b.run(3)
    full = _group("hip", "small", k=3, rounds=6, tamper=tamper)
    for cb, cf in zip(b.clients, full.clients):
        np.testing.assert_array_equal(cb.global_flat(), cf.global_flat())
        for key in ("secagg_clamped", "global", "loss", "per_rank"):
            np.testing.assert_array_equal(cb.history()[key], cf.history()[key])
    assert full.clients[1].history()["secagg_clamped"].tolist() == [3] * 6


def test_refusals():
    X, y = _data("small")
    flat = init_flat(SMALL, 0)
    mk = lambda cfg, **kw: HipRoundEngine(X, y, 3, cfg, SimRank(3, 0, DEV), flat, n_total=3 * len(X),
                                          client_sizes=[len(X)] * 3, **kw)
    e = mk(_cfg("small"))
    assert e.aggregation == "host-gather" and not e.engine.lagged and e._peer is None and e._native_comm is None
    with pytest.raises(RuntimeError, match="issues its own FedAvg"):
        e.trace(1)
    with pytest.raises(RuntimeError, match="aggregated from Python"):
        e.prime_graph(4)
    with pytest.raises(ValueError, match="aggregator"):
        mk(_cfg("small", aggregator="median"))
    one = HipRoundEngine(X, y, 3, _cfg("small"), None, flat)
    assert one.aggregation == "none" and one.secagg == 0 and "secagg" not in one.layout
    from fedmi.ops import native
    m = native()
    t = torch.zeros(image_layout(SMALL)[2] + TAILS, device=DEV)
    tab, cl = _tab([t] * 65), _tab([torch.zeros(1, dtype=torch.int32, device=DEV)] * 65)
    args = (_state(1, 0).data_ptr(), _rtab(2, [0, 1]).data_ptr())
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="clients 0..63"):
        m.secagg_mask(SMALL, 24, SEED, tab.data_ptr(), 2, 63, *args, cl.data_ptr(), 1, s)
    with pytest.raises(RuntimeError, match="bits"):
        m.secagg_mask(SMALL, 31, SEED, tab.data_ptr(), 2, 0, *args, cl.data_ptr(), 1, s)
    with pytest.raises(RuntimeError, match="1..64 clients"):
        m.secagg_open(SMALL, 24, tab.data_ptr(), 65, tab.data_ptr(), 1, *args, TAILS, 1, s)


# ---- 5. three ranks sharing one GPU ----
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
        # secagg_seed=None: every rank takes rank 0's draw over the control plane
        e = HipRoundEngine(X[idx[rank]], y[idx[rank]], 3, _cfg("small", secagg_seed=None), comm,
                           init_flat(SMALL, 2 * 1000003 + rank), n_total=sum(len(i) for i in idx))
        agg, seed = e.aggregation, e.secagg_seed
        e.run(ROUNDS)
        h = e.history()
        torch.cuda.synchronize()
        comm.Barrier()
        q.put((rank, (agg, seed, e.global_flat(), h["global"], h["loss"], h["per_rank"], h["rounds_run"]), None))
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
    g = _group("hip", "small", k=3)
    h = g.history()
    ref = (g.global_flat(), h["global"], h["loss"], h["per_rank"], h["rounds_run"])
    assert len({res[1] for _, res, _ in out}) == 1            # one seed for the job
    for rank, res, _ in out:
        assert res[0] == "host-gather"
        for a, b in zip(res[2:], ref):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank}")

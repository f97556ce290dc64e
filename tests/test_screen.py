"""Multi-Krum screening on the GPU: the fl_screen kernels and the aggregate launch behind them on
synthetic buffers (bitwise against the host models of fedmi/fl/aggregate.py), one captured graph of
the three launches replayed over rounds, client groups with colluding tamperers against the torch
group, and three ranks gathering over the host plane.

The kernels are held to their models bit for bit, so no tolerance enters the kernel tests; the accuracy
of the model itself (its chain bound against float64) is tests/test_screen_cpu.py's.  Groups: the
planted tamperers are far away, so the kept sets must be equal; the weights are held to the project's
2e-5 (``nerr``) of the torch group.  bf16 groups: tests/test_robust.py holds its bf16 groups to no numeric
tolerance against fp32 (finite, clients agree, bitwise invariant to the cut client), and so does the
bf16 case here, which adds that the kept sets equal its own fp32 run's.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.aggregate import mask_bits, pair_distances_model, robust_aggregate_torch, screen_select
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass, nerr

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL, INCOME = [17, 24, 3], [14, 50, 200, 2]
TAILS = 7
RULES = {"mean": (2, 0.0), "median": (1, 0.0), "trimmed_mean": (2, 0.2)}   # (kernel kind, beta) a screening engine runs
SENTINEL = 0x5A5A5A5A5A5A5A5A


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
    return [np.ones(K, bool), pick(max(1, (3 * K + 3) // 4)), pick(1), pick(min(2, K))]


def _rtab(masks):
    t = np.zeros((len(masks), 4), np.uint32)
    for r, m in enumerate(masks):
        bits = mask_bits(m)
        t[r, 0] = np.float32(1.0).view(np.uint32)
        t[r, 1] = np.float32(m.sum()).view(np.uint32)
        t[r, 2], t[r, 3] = bits & 0xFFFFFFFF, bits >> 32
    return torch.as_tensor(t.reshape(-1).view(np.int32)).to(DEV)


def _inputs(dims, K, seed):
    """[K, Pimg + TAILS]: honest clients ``base + 0.1 noise``, a NaN client (K >= 3), a +inf and a -inf client
    (K >= 5), a 1e30 client whose squares overflow and an exact duplicate (K >= 8), NaN in the image
    padding of client 0 and 1e30 in client 1's."""
    pimg = image_layout(dims)[2]
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(pimg + TAILS) + 0.1 * rng.standard_normal((K, pimg + TAILS))).astype(np.float32)
    if K >= 3:
        a[K // 2, :pimg] = np.nan
    if K >= 5:
        a[1, :pimg], a[K - 1, :pimg] = np.inf, -np.inf
    if K >= 8:
        a[3, :pimg] = 1e30
        a[6, :pimg] = a[2, :pimg]
    real = dense_to_image(np.ones(param_count(dims), np.float32), dims) != 0
    a[0, :pimg][~real] = np.nan
    a[min(1, K - 1), :pimg][~real] = 1e30
    return a, real, pimg


def _tab(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


def _fold(a):
    acc = torch.as_tensor(a[0]).clone()
    for row in a[1:]:
        acc += torch.as_tensor(row)
    return acc.numpy()


class _Screen:
    """The three launches over K device buffers with caller-owned scratch, as _AggLaunch issues them."""

    def __init__(self, dims, src, rtab, rounds):
        from fedmi.ops import native
        self.m, self.dims, self.src, self.K = native(), dims, src, len(src)
        self.rtab, self.rounds = rtab, rounds
        self.tab = _tab(src)
        self.dist = torch.full((self.K * self.K,), -7.0, device=DEV)
        self.keep = torch.full((1,), SENTINEL, dtype=torch.int64, device=DEV)
        self.hist = torch.full((rounds,), SENTINEL, dtype=torch.int64, device=DEV)

    def run_dist(self, state, stream=None, tile=0):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self.m.screen_dist(self.dims, self.tab.data_ptr(), self.K, self.dist.data_ptr(), state.data_ptr(),
                           self.rtab.data_ptr(), self.rounds, s, tile)
        if stream is None:
            torch.cuda.synchronize()

    def run_select(self, state, f, m, stream=None):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self.m.screen_select(self.dist.data_ptr(), self.K, f, m or 0, self.keep.data_ptr(), self.hist.data_ptr(),
                             state.data_ptr(), self.rtab.data_ptr(), self.rounds, s)
        if stream is None:
            torch.cuda.synchronize()

    def run_robust(self, state, agg, dst, stream=None, keep=True, dt=None):
        """``dt``: the destinations' pointer table when the caller built it (a capture copies nothing)."""
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        dt = _tab(dst) if dt is None else dt
        kind, beta = RULES[agg]
        self.m.robust_aggregate(self.dims, kind, beta, self.tab.data_ptr(), self.K, dt.data_ptr(), len(dst),
                                state.data_ptr(), self.rtab.data_ptr(), TAILS, self.rounds, s,
                                self.keep.data_ptr() if keep else 0)
        if stream is None:
            torch.cuda.synchronize()
        return dt

    def matrix(self):
        return self.dist.cpu().numpy().reshape(self.K, self.K)

    def kept(self):
        return int(self.keep.cpu().numpy().view(np.uint64)[0])


def _fs(K):
    """(f, m) cases of a K-client launch: the largest f the full mask allows, Krum, and f = 0 keeping 2."""
    fmax = max(0, (K - 3) // 2)
    return [(fmax, None), (fmax, 1), (0, 2)]


def _check_kernels(dims, K, seed, rounds_checked=(0, 1, 2, 3)):
    a, real, pimg = _inputs(dims, K, seed)
    masks = _masks(K, seed)
    rtab = _rtab(masks)
    tails = _fold(a[:, pimg:])
    screened = 0
    for r in rounds_checked:
        mask = masks[r]
        tag = f"K={K} mask={np.flatnonzero(mask).tolist()}"
        src = [torch.as_tensor(row).to(DEV) for row in a]
        sc = _Screen(dims, src, rtab, len(masks))
        st = _state(1, r)
        sc.run_dist(st)
        d = sc.matrix()
        act = np.outer(mask, mask)
        model = pair_distances_model(a[:, :pimg], mask, real)
        np.testing.assert_array_equal(d[act].view(np.int32), model[act].view(np.int32), err_msg=tag + ": matrix")
        sub = d[np.ix_(mask, mask)]
        np.testing.assert_array_equal(sub.view(np.int32), sub.T.view(np.int32), err_msg=tag + ": symmetry")
        assert (np.diag(sub).view(np.int32) == 0).all() and not np.isnan(sub).any() and (sub >= 0).all(), tag
        assert sc.kept() == SENTINEL and (sc.hist.cpu().numpy() == SENTINEL).all(), tag   # dist writes the matrix alone
        for s, row in zip(src, a):
            _same_bits(s.cpu().numpy(), row, tag + ": a source changed")
        for f, m in _fs(K):
            sc.run_select(st, f, m)
            want = screen_select(d, mask, f, m)
            kept = sc.kept()
            assert kept == mask_bits(want), (tag, f, m, bin(kept), want)
            hist = sc.hist.cpu().numpy().view(np.uint64)
            assert int(hist[r]) == kept and all(int(h) == SENTINEL for q, h in enumerate(hist) if q != r), tag
            assert kept & ~mask_bits(mask) == 0
            screened += int(kept != mask_bits(mask))
            for agg in RULES:
                dst = [torch.full((pimg + TAILS,), 7.0, device=DEV) for _ in range(2)]
                sc.run_robust(st, agg, dst)
                out = dst[0].cpu().numpy()
                t2 = f"{tag} f={f} m={m} {agg}"
                _same_bits(dst[1].cpu().numpy(), out, t2 + ": destinations differ")
                assert (out[:pimg][~real].view(np.int32) == 0).all(), t2     # padding exact 0
                _same_bits(out[pimg:], tails, t2 + ": tails")                # the left fold over all K sources
                kind = "trimmed_mean" if agg == "mean" else agg
                ref = robust_aggregate_torch(torch.as_tensor(a[:, :pimg]), want, kind, RULES[agg][1]).numpy()
                _same_bits(out[:pimg][real], ref[real], t2 + ": image")
                if sum(want) == 1:
                    _same_bits(out[:pimg][real], a[want.index(True), :pimg][real], t2 + ": Krum returns the kept model")
        if r == 1:
            # in place, every rule: every source is a destination (the kept mask of the last select above:
            # f = 0, m = 2), on fresh copies of the sources each time
            want = screen_select(d, mask, 0, 2)
            for agg in RULES:
                kind = "trimmed_mean" if agg == "mean" else agg
                ref = robust_aggregate_torch(torch.as_tensor(a[:, :pimg]), want, kind, RULES[agg][1]).numpy()
                src2 = [torch.as_tensor(row).to(DEV) for row in a]
                sc2 = _Screen(dims, src2, rtab, len(masks))
                sc2.keep.copy_(sc.keep)
                sc2.run_robust(st, agg, src2)
                for s in src2:
                    out = s.cpu().numpy()
                    _same_bits(out[:pimg][real], ref[real], f"{tag} {agg}: in place")
                    assert (out[:pimg][~real].view(np.int32) == 0).all()
                    _same_bits(out[pimg:], tails, f"{tag} {agg}: in place tails")
    # a state that is not live: dist, keep and hist untouched, the aggregate the fold of the whole buffers
    whole = _fold(a)
    for state in (_state(0, 0), _state(1, len(masks)), _state(1, -1)):
        src = [torch.as_tensor(row).to(DEV) for row in a]
        sc = _Screen(dims, src, rtab, len(masks))
        sc.run_dist(state)
        sc.run_select(state, 0, 1)
        assert (sc.matrix() == -7.0).all() and sc.kept() == SENTINEL and (sc.hist.cpu().numpy() == SENTINEL).all()
        dst = [torch.full((pimg + TAILS,), 7.0, device=DEV)]
        sc.run_robust(state, "median", dst)
        _same_bits(dst[0].cpu().numpy(), whole, f"K={K}: not live")
    return screened


@pytest.mark.parametrize("K", [2, 3, 5, 8, 9, 17, 33, 64])
def test_kernels_small_image(K):
    screened = _check_kernels(SMALL, K, 300 + K)
    assert screened > 0 or K < 3     # some launch cut the sampled set


@pytest.mark.parametrize("K", [5, 17])
def test_kernels_income_image(K):
    pimg = image_layout(INCOME)[2]
    assert (pimg // 4) % 256 != 0     # the last trip of the distance loop is partial
    _check_kernels(INCOME, K, 20 + K, rounds_checked=(0, 1))


@pytest.mark.parametrize("dims", [SMALL, INCOME], ids=["small", "income"])
def test_pair_of_64_equals_a_launch_of_2_and_every_tile(dims):
    K = 64
    a, real, pimg = _inputs(dims, K, 9)
    rtab = _rtab([np.ones(K, bool)])
    src = [torch.as_tensor(row).to(DEV) for row in a]
    sc = _Screen(dims, src, rtab, 1)
    st = _state(1, 0)
    sc.run_dist(st)
    d = sc.matrix().copy()
    _same_bits(d, pair_distances_model(a[:, :pimg], np.ones(K, bool), real), "K=64 matrix")
    for tile in (1, 2, 4):
        sc.dist.fill_(-7.0)
        sc.run_dist(st, tile=tile)
        np.testing.assert_array_equal(sc.matrix().view(np.int32), d.view(np.int32), err_msg=f"tile {tile}")
    rtab2 = _rtab([np.ones(2, bool)])
    for i, j in ((0, 63), (5, 37), (62, 63), (2, 6), (1, 33), (3, 40), (17, 16)):
        two = _Screen(dims, [src[i], src[j]], rtab2, 1)
        two.run_dist(st)
        m2 = two.matrix()
        assert m2[0, 1].view(np.int32) == m2[1, 0].view(np.int32) == d[i, j].view(np.int32), (i, j, m2, d[i, j])
        assert m2[0, 0] == 0 and m2[1, 1] == 0


def test_entry_points_refuse_bad_arguments():
    from fedmi.ops import native
    m = native()
    pimg = image_layout(SMALL)[2]
    t = torch.zeros(pimg + TAILS, device=DEV)
    tab, st, rt = _tab([t] * 65), _state(1, 0), _rtab([np.ones(64, bool)])
    sc = torch.zeros(65 * 65, device=DEV)
    w = torch.zeros(4, dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="1..64 clients"):
        m.screen_dist(SMALL, tab.data_ptr(), 65, sc.data_ptr(), st.data_ptr(), rt.data_ptr(), 1, s)
    with pytest.raises(RuntimeError, match="1..64 clients"):
        m.screen_select(sc.data_ptr(), 65, 0, 0, w.data_ptr(), w.data_ptr(), st.data_ptr(), rt.data_ptr(), 1, s)
    with pytest.raises(RuntimeError, match="tile"):
        m.screen_dist(SMALL, tab.data_ptr(), 4, sc.data_ptr(), st.data_ptr(), rt.data_ptr(), 1, s, 3)
    with pytest.raises(RuntimeError, match="f and m"):
        m.screen_select(sc.data_ptr(), 4, -1, 0, w.data_ptr(), w.data_ptr(), st.data_ptr(), rt.data_ptr(), 1, s)
    with pytest.raises(RuntimeError, match="bad arguments"):
        m.screen_select(sc.data_ptr(), 4, 0, 0, 0, w.data_ptr(), st.data_ptr(), rt.data_ptr(), 1, s)


def test_captured_graph_of_the_three_launches_replays_over_rounds():
    K, f, m = 9, 2, None
    a, real, pimg = _inputs(SMALL, K, 77)
    masks = [np.ones(K, bool), np.arange(K) != 4, np.arange(K) % 4 != 1, np.arange(K) < 7]
    rtab = _rtab(masks)
    src = [torch.as_tensor(row).to(DEV) for row in a]
    # eager results round by round
    eager = []
    for r, mask in enumerate(masks):
        sc = _Screen(SMALL, src, rtab, len(masks))
        st = _state(1, r)
        sc.run_dist(st)
        sc.run_select(st, f, m)
        dst = [torch.zeros(pimg + TAILS, device=DEV)]
        sc.run_robust(st, "mean", dst)
        eager.append((sc.kept(), dst[0].cpu().numpy()))
        assert sc.kept() == mask_bits(screen_select(sc.matrix(), mask, f, m))
    assert len({k for k, _ in eager}) == len(masks)          # four different kept sets
    # one graph; the round comes from the state the launches read
    sc = _Screen(SMALL, src, rtab, len(masks))
    state = _state(1, 0)
    dst = [torch.zeros(pimg + TAILS, device=DEV)]
    dt = _tab(dst)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        s = torch.cuda.current_stream().cuda_stream
        sc.run_dist(state, stream=s)
        sc.run_select(state, f, m, stream=s)
        sc.run_robust(state, "mean", dst, stream=s, dt=dt)
    torch.cuda.synchronize()
    for r in range(len(masks)):
        state.copy_(_state(1, r))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert sc.kept() == eager[r][0], r
        _same_bits(dst[0].cpu().numpy(), eager[r][1], f"replay of round {r}")
    hist = sc.hist.cpu().numpy().view(np.uint64)
    assert [int(h) for h in hist] == [k for k, _ in eager]
    del dt


# ---- groups ----
ROUNDS = 6
GROUP_EPS = 1e-4   # the clients' Adam eps of the groups held to the torch group (tests/test_robust.py)
SHAPES = {"small": (240, 17, 3, (24,)), "income": (1200, 14, 2, (50, 200))}
BAD = (2, 5)


def _dims(shape):
    return [SHAPES[shape][1], *SHAPES[shape][3], SHAPES[shape][2]]


def _cfg(shape, **kw):
    base = dict(hidden=SHAPES[shape][3], max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, eps=GROUP_EPS,
                screen="multi_krum", screen_byzantine=2)
    return EngineConfig(**{**base, **kw})


def _data(shape):
    rows, F, C, _ = SHAPES[shape]
    return make_multiclass(rows, F, C, DATA_SEED)


def _collude(shape, backend, value):
    """The tamperers all publish client 0's model + 50 (``value`` None), or ``value`` everywhere -- on the
    image (hip: padding included) or the dense parameters (torch), never the tails."""
    n = image_layout(_dims(shape))[2] if backend == "hip" else param_count(_dims(shape))

    def tamper(r, bufs):
        for k in BAD:
            bufs[k][:n] = bufs[0][:n] + 50.0 if value is None else value
    return tamper


def _group(backend, shape, value=None, k=7, **kw):
    X, y = _data(shape)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, _cfg(shape, **kw), backend=backend, shard_mode="iid", seed=2,
                    tamper=_collude(shape, backend, value) if k > max(BAD) else None)
    g.run(ROUNDS)
    return g


def _assert_clients_agree(g):
    lead = g.clients[0]
    h = lead.history()
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), lead.global_flat())
        for key in ("global", "loss", "per_rank", "screen_kept"):
            np.testing.assert_array_equal(c.history()[key], h[key])


def _kept_clients(h):
    return [[k for k in range(64) if (int(w) >> k) & 1] for w in h["screen_kept"]]


@pytest.mark.parametrize("agg", ["mean", "median"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_hip_group_against_the_torch_group(shape, agg):
    hip = _group("hip", shape, aggregator=agg)
    ref = _group("torch", shape, aggregator=agg)
    h, ht = hip.history(), ref.history()
    assert h["rounds_run"] == ROUNDS and h["screen_kept"].dtype == np.uint64
    np.testing.assert_array_equal(h["screen_kept"], ht["screen_kept"])
    for kept in _kept_clients(h):
        assert len(kept) == 5 and not set(kept) & set(BAD), kept
    lead = hip.clients[0]
    assert lead.layout["aggregator"] == agg and lead.layout["screen"] == "multi_krum" and lead.agg_scale == 1.0
    w = hip.global_flat()
    err = nerr(w, ref.global_flat())
    print(f"group {shape} {agg}: HIP vs torch {err:.3g}")
    assert np.isfinite(w).all() and err < 2e-5, err
    np.testing.assert_allclose(h["loss"], ht["loss"], rtol=1e-4)
    _assert_clients_agree(hip)
    # what the rejected clients send is never read into the result
    nan = _group("hip", shape, value=float("nan"), aggregator=agg)
    np.testing.assert_array_equal(nan.global_flat(), w)
    np.testing.assert_array_equal(nan.history()["screen_kept"], h["screen_kept"])
    np.testing.assert_array_equal(nan.history()["global"], h["global"])
    # the zero-padding invariant survived tamperers that wrote 50 / NaN into the padding
    img = nan.clients[0].params[nan.rounds & 1][:lead.Pimg].cpu().numpy()
    real = dense_to_image(np.ones(lead.P, np.float32), lead.dims) != 0
    assert (img[~real].view(np.int32) == 0).all()


def test_hip_group_composes_with_a_server_optimizer():
    kw = dict(server_opt="adam", server_lr=1e-2)
    hip, ref = _group("hip", "small", **kw), _group("torch", "small", **kw)
    np.testing.assert_array_equal(hip.history()["screen_kept"], ref.history()["screen_kept"])
    for kept in _kept_clients(hip.history()):
        assert not set(kept) & set(BAD)
    _assert_clients_agree(hip)
    w = hip.global_flat()
    assert np.isfinite(w).all() and np.abs(hip.clients[0].server_m.cpu().numpy()).max() > 0
    err = nerr(w, ref.global_flat())
    print(f"group small mean + server adam: HIP vs torch {err:.3g}")
    assert err < 2e-5, err
    np.testing.assert_allclose(hip.history()["loss"], ref.history()["loss"], rtol=1e-4)
    nan = _group("hip", "small", value=float("nan"), **kw)
    np.testing.assert_array_equal(nan.global_flat(), w)


def test_hip_group_bf16():
    a = _group("hip", "small", dtype="bf16")
    b = _group("hip", "small", value=float("nan"), dtype="bf16")
    fp32 = _group("hip", "small")
    wa = a.global_flat()
    assert np.isfinite(wa).all()
    np.testing.assert_array_equal(wa, b.global_flat())
    np.testing.assert_array_equal(a.history()["screen_kept"], b.history()["screen_kept"])
    np.testing.assert_array_equal(a.history()["screen_kept"], fp32.history()["screen_kept"])
    _assert_clients_agree(a)


# ---- three ranks sharing one GPU ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


RANK_KW = dict(screen_byzantine=0, screen_keep=2)


def _rank_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    try:
        from fedmi.data.sharding import shard_indices
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="xgmi", device="cuda:0", rccl=False)
        X, y = _data("small")
        idx = [shard_indices(len(X), r, world, mode="iid", seed=2, labels=y, alpha=0.5) for r in range(world)]
        e = HipRoundEngine(X[idx[rank]], y[idx[rank]], 3, _cfg("small", **RANK_KW), comm,
                           init_flat(SMALL, 2 * 1000003 + rank), n_total=sum(len(i) for i in idx))
        agg, lay = e.aggregation, (e.layout["aggregator"], e.layout["screen"])
        e.run(ROUNDS)
        h = e.history()
        torch.cuda.synchronize()
        comm.Barrier()
        q.put((rank, (agg, lay, e.global_flat(), h["global"], h["loss"], h["per_rank"], h["screen_kept"], h["rounds_run"]),
               None))
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
    g = _group("hip", "small", k=3, **RANK_KW)
    h = g.history()
    assert all(bin(int(w)).count("1") == 2 for w in h["screen_kept"])
    ref = (g.global_flat(), h["global"], h["loss"], h["per_rank"], h["screen_kept"], h["rounds_run"])
    for rank, res, _ in out:
        assert res[0] == "host-gather" and res[1] == ("mean", "multi_krum")
        for a, b in zip(res[2:], ref):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank}")

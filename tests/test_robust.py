"""Robust aggregation on the GPU: the fl_robust kernel alone on synthetic buffers, client groups
with a Byzantine client against the torch group and a float64 group oracle, three ranks gathering
over the host plane, and the refusals.

Kernel bound.  With n kept values the kernel computes n - 1 additions (the first, 0 + v, is exact) and
one division, each rounded once: |result - exact| <= ((n - 1) u sum|kept| + u |result|) (1 + O(u)),
u = 2^-24; asserted as 1.001 x that against the float64 numpy oracle (sort, slice, mean), and the
bound itself must stay under 1e-5 of the magnitude summed (n <= 64: 63 u = 3.8e-6), so it is not
vacuous.
"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.aggregate import robust_aggregate_torch, trim_count
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .reference_oracle import DATA_SEED, Float64RoundOracle, make_multiclass, nerr
from .server_oracle import server_step_f64

pytestmark = pytest.mark.gpu

DEV = "cuda"
KIND = {"median": 1, "trimmed_mean": 2}
SMALL, INCOME = [17, 24, 3], [14, 50, 200, 2]
TAILS = 7
U = 2.0 ** -24


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


def _inputs(dims, K, seed):
    """[K, Pimg + TAILS] normals with planted ties, +-0, one NaN client (K >= 3: below that nothing
    can be cut), one +inf and one -inf client (K >= 5), and NaN in the image padding of client 0."""
    pimg = image_layout(dims)[2]
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((K, pimg + TAILS)).astype(np.float32)
    a[:, 100:160] = np.round(a[:, 100:160])
    a[:, 160:200] = a[0, 160:200]
    a[:, 200:240] = 0.0
    a[::2, 200:240] = -0.0
    if K >= 3:
        a[K // 2, :pimg] = np.nan
    if K >= 5:
        a[1, :pimg], a[K - 1, :pimg] = np.inf, -np.inf
    real = dense_to_image(np.ones(param_count(dims), np.float32), dims) != 0
    a[0, :pimg][~real] = np.nan
    return a, real, pimg


def _tab(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


def _launch(m, dims, kind, beta, src, dst, state, rtab, rounds):
    st, dt = _tab(src), _tab(dst)
    m.robust_aggregate(dims, KIND[kind], beta, st.data_ptr(), len(src), dt.data_ptr(), len(dst), state.data_ptr(),
                       rtab.data_ptr(), TAILS, rounds, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _fold(a):
    acc = torch.as_tensor(a[0]).clone()
    for row in a[1:]:
        acc += torch.as_tensor(row)
    return acc.numpy()


def _check_kernel(dims, K, seed):
    from fedmi.ops import native
    m = native()
    a, real, pimg = _inputs(dims, K, seed)
    masks = _masks(K, seed)
    rtab = _rtab(masks)
    tails = _fold(a[:, pimg:])
    checked = 0
    for kind, beta in (("median", 0.0), ("trimmed_mean", 0.2), ("trimmed_mean", 0.0)):
        for r, mask in enumerate(masks):
            src = [torch.as_tensor(row).to(DEV) for row in a]
            dst = [torch.full((pimg + TAILS,), 7.0, device=DEV) for _ in range(2)]
            _launch(m, dims, kind, beta, src, dst, _state(1, r), rtab, len(masks))
            out = dst[0].cpu().numpy()
            tag = f"K={K} {kind} beta={beta} mask={np.flatnonzero(mask).tolist()}"
            for s, row in zip(src, a):
                _same_bits(s.cpu().numpy(), row, tag + ": a source changed")
            _same_bits(dst[1].cpu().numpy(), out, tag + ": destinations differ")
            # padding exact zero although client 0's padding is NaN; tails the rank-order fold
            assert (out[:pimg][~real].view(np.int32) == 0).all(), tag
            _same_bits(out[pimg:], tails, tag + ": tails")
            # bitwise the fp32 torch model of the rule
            model = robust_aggregate_torch(torch.as_tensor(a[:, :pimg]), mask, kind, beta).numpy()
            _same_bits(out[:pimg][real], model[real], tag + ": image")
            # float64 oracle
            kr = int(mask.sum())
            t = trim_count(kind, beta, kr)
            kept = np.sort(a[:, :pimg][mask][:, real].astype(np.float64), axis=0)[t:kr - t]
            with np.errstate(invalid="ignore"):   # (inf - inf where both infinite clients are kept)
                ref, sabs, n = kept.mean(axis=0), np.abs(kept).sum(axis=0), kr - 2 * t
            fin = np.isfinite(ref)
            if t >= 2 or (t >= 1 and K < 5) or K < 3:
                assert fin.all(), tag     # the NaN and the +-inf clients are all cut
            if fin.any():                 # (K_r = 1 may have picked the NaN client alone)
                bound = 1.001 * ((n - 1) * U * sabs[fin] + U * np.abs(ref[fin]))
                err = np.abs(out[:pimg][real][fin].astype(np.float64) - ref[fin])
                assert (err <= bound).all(), (tag, float((err - bound).max()))
                assert bound.max() <= 1e-5 * sabs[fin].max(), tag           # not vacuous
                checked += int(fin.sum())
            np.testing.assert_array_equal(out[:pimg][real][~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
            np.testing.assert_array_equal(np.isnan(out[:pimg][real]), np.isnan(ref))
            # a second launch on the same inputs: the same bits
            again = [torch.full((pimg + TAILS,), -3.0, device=DEV)]
            _launch(m, dims, kind, beta, src, again, _state(1, r), rtab, len(masks))
            _same_bits(again[0].cpu().numpy(), out, tag + ": replay")
            if r == 1:
                # in place: every source is a destination
                _launch(m, dims, kind, beta, src, src, _state(1, r), rtab, len(masks))
                for s in src:
                    _same_bits(s.cpu().numpy(), out, tag + ": in place")
    assert checked > pimg // 2, checked   # the oracle bound was asserted on finite results
    # a state that is not live (stopped, or a round past max_rounds): the rank-order sum of the whole
    # buffer, padding included
    whole = _fold(a)
    for state, rounds in ((_state(0, 0), len(masks)), (_state(1, len(masks)), len(masks)), (_state(1, -1), len(masks))):
        src = [torch.as_tensor(row).to(DEV) for row in a]
        dst = [torch.full((pimg + TAILS,), 7.0, device=DEV)]
        _launch(m, dims, "median", 0.0, src, dst, state, rtab, rounds)
        _same_bits(dst[0].cpu().numpy(), whole, f"K={K}: not live")


@pytest.mark.parametrize("K", [2, 3, 4, 5, 8, 9, 16, 17, 33, 64])
def test_kernel_small_image(K):
    _check_kernel(SMALL, K, 100 + K)


@pytest.mark.parametrize("K", [5, 17])
def test_kernel_income_image_partial_last_workgroup(K):
    pimg = image_layout(INCOME)[2]
    assert (pimg // 4) % 64 != 0 and pimg % 64 != 0 and TAILS % 64 != 0
    _check_kernel(INCOME, K, 7 + K)


# ---- groups ----
ROUNDS = 6
GROUP_EPS = 1e-4   # the clients' Adam eps of the groups held to the torch group (tests/test_server_opt.py)
SHAPES = {"small": (240, 17, 3, (24,)), "income": (1200, 14, 2, (50, 200))}
BETA = 0.2


def _cfg(shape, agg, **kw):
    base = dict(hidden=SHAPES[shape][3], max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, aggregator=agg,
                trim_ratio=BETA, eps=GROUP_EPS)
    return EngineConfig(**{**base, **kw})


def _data(shape):
    rows, F, C, _ = SHAPES[shape]
    return make_multiclass(rows, F, C, DATA_SEED)


def _group(backend, shape, agg, tamper=None, k=5, rounds=ROUNDS, **kw):
    X, y = _data(shape)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, _cfg(shape, agg, **kw), backend=backend, shard_mode="iid", seed=2, tamper=tamper)
    g.run(rounds)
    return g


def _dims(shape):
    return [SHAPES[shape][1], *SHAPES[shape][3], SHAPES[shape][2]]


def _poison(value, shape="small"):
    def tamper(r, bufs):
        bufs[2][:image_layout(_dims(shape))[2]] = value   # client 2's image, padding included; not the tails
    return tamper


class Float64RobustGroupOracle:
    """The arithmetic of ClientGroup(backend="torch") with a robust aggregator, in float64: every
    client starts round 0 from its own model and later rounds from the global one; the sampled
    clients train; their models are aggregated by ``robust_aggregate_torch`` in float64; an optional
    server step follows."""

    def __init__(self, shards, n_classes, cfg, flats, participants):
        self.cfg, self.participants = cfg, participants
        self.clients = [Float64RoundOracle(X, y, n_classes, cfg, f) for (X, y), f in zip(shards, flats)]
        self.x = None
        P = self.clients[0].weights().size
        self.sm = np.zeros(P)
        self.sv = None if cfg.server_opt in ("none", "sgd") else np.full(P, float(cfg.server_tau) ** 2)
        self.rounds = 0

    @staticmethod
    def _set(o, flat):
        off = 0
        with torch.no_grad():
            for p in o.params:
                p.copy_(torch.as_tensor(flat[off:off + p.numel()]).view_as(p))
                off += p.numel()

    def run(self, n):
        import warnings
        for _ in range(n):
            part = [int(k) for k in self.participants(self.rounds)]
            x = self.x if self.x is not None else self.clients[0].weights().copy()
            for k, o in enumerate(self.clients):
                if self.x is not None:
                    self._set(o, self.x)
                if k in part:
                    o.run(1)
                else:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore", UserWarning)
                        o.scheduler.step()
            stack = torch.as_tensor(np.stack([o.weights() for o in self.clients]))
            a = robust_aggregate_torch(stack, [k in part for k in range(len(self.clients))], self.cfg.aggregator,
                                       float(self.cfg.trim_ratio)).numpy()
            if self.cfg.server_opt != "none":
                a, self.sm, self.sv = server_step_f64(x, a, self.sm, self.sv, self.cfg)
            self.x = a
            self.rounds += 1


@functools.lru_cache(maxsize=None)
def _references(shape, agg, participation, server):
    kw = dict(participation=participation, **(dict(server_opt="adam", server_lr=1e-2) if server else {}))
    g = _group("torch", shape, agg, **kw)
    lead = g.clients[0]
    flats = [init_flat(_dims(shape), 2 * 1000003 + (0 if server else r)) for r in range(5)]
    o = Float64RobustGroupOracle([(c.X.numpy(), c.y.numpy()) for c in g.clients], SHAPES[shape][2], lead.cfg, flats,
                                 lead.participants)
    o.run(ROUNDS)
    out = {"t_w": g.global_flat(), "t_glob": g.history()["global"].copy(), "t_loss": g.history()["loss"].copy(), "o_w": o.x}
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
        assert (hc["rounds_run"], hc["stop_round"], hc["stop_trigger"]) == (h["rounds_run"], h["stop_round"], h["stop_trigger"])


def _assert_weights_rule(tag, w, ref):
    """fp32 weights within the project's 2e-5 of the torch group; where the torch group is itself
    further than that from the float64 group oracle, within 4x its error of the oracle."""
    cond, et, eo = nerr(ref["t_w"], ref["o_w"]), nerr(w, ref["t_w"]), nerr(w, ref["o_w"])
    print(f"{tag}: torch vs float64 {cond:.3g}  HIP vs torch {et:.3g}  HIP vs float64 {eo:.3g}  ratio {eo / cond:.2f}")
    if cond <= 2e-5:
        assert et < 2e-5, (tag, et)
    else:
        assert eo <= 4 * cond, (tag, eo, cond)


@pytest.mark.parametrize("agg", ["median", "trimmed_mean"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_hip_group_with_a_byzantine_client(shape, dtype, agg):
    a = _group("hip", shape, agg, _poison(float("nan"), shape), dtype=dtype)
    b = _group("hip", shape, agg, _poison(float("inf"), shape), dtype=dtype)
    wa = a.global_flat()
    assert np.isfinite(wa).all()
    np.testing.assert_array_equal(wa, b.global_flat())       # NaN and +inf are trimmed alike at the top
    np.testing.assert_array_equal(a.history()["global"], b.history()["global"])
    _assert_clients_agree(a)
    # the zero-padding invariant survived a client whose whole image (padding included) was NaN
    lead = a.clients[0]
    img = lead.params[a.rounds & 1][:lead.Pimg].cpu().numpy()
    real = dense_to_image(np.ones(lead.P, np.float32), lead.dims) != 0
    assert (img[~real].view(np.int32) == 0).all()
    clean = _group("hip", shape, agg, dtype=dtype)
    _assert_clients_agree(clean)
    assert clean.history()["rounds_run"] == ROUNDS
    assert np.abs(clean.global_flat() - wa).max() > 0
    if dtype == "fp32":
        ref = _references(shape, agg, 1.0, False)
        _assert_weights_rule(f"group {shape} {agg}", clean.global_flat(), ref)
        np.testing.assert_allclose(clean.history()["loss"], ref["t_loss"], rtol=1e-4)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_hip_group_mean_is_poisoned_by_the_same_client(dtype):
    g = _group("hip", "small", "mean", _poison(float("nan")), dtype=dtype)
    assert not np.isfinite(g.global_flat()).any()


@pytest.mark.parametrize("case", ["participation", "server"])
def test_hip_group_participation_and_server_optimizer(case):
    kw = dict(participation=0.6) if case == "participation" else dict(server_opt="adam", server_lr=1e-2)
    g = _group("hip", "small", "median", **kw)
    _assert_clients_agree(g)
    ref = _references("small", "median", kw.get("participation", 1.0), case == "server")
    _assert_weights_rule(f"group small median {case}", g.global_flat(), ref)
    np.testing.assert_allclose(g.history()["loss"], ref["t_loss"], rtol=1e-4)
    if case == "participation":
        # 3 of 5 sampled: the NaN client is cut whenever it is sampled (t = 1), ignored when it is not
        lead = g.clients[0]
        assert any(2 in lead.participants(r) for r in range(ROUNDS)) and any(2 not in lead.participants(r) for r in range(ROUNDS))
        p = _group("hip", "small", "median", _poison(float("nan")), **kw)
        assert np.isfinite(p.global_flat()).all()
        _assert_clients_agree(p)
    else:
        assert np.abs(g.clients[0].server_m.cpu().numpy()).max() > 0


def test_rounds_past_an_early_stop_change_nothing():
    """Patience 1 with a loose tolerance stops after round 1: six more rounds leave the global image
    of a group that issued exactly two rounds (the kernel's rank-order fold republishes it)."""
    kw = dict(early_stop=True, patience=1, tolerance=0.5, max_rounds=16)
    a = _group("hip", "small", "median", rounds=2, **kw)
    b = _group("hip", "small", "median", rounds=8, **kw)
    assert a.history()["stop_round"] == b.history()["stop_round"] == 2 and b.history()["rounds_run"] == 2
    for ca, cb in zip(a.clients, b.clients):
        np.testing.assert_array_equal(ca.global_flat(), cb.global_flat())


# ---- three ranks sharing one GPU ----
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
        e = HipRoundEngine(X[idx[rank]], y[idx[rank]], 3, _cfg("small", "median"), comm,
                           init_flat(SMALL, 2 * 1000003 + rank), n_total=sum(len(i) for i in idx))
        agg, lay = e.aggregation, e.layout["aggregator"]
        e.run(ROUNDS)
        h = e.history()
        torch.cuda.synchronize()
        comm.Barrier()
        q.put((rank, (agg, lay, e.global_flat(), h["global"], h["loss"], h["per_rank"], h["rounds_run"]), None))
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
    g = _group("hip", "small", "median", k=3)
    h = g.history()
    ref = (g.global_flat(), h["global"], h["loss"], h["per_rank"], h["rounds_run"])
    for rank, res, _ in out:
        assert res[0] == "host-gather" and res[1] == "median"
        for a, b in zip(res[2:], ref):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank}")


# ---- refusals ----
def test_refusals():
    from fedmi.ops import native
    X, y = _data("small")
    flat = init_flat(SMALL, 0)
    sizes = [len(X)] * 3
    mk = lambda cfg, **kw: HipRoundEngine(X, y, 3, cfg, SimRank(3, 0, DEV), flat, n_total=3 * len(X),
                                          client_sizes=sizes, **kw)
    e = mk(_cfg("small", "median"))
    assert e.aggregation == "host-gather" and e.layout["aggregator"] == "median" and not e.engine.lagged
    assert e._peer is None and e._native_comm is None
    with pytest.raises(RuntimeError, match="issues its own FedAvg"):
        e.trace(1)
    with pytest.raises(RuntimeError, match="aggregated from Python"):
        e.prime_graph(4)
    with pytest.raises(ValueError, match="differential privacy"):
        mk(_cfg("small", "median", dp_clip=0.5, dp_seed=1))
    pimg = image_layout(SMALL)[2]
    bufs = [torch.zeros(pimg + 3 * 10, device=DEV) for _ in range(2)]
    with pytest.raises(ValueError, match="robust aggregator"):
        mk(_cfg("small", "trimmed_mean"), comm_buffers=bufs)
    one = HipRoundEngine(X, y, 3, _cfg("small", "median"), None, flat)
    assert one.aggregation == "none" and one.layout["aggregator"] == "mean" and one.robust == 0
    m = native()
    t = torch.zeros(pimg + TAILS, device=DEV)
    tab = _tab([t] * 65)
    with pytest.raises(RuntimeError, match="1..64 clients"):
        m.robust_aggregate(SMALL, 1, 0.0, tab.data_ptr(), 65, tab.data_ptr(), 1, _state(1, 0).data_ptr(),
                           _rtab([np.ones(64, bool)]).data_ptr(), TAILS, 1, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match="beta"):
        m.robust_aggregate(SMALL, 2, 0.5, tab.data_ptr(), 4, tab.data_ptr(), 1, _state(1, 0).data_ptr(),
                           _rtab([np.ones(4, bool)]).data_ptr(), TAILS, 1, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ValueError, match="at most 64 clients"):
        HipRoundEngine(X, y, 3, _cfg("small", "median"), SimRank(65, 0, DEV), flat, n_total=65 * len(X),
                       client_sizes=[len(X)] * 65)

"""The stochastic update compressors on the GPU: the kernel (fl_compress.hip, the stochastic entry)
against the host model ``compress_torch`` on the same inputs, bitwise; the engine around it checked in
situ from the engine's own buffers (local steps, bf16 packing, client sampling, a server optimizer, secure
aggregation); graph replays against eager rounds; resume; and the continuity of rand-k at ratio 1 with
dense rounds.

HIP-versus-torch trajectories are deliberately not compared at ratio < 1 or finite ``s``: a one-ulp
difference in ``u`` flips a rounding decision, and the two runs part ways for good.
"""
import numpy as np
import pytest
import torch

from fedmi.fl.compress import compress_round, qsgd_norm, randk_keys, topk_count, uplink_bytes
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, image_layout, image_to_dense, init_flat, param_count
from fedmi.privacy import philox

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr

pytestmark = pytest.mark.gpu

# 5-4-2: P = 34, less than one wave's worth of quads; 17-24-3: P = 507, no multiple of 4; 14-50-200-2:
# P = 11352, three workgroups, the last one partial -- the smallest shape where workgroups could disagree
KERNEL_DIMS = {"5-4-2": [5, 4, 2], "17-24-3": [17, 24, 3], "14-50-200-2": [14, 50, 200, 2]}
KINDS = {"qsgd": 3, "randk": 4}
MAX_ROUNDS = 8
COMM_GARBAGE, OUT_GARBAGE, STAT_GARBAGE = 123.0, 7.0, 9.0
SEED = 0xC0FFEE0123456789


def _bits(t):
    return np.ascontiguousarray(np.asarray(t, np.float32)).view(np.uint32)


def _same_bits(a, b, msg):
    a, b = _bits(a), _bits(b)
    nan = lambda t: (t & 0x7FFFFFFF) > 0x7F800000      # (a NaN's payload may differ: w * NaN)
    bad = (a != b) & ~(nan(a) & nan(b))
    assert not bad.any(), (msg, int(bad.sum()), np.flatnonzero(bad)[:8])


class KernelCase:
    """One fl_compress launch on buffers of its own.  Padding of local, x and the residual's input half
    holds huge values (read as data they would own the norm); comm (where the Adam kernel leaves
    w * local and zero padding), the residual's output half and the statistic table hold garbage, so
    whatever the kernel does not write is seen."""

    def __init__(self, dims, local, x, e, w, r, live=True, client=3):
        from fedmi.ops import native
        self.m, self.dims, self.r, self.w, self.client = native(), list(dims), int(r), float(np.float32(w)), int(client)
        self.P, self.Pimg = param_count(dims), image_layout(dims)[2]
        self.pad = dense_to_image(np.ones(self.P, np.float32), dims) == 0
        assert self.pad.sum() == self.Pimg - self.P and self.pad.any()
        self.dense = [np.asarray(t, np.float32) for t in (local, x, e)]
        dev = torch.device("cuda")

        def img(v, fill):
            out = dense_to_image(v, dims)
            out[self.pad] = fill
            return torch.as_tensor(out, device=dev)
        self.local, self.x = img(self.dense[0], 1e30), img(self.dense[1], -1e30)
        halves = [torch.full((self.Pimg,), OUT_GARBAGE, device=dev), torch.full((self.Pimg,), OUT_GARBAGE, device=dev)]
        halves[r & 1] = img(self.dense[2], 5e29)
        self.res = torch.cat(halves)
        self.comm = torch.full((self.Pimg + 5,), COMM_GARBAGE, device=dev)
        self.stat = torch.full((MAX_ROUNDS,), STAT_GARBAGE, device=dev)
        st = np.zeros(1, dtype=_STATE_DTYPE)
        st["live"], st["cur_round"], st["next_round"], st["stop_round"] = int(live), r, r + 1, -1
        self.state = torch.as_tensor(st.view(np.uint8).copy()).to(dev)
        rt = np.zeros(4 * MAX_ROUNDS, np.float32)
        rt[4 * r] = w
        self.rtab = torch.as_tensor(rt, device=dev)
        self.before = [t.clone() for t in (self.local, self.x, self.res, self.comm, self.stat)]

    def launch(self, kind, k=0, error_feedback=True, levels=127):
        torch.cuda.synchronize()
        self.m.compress_launch(self.dims, KINDS[kind], int(k), bool(error_feedback),
                               self.local.data_ptr(), self.x.data_ptr(), self.comm.data_ptr(), self.res.data_ptr(),
                               self.stat.data_ptr(), self.state.data_ptr(), self.rtab.data_ptr(), MAX_ROUNDS,
                               torch.cuda.current_stream().cuda_stream, levels=int(levels), client=self.client, seed=SEED)
        torch.cuda.synchronize()
        return self

    def half(self, which, t=None):
        t = self.res if t is None else t
        return t[which * self.Pimg:(which + 1) * self.Pimg].cpu().numpy()

    def check_untouched(self, what):
        names = ("local", "x", "residual", "comm", "stat")
        for name, now, old in zip(names, (self.local, self.x, self.res, self.comm, self.stat), self.before):
            if name in what:
                np.testing.assert_array_equal(_bits(now.cpu().numpy()), _bits(old.cpu().numpy()), err_msg=name)

    def check(self, kind, k, error_feedback=True, levels=127):
        """Contribution, new residual and statistic against compress_round of the same inputs, bitwise
        (qsgd: given the kernel's own norm, itself held to the host model of the sum by the caller);
        padding and everything else untouched."""
        r, P, Pimg = self.r, self.P, self.Pimg
        self.check_untouched(("local", "x"))
        np.testing.assert_array_equal(_bits(self.half(r & 1)), _bits(self.half(r & 1, self.before[2])))   # input half
        comm, out = self.comm.cpu().numpy(), self.half((r + 1) & 1)
        assert (comm[:Pimg][self.pad] == COMM_GARBAGE).all() and (comm[Pimg:] == COMM_GARBAGE).all(), "comm padding / tail"
        assert (out[self.pad] == OUT_GARBAGE).all(), "residual padding written"
        stat = self.stat.cpu().numpy()
        assert (np.delete(stat, r) == STAT_GARBAGE).all()
        norm = float(stat[r]) if kind == "qsgd" else None
        want, e_new, st = compress_round(*self.dense, self.w, kind, k, error_feedback, levels=levels, seed=SEED,
                                         round=r, client=self.client, norm=norm)
        _same_bits(image_to_dense(comm[:Pimg], self.dims), want.numpy(), "contribution")
        _same_bits(image_to_dense(out, self.dims), e_new.numpy(), "residual")
        _same_bits(stat[r:r + 1], np.float32([st]), "statistic")
        return stat[r]


def _inputs(P, seed, kind="random"):
    g = np.random.default_rng(seed)
    x = g.standard_normal(P).astype(np.float32)
    if kind == "random":
        return x + 0.05 * g.standard_normal(P).astype(np.float32), x, 0.02 * g.standard_normal(P).astype(np.float32)
    # crafted u: local = x, so u = (+0) + e = e
    if kind == "zeros":          # exact zeros of both signs and three entries
        e = np.zeros(P, np.float32)
        e[1::2] = -0.0
        e[[P - 1, 3, P // 2]] = [2.0, -3.0, 1.0]
    elif kind == "nan":          # the norm is not finite
        e = (0.02 * g.standard_normal(P)).astype(np.float32)
        e[P // 3] = np.nan
        e[P // 5] = -np.inf
    elif kind == "dominant":     # one entry 1e6 times the rest: the norm is that entry, give or take an ulp
        e = (0.02 * g.standard_normal(P)).astype(np.float32)
        e[P // 2] = -2e4
    return x.copy(), x, e


# ---- 1: the kernel against the host model ----
@pytest.mark.parametrize("shape", sorted(KERNEL_DIMS))
@pytest.mark.parametrize("inputs", ["random", "zeros", "nan", "dominant"])
def test_qsgd_kernel_matches_compress_torch_bitwise(shape, inputs):
    """Bitwise given the kernel's own norm; the norm itself equals the host model of the kernel's
    summation order (every workgroup holds the same one: the three workgroups of 14-50-200-2 write
    outputs that all follow block 0's statistic)."""
    dims = KERNEL_DIMS[shape]
    P = param_count(dims)
    local, x, e = _inputs(P, P + len(inputs), inputs)
    u = (torch.as_tensor(local) - torch.as_tensor(x)) + torch.as_tensor(e)
    for i, s in enumerate((1, 2, 127, 32767)):
        r = 2 + (i & 1)          # both buffer parities
        for ef in (True, False):
            norm = KernelCase(dims, local, x, e, 0.3, r).launch("qsgd", 0, ef, s).check("qsgd", P, ef, s)
            _same_bits([norm], [qsgd_norm(u)], "norm")
            assert (np.isfinite(norm) and norm > 0) == (inputs != "nan")


@pytest.mark.parametrize("shape", sorted(KERNEL_DIMS))
@pytest.mark.parametrize("inputs", ["random", "zeros", "nan", "dominant"])
def test_randk_kernel_matches_compress_torch_bitwise(shape, inputs):
    dims = KERNEL_DIMS[shape]
    P = param_count(dims)
    local, x, e = _inputs(P, P + len(inputs), inputs)
    ks = sorted({1, topk_count(0.01, P), P // 2, P})
    for i, k in enumerate(ks):
        r = 2 + (i & 1)          # both buffer parities
        for ef in (True, False):
            q = KernelCase(dims, local, x, e, 0.3, r).launch("randk", k, ef).check("randk", k, ef)
            key = np.sort(randk_keys(P, SEED, r, 3))[::-1]
            assert q == np.float32(key[k - 1]) * np.float32(2.0 ** -31)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("shape", sorted(KERNEL_DIMS))
def test_kernel_no_op_cases(kind, shape):
    dims = KERNEL_DIMS[shape]
    P = param_count(dims)
    local, x, e = _inputs(P, 5)
    for r in (2, 3):
        # not sampled: the contribution stays; the residual is carried to the half the next round reads
        c = KernelCase(dims, local, x, e, 0.0, r).launch(kind, topk_count(0.1, P))
        c.check_untouched(("local", "x", "comm"))
        np.testing.assert_array_equal(_bits(c.half(r & 1)), _bits(c.half(r & 1, c.before[2])))
        out = c.half((r + 1) & 1)
        assert (out[c.pad] == OUT_GARBAGE).all()
        np.testing.assert_array_equal(_bits(image_to_dense(out, dims)), _bits(e))
        stat = c.stat.cpu().numpy()
        assert stat[r] == 0 and (np.delete(stat, r) == STAT_GARBAGE).all()
        # not live: nothing at all
        KernelCase(dims, local, x, e, 0.3, r, live=False).launch(kind, topk_count(0.1, P)).check_untouched(
            ("local", "x", "residual", "comm", "stat"))
    if kind == "qsgd":   # u = 0 everywhere: norm 0, the round travels as it is (w * x)
        z = np.zeros(P, np.float32)
        assert KernelCase(dims, x, x, z, 0.5, 2).launch("qsgd", 0, True, 2).check("qsgd", P, True, 2) == 0


def test_module_constants_and_launch_arguments():
    from fedmi.ops import native
    m = native()
    assert (m.QSGD_STREAM, m.RANDK_STREAM) == (philox.QSGD_STREAM, philox.RANDK_STREAM)
    c = KernelCase([5, 4, 2], *_inputs(34, 1), 0.3, 2)
    for bad in (dict(kind=5), dict(kind=3, levels=0), dict(kind=3, levels=32768), dict(kind=4, k=0), dict(kind=4, k=35)):
        a = {**dict(kind=3, k=1, levels=127), **bad}
        with pytest.raises(RuntimeError, match="compress_launch"):
            m.compress_launch(c.dims, a["kind"], a["k"], True, c.local.data_ptr(), c.x.data_ptr(), c.comm.data_ptr(),
                              c.res.data_ptr(), c.stat.data_ptr(), c.state.data_ptr(), c.rtab.data_ptr(), MAX_ROUNDS,
                              torch.cuda.current_stream().cuda_stream, levels=a["levels"])
    c.check_untouched(("local", "x", "residual", "comm", "stat"))


# ---- 2: the engine, in situ ----
ENGINE_SHAPES = {"17-24-3": (96, 17, 3, (24,)), "14-50-200-2": (96, 14, 2, (50, 200))}


def _data(shape):
    rows, F, C, hidden = ENGINE_SHAPES[shape]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    return X, y, C, init_flat([F, *hidden, C], INIT_SEED), hidden


def _cfg(shape, **kw):
    return EngineConfig(**{**dict(hidden=ENGINE_SHAPES[shape][3], max_rounds=8, early_stop=False, graph_rounds=0,
                                  compress_seed=SEED, compress_levels=4), **kw})


def _engine(shape, **kw):
    X, y, C, flat, _ = _data(shape)
    return HipRoundEngine(X, y, C, _cfg(shape, **kw), None, flat)


def _check_contribution(e, r, comm_buf, tag):
    """The buffers of client `e` after round r's local phase: contribution and new residual are
    compress_round of the engine's own local model, round input and old residual, bitwise."""
    Pimg, dims = e.Pimg, e.dims
    d = lambda t: image_to_dense(t.cpu().numpy(), dims)
    pad = dense_to_image(np.ones(e.P, np.float32), dims) == 0
    w = float(e.rtab.cpu().numpy().view(np.float32)[4 * r])
    old, new = (e.cp_res[q * Pimg:(q + 1) * Pimg] for q in (r & 1, (r + 1) & 1))
    comm = comm_buf[:Pimg]
    assert not comm.cpu().numpy()[pad].any() and not new.cpu().numpy()[pad].any(), f"{tag}: padding"
    stat = float(e.cp_stat[r])
    if w == 0.0:
        assert not comm.any() and stat == 0 and torch.equal(old, new), f"{tag}: unsampled client"
        return False
    kind = e.cfg.compress
    want, e_new, st = compress_round(d(e.local), d(e.params[r & 1][:Pimg]), d(old), w, kind, e.compress_k,
                                     bool(e.cfg.error_feedback), levels=int(e.cfg.compress_levels),
                                     seed=e.compress_seed, round=r, client=e.rank,
                                     norm=stat if kind == "qsgd" else None)
    _same_bits(d(comm), want.numpy(), f"{tag}: contribution")
    _same_bits(d(new), e_new.numpy(), f"{tag}: residual")
    assert stat == np.float32(st) and stat > 0, (tag, stat, st)
    return True


@pytest.mark.parametrize("shape", sorted(ENGINE_SHAPES))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_engine_rounds_follow_the_rule_bitwise(kind, dtype, shape):
    """Step API, three local steps, four rounds (both buffer parities, residual non-zero from round 1 on)."""
    e = _engine(shape, compress=kind, dtype=dtype, local_steps=3)
    lay = e.layout["compress"]
    assert (lay["kind"], lay["k"], lay["dense_bytes"]) == (kind, e.compress_k, 4 * e.P)
    assert lay["uplink_bytes"] == uplink_bytes(kind, e.compress_k, e.P, 4) == e.uplink_bytes() < 4 * e.P
    assert lay.get("levels") == (4 if kind == "qsgd" else None)
    assert not e.engine.fused and e.compress_seed == SEED
    for r in range(4):
        g = e.global_flat()
        e.step_train()
        e.stream.synchronize()
        assert _check_contribution(e, r, e.params[(r + 1) & 1], f"{shape} {dtype} {kind} round {r}")
        if r:
            assert np.abs(g - e.local_flat()).max() > 0 and e.cp_res[(r & 1) * e.Pimg:][:e.Pimg].any()
        e.step_eval()
        e.step_aggregate()
    e.sync_history()
    h = e.history()
    assert h["rounds_run"] == 4 and (h["compress_stat"] > 0).all() and np.isfinite(h["loss"]).all()
    assert np.isfinite(e.global_flat()).all()


@pytest.mark.parametrize("case", ["server", "secagg", "participation"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_compositions_follow_the_rule_bitwise(kind, case):
    """Five clients in one process, one shared seed (the client index separates their words); the hook
    before the aggregation sees every client's clear buffers."""
    shape = "14-50-200-2"
    kw = {"server": dict(server_opt="adam", server_lr=1e-2), "secagg": dict(secagg=True),
          "participation": dict(participation=0.6, dtype="bf16", error_feedback=False)}[case]
    X, y, _, _, _ = _data(shape)
    seen = []

    def hook(r, bufs):
        g.stream.synchronize()
        seen.append([_check_contribution(e, r, b, f"{kind} {case} round {r} client {e.rank}")
                     for e, b in zip(g.clients, bufs)])
    g = ClientGroup(X, y, 5, _cfg(shape, compress=kind, **kw), backend="hip", tamper=hook)
    g.run(4)
    assert len(seen) == 4
    assert all(sum(s) == (3 if case == "participation" else 5) for s in seen)
    flat = g.global_flat()
    assert np.isfinite(flat).all()
    for e in g.clients[1:]:
        np.testing.assert_array_equal(e.global_flat(), flat)
    stats = np.stack([e.history()["compress_stat"] for e in g.clients])
    if kind == "randk" and case != "participation":   # same seed and round, another client: another selection
        assert len({float(v) for v in stats[:, 0]}) == 5


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_graph_replays_equal_eager_rounds_and_the_round_word_advances(kind, dtype):
    """A two-round graph replayed over four rounds: the round is read from the device state, so rounds 2
    and 3 draw their own words, not those baked in at capture."""
    out = []
    for g in (0, 2):
        e = _engine("14-50-200-2", compress=kind, dtype=dtype, graph_rounds=g)
        e.run(4)
        assert (e.engine.graph_captures > 0) == (g > 0)
        out.append((e.global_flat(), e.compress_residual, e.history()["compress_stat"], e.history()["loss"]))
    for a, b in zip(*out):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    stat = out[1][2]
    assert np.abs(out[1][1]).max() > 0 and (stat > 0).all() and len(set(stat.tolist())) == 4
    if kind == "randk":   # the quantile of round r's own keys
        P, k = e.P, e.compress_k
        want = [np.float32(np.sort(randk_keys(P, SEED, r, 0))[::-1][k - 1]) * np.float32(2.0 ** -31) for r in range(4)]
        np.testing.assert_array_equal(stat, np.float32(want))


def test_trace_reports_the_kind_and_single_kernel_timing_refuses():
    e = _engine("17-24-3", compress="qsgd")
    tr = e.trace(2, close=True)
    assert tr["launches"]["compress"] == 2 and tr["compress"] > 0 and "dp" not in tr["launches"], tr
    for call in (lambda: e.engine.time_kernels(1, 1, e.stream.cuda_stream), lambda: e.engine.launch_one(1, 0, e.stream.cuda_stream)):
        with pytest.raises(RuntimeError, match="compress"):
            call()
    with pytest.raises(RuntimeError, match="set_compress_seed"):
        _engine("17-24-3", compress="topk").engine.set_compress_seed(1)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_group_resume_continues_bit_for_bit_and_states_must_match(kind):
    X, y, C, flat, _ = _data("17-24-3")
    mk = lambda **kw: ClientGroup(X, y, 3, _cfg("17-24-3", compress=kind, **kw), backend="hip")
    snap = lambda g: [np.concatenate([e.global_flat(), e.local_flat(), e.compress_residual, e.history()["compress_stat"]])
                      for e in g.clients]
    a = mk(compress_seed=None)                               # private seeds: the state carries them
    a.run(3)
    states = [e.portable_state() for e in a.clients]
    assert len({st["compress_seed"] for st in states}) == 3
    b = mk(compress_seed=None)
    for e, st in zip(b.clients, states):
        e.load_portable_state(st)
        assert e.compress_seed == st["compress_seed"]
    b.rounds = 3
    a.run(3)
    b.run(3)
    for u, v in zip(snap(a), snap(b)):
        np.testing.assert_array_equal(_bits(u), _bits(v))
    # a fixed seed: the resumed run equals the uninterrupted one
    c, d, f = mk(), mk(), mk()
    c.run(3)
    for e, src in zip(d.clients, c.clients):
        e.load_portable_state(src.portable_state())
    d.rounds = 3
    d.run(3)
    f.run(6)
    for u, v in zip(snap(d), snap(f)):
        np.testing.assert_array_equal(_bits(u), _bits(v))
    one = _engine("17-24-3", compress=kind)
    one.run(2)
    st = one.portable_state()
    with pytest.raises(ValueError, match="compress_seed"):
        _engine("17-24-3", compress="topk").load_portable_state(st)
    with pytest.raises(ValueError, match="compress_seed"):
        _engine("17-24-3", compress=kind).load_portable_state(_engine("17-24-3", compress="sign").portable_state())
    # the torch engine takes the same state
    t = TorchRoundEngine(X, y, C, _cfg("17-24-3", compress=kind), None, flat)
    t.load_portable_state(st)
    assert t.compress_seed == st["compress_seed"]
    np.testing.assert_array_equal(_bits(t.compress_residual.numpy()), _bits(st["compress_residual"]))


# ---- 3: continuity with dense rounds ----
GROUP_EPS = 1e-4   # the clients' Adam eps (tests/test_server_opt.py: lr / eps amplifies fp32 roundings)


def test_full_randk_group_is_continuous_with_the_dense_group():
    """Rand-k at ratio 1 with error feedback keeps everything and its residual stays 0: the group differs
    from the dense group only by the rounding of fadd(x, fsub(local, x)) against local.  Four clients, six
    rounds, the clients' Adam eps at 1e-4; held to the project's 2e-5 (max|err| / max|ref|).
    Measured on MI355X: 2.3e-7 (docs/ARCHITECTURE.md)."""
    X, y, _, _, _ = _data("14-50-200-2")
    flats = []
    for kw in (dict(compress="randk", compress_ratio=1.0), {}):
        g = ClientGroup(X, y, 4, _cfg("14-50-200-2", eps=GROUP_EPS, **kw), backend="hip")
        g.run(6)
        flats.append(g.global_flat())
        if kw:
            assert not any(np.asarray(e.compress_residual).any() for e in g.clients)
            assert all((e.history()["compress_stat"] >= 0).all() for e in g.clients)
    dist = nerr(flats[0], flats[1])
    print("rand-k ratio 1 vs dense after 6 rounds: HIP pair", dist)
    assert dist <= 2e-5, dist

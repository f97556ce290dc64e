"""Update compression with error feedback on the GPU: the kernel (fl_compress.hip) against the host
model ``compress_torch`` on the same inputs, bitwise; the engine around it checked in situ from the
engine's own buffers (placement, buffer parity, rtab, local steps, compositions, graphs, bf16 packing,
resume); and the continuity of top-k at ratio 1 with dense rounds.

HIP-versus-torch trajectories are deliberately not compared for ratio < 1: a one-ulp difference at the
threshold flips a selection, and the two runs part ways for good.
"""
import numpy as np
import pytest
import torch

from fedmi.fl.compress import compress_round, sign_scale, topk_count, uplink_bytes
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, image_layout, image_to_dense, init_flat, param_count

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
# 5-4-2: P = 34, less than one wave's worth of quads; 17-24-3: P = 507, no multiple of 4; 14-50-200-2:
# P = 11352, three workgroups, the last one partial -- the smallest shape where workgroups could disagree
KERNEL_DIMS = {"5-4-2": [5, 4, 2], "17-24-3": [17, 24, 3], "14-50-200-2": [14, 50, 200, 2]}
MAX_ROUNDS = 8
COMM_GARBAGE, OUT_GARBAGE, STAT_GARBAGE = 123.0, 7.0, 9.0


def _bits(t):
    return np.ascontiguousarray(np.asarray(t, np.float32)).view(np.uint32)


def _same_bits(a, b, msg):
    a, b = _bits(a), _bits(b)
    nan = lambda t: (t & 0x7FFFFFFF) > 0x7F800000      # (a NaN's payload may differ: w * NaN)
    bad = (a != b) & ~(nan(a) & nan(b))
    assert not bad.any(), (msg, int(bad.sum()), np.flatnonzero(bad)[:8])


class KernelCase:
    """One fl_compress launch on buffers of its own.  Padding of local, x and the residual's input half
    holds huge values (read as data they would own every selection and the sign scale); comm (where the
    Adam kernel leaves w * local and zero padding), the residual's output half and the statistic table
    hold garbage, so whatever the kernel does not write is seen."""

    def __init__(self, dims, local, x, e, w, r, live=True):
        from fedmi.ops import native
        self.m, self.dims, self.r, self.w = native(), list(dims), int(r), float(np.float32(w))
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

    def launch(self, kind, k=0, error_feedback=True):
        torch.cuda.synchronize()
        self.m.compress_launch(self.dims, {"topk": 1, "sign": 2}[kind], int(k), bool(error_feedback),
                               self.local.data_ptr(), self.x.data_ptr(), self.comm.data_ptr(), self.res.data_ptr(),
                               self.stat.data_ptr(), self.state.data_ptr(), self.rtab.data_ptr(), MAX_ROUNDS,
                               torch.cuda.current_stream().cuda_stream)
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

    def check(self, kind, k, error_feedback=True):
        """Contribution, new residual and statistic against compress_torch of the same inputs, bitwise
        (sign: given the kernel's own s); padding and everything else untouched."""
        r, P, Pimg = self.r, self.P, self.Pimg
        self.check_untouched(("local", "x"))
        np.testing.assert_array_equal(_bits(self.half(r & 1)), _bits(self.half(r & 1, self.before[2])))   # input half
        comm, out = self.comm.cpu().numpy(), self.half((r + 1) & 1)
        assert (comm[:Pimg][self.pad] == COMM_GARBAGE).all() and (comm[Pimg:] == COMM_GARBAGE).all(), "comm padding / tail"
        assert (out[self.pad] == OUT_GARBAGE).all(), "residual padding written"
        stat = self.stat.cpu().numpy()
        assert (np.delete(stat, r) == STAT_GARBAGE).all()
        s = float(stat[r]) if kind == "sign" else None
        want, e_new, st = compress_round(*self.dense, self.w, kind, k, error_feedback, s=s)
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
    if kind == "equal":          # all magnitudes equal, mixed signs
        e = np.where(g.random(P) < 0.5, -0.25, 0.25).astype(np.float32)
    elif kind == "zeros":        # more exact zeros (of both signs) than P - k for every k > 3
        e = np.zeros(P, np.float32)
        e[1::2] = -0.0
        e[[P - 1, 3, P // 2]] = [2.0, -3.0, 1.0]
    elif kind == "groups":       # few distinct magnitudes: every k falls inside a tie group
        e = (np.round(2.0 * g.standard_normal(P)) / 8.0).astype(np.float32)
    elif kind == "nan":
        e = (0.02 * g.standard_normal(P)).astype(np.float32)
        e[P // 3] = np.nan
        e[P // 5] = -np.inf
    return x.copy(), x, e


# ---- 1: the kernel against the host model ----
@pytest.mark.parametrize("shape", sorted(KERNEL_DIMS))
@pytest.mark.parametrize("inputs", ["random", "equal", "zeros", "groups", "nan"])
def test_topk_kernel_matches_compress_torch_bitwise(shape, inputs):
    dims = KERNEL_DIMS[shape]
    P = param_count(dims)
    local, x, e = _inputs(P, P + len(inputs), inputs)
    ks = sorted({1, 2, topk_count(0.01, P), topk_count(0.1, P), P // 2, P - 1, P})
    for i, k in enumerate(ks):
        r = 2 + (i & 1)          # both buffer parities
        stat = KernelCase(dims, local, x, e, 0.3, r).launch("topk", k).check("topk", k)
        if inputs in ("random", "equal"):    # (the other inputs hold exact zeros)
            assert stat > 0
    KernelCase(dims, local, x, e, 1.0, 3).launch("topk", ks[3], error_feedback=False).check("topk", ks[3], False)


@pytest.mark.parametrize("shape", sorted(KERNEL_DIMS))
@pytest.mark.parametrize("inputs", ["random", "equal", "zeros", "groups"])
def test_sign_kernel_matches_compress_torch_and_its_scale_the_float64_sum(shape, inputs):
    """Bitwise given the kernel's own s.  s itself: every workgroup adds, per thread, at most
    ceil(P / 1024) magnitudes to a running sum (the first add, to +0, is exact, counted anyway), then 6
    xor-tree adds, then 16 wave-order adds (again from +0), then one division -- a chain of n =
    ceil(P / 1024) + 6 + 16 + 1 correctly rounded fp32 operations on non-negative terms, so every partial
    sum is at most the whole and |s - mean| <= n u mean (1 + n u)^n, u = 2^-24; the second-order factor is
    below 1 + 1e-5 at n <= 35 and covered by 1.001.  The host model of that order must agree bitwise."""
    dims = KERNEL_DIMS[shape]
    P = param_count(dims)
    local, x, e = _inputs(P, P + len(inputs), inputs)
    for r, ef in ((2, True), (3, False)):
        c = KernelCase(dims, local, x, e, 0.7, r).launch("sign", 0, ef)
        s = c.check("sign", P, ef)
        u = (torch.as_tensor(local) - torch.as_tensor(x)) + torch.as_tensor(e)
        mean = float(u.double().abs().sum()) / P
        n = (P + 1023) // 1024 + 6 + 16 + 1
        print(shape, inputs, "s", float(s), "float64 mean", mean, "err / bound", abs(float(s) - mean) / (n * U * mean))
        assert s > 0 and abs(float(s) - mean) <= 1.001 * n * U * mean
        assert _bits([s])[0] == _bits([sign_scale(u)])[0]


@pytest.mark.parametrize("kind", ["topk", "sign"])
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


# ---- 2: the engine, in situ ----
ENGINE_SHAPES = {"17-24-3": (96, 17, 3, (24,)), "14-50-200-2": (96, 14, 2, (50, 200))}


def _data(shape):
    rows, F, C, hidden = ENGINE_SHAPES[shape]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    return X, y, C, init_flat([F, *hidden, C], INIT_SEED), hidden


def _cfg(shape, **kw):
    return EngineConfig(**{**dict(hidden=ENGINE_SHAPES[shape][3], max_rounds=8, early_stop=False, graph_rounds=0), **kw})


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
                                     bool(e.cfg.error_feedback), s=stat if kind == "sign" else None)
    _same_bits(d(comm), want.numpy(), f"{tag}: contribution")
    _same_bits(d(new), e_new.numpy(), f"{tag}: residual")
    assert stat == np.float32(st) and stat > 0, (tag, stat, st)
    return True


@pytest.mark.parametrize("shape", sorted(ENGINE_SHAPES))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["topk", "sign"])
def test_engine_rounds_follow_the_rule_bitwise(kind, dtype, shape):
    """Step API, two local steps, five rounds (both buffer parities, residual non-zero from round 1 on).
    bf16: the packed image a round trains from is a pack of the fp32 global image (not the Adam-packed
    local model, which one dense bf16 client would stage)."""
    e = _engine(shape, compress=kind, dtype=dtype, local_steps=2)
    lay = e.layout["compress"]
    assert (lay["kind"], lay["k"], lay["dense_bytes"]) == (kind, e.compress_k, 4 * e.P)
    assert lay["uplink_bytes"] == uplink_bytes(kind, e.compress_k, e.P) == e.uplink_bytes() < 4 * e.P
    assert not e.layout["adam_spec"] and not e.engine.fused
    X, y, C, _, _ = _data(shape)
    for r in range(5):
        g = e.global_flat()
        e.step_train()
        e.stream.synchronize()
        assert _check_contribution(e, r, e.params[(r + 1) & 1], f"{shape} {dtype} {kind} round {r}")
        if r:
            assert np.abs(g - e.local_flat()).max() > 0 and e.cp_res[(r & 1) * e.Pimg:][:e.Pimg].any()
        if dtype == "bf16":
            f = HipRoundEngine(X, y, C, _cfg(shape, dtype="bf16", max_rounds=2), None, g)
            f.step_train()
            assert e.engine.packed_global(e.stream.cuda_stream) == f.engine.packed_global(f.stream.cuda_stream)
        e.step_eval()
        e.step_aggregate()
    e.sync_history()
    h = e.history()
    assert h["rounds_run"] == 5 and (h["compress_stat"] > 0).all() and np.isfinite(h["loss"]).all()
    assert np.isfinite(e.global_flat()).all()


@pytest.mark.parametrize("case", ["server", "median", "participation"])
@pytest.mark.parametrize("shape", sorted(ENGINE_SHAPES))
def test_compositions_follow_the_rule_bitwise(case, shape):
    """Four clients in one process; the hook before the aggregation sees every client's buffers."""
    kw = {"server": dict(compress="topk", server_opt="adam", server_lr=1e-2),
          "median": dict(compress="sign", aggregator="median"),
          "participation": dict(compress="topk", participation=0.5, dtype="bf16")}[case]
    X, y, _, _, _ = _data(shape)
    seen = []

    def hook(r, bufs):
        g.stream.synchronize()
        seen.append([_check_contribution(e, r, b, f"{shape} {case} round {r} client {e.rank}")
                     for e, b in zip(g.clients, bufs)])
    g = ClientGroup(X, y, 4, _cfg(shape, **kw), backend="hip", tamper=hook)
    g.run(6)
    assert len(seen) == 6
    assert all(sum(s) == (2 if case == "participation" else 4) for s in seen)
    flat = g.global_flat()
    assert np.isfinite(flat).all()
    for e in g.clients[1:]:
        np.testing.assert_array_equal(e.global_flat(), flat)
    if case == "server":
        assert np.abs(g.clients[0].server_m.cpu().numpy()).max() > 0
    if case == "median":
        assert float(g.clients[0].rtab.cpu().numpy().view(np.float32)[0]) == 1.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["topk", "sign"])
def test_graph_replays_equal_eager_rounds(kind, dtype):
    out = []
    for g in (0, 2):
        e = _engine("14-50-200-2", compress=kind, dtype=dtype, graph_rounds=g)
        e.run(6)
        assert (e.engine.graph_captures > 0) == (g > 0)
        out.append((e.global_flat(), e.compress_residual, e.history()["compress_stat"], e.history()["loss"]))
    for a, b in zip(*out):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert np.abs(out[0][1]).max() > 0 and (out[0][2] > 0).all()


def test_trace_reports_the_kind_and_single_kernel_timing_refuses():
    e = _engine("17-24-3", compress="topk")
    tr = e.trace(2, close=True)
    assert tr["launches"]["compress"] == 2 and tr["compress"] > 0 and "dp" not in tr["launches"], tr
    for call in (lambda: e.engine.time_kernels(1, 1, e.stream.cuda_stream), lambda: e.engine.launch_one(1, 0, e.stream.cuda_stream)):
        with pytest.raises(RuntimeError, match="compress"):
            call()
    d = _engine("17-24-3")
    assert d.layout["compress"] == {"kind": "none", "k": d.P, "uplink_bytes": 4 * d.P, "dense_bytes": 4 * d.P}
    assert "compress" not in d.trace(2, close=True)["launches"] and "compress_stat" not in d.history()


@pytest.mark.parametrize("kind", ["topk", "sign"])
def test_resume_continues_bit_for_bit_and_states_must_match(kind):
    a = _engine("17-24-3", compress=kind)
    a.run(3)
    st = a.portable_state()
    assert st["compress_residual"].shape == (a.P,) and np.abs(st["compress_residual"]).max() > 0
    b = _engine("17-24-3", compress=kind)
    b.load_portable_state(st)
    a.run(3)
    b.run(3)
    c = _engine("17-24-3", compress=kind)
    c.run(6)
    for e in (a, b):
        np.testing.assert_array_equal(_bits(e.global_flat()), _bits(c.global_flat()))
        np.testing.assert_array_equal(_bits(e.compress_residual), _bits(c.compress_residual))
        np.testing.assert_array_equal(e.history()["compress_stat"], c.history()["compress_stat"])
    with pytest.raises(ValueError, match="compress"):
        _engine("17-24-3").load_portable_state(st)
    with pytest.raises(ValueError, match="compress"):
        _engine("17-24-3", compress=kind).load_portable_state(_engine("17-24-3").portable_state())
    # the torch engine takes the same state
    X, y, C, flat, _ = _data("17-24-3")
    t = TorchRoundEngine(X, y, C, _cfg("17-24-3", compress=kind), None, flat)
    t.load_portable_state(st)
    np.testing.assert_array_equal(_bits(t.compress_residual.numpy()), _bits(st["compress_residual"]))


def test_early_stop_freezes_the_residual():
    e = _engine("17-24-3", compress="topk", early_stop=True, patience=2, tolerance=0.5, max_rounds=40)
    e.run(40)
    h = e.history()
    assert e.stopped and h["rounds_run"] == h["stop_round"] < 40
    res, flat = e.compress_residual, e.global_flat()
    both = e.cp_res.clone()
    e._stopped_seen = False      # issue rounds past the stop: exact no-ops on the device
    e._issue(3)
    e.sync_history()
    assert torch.equal(e.cp_res, both)
    np.testing.assert_array_equal(_bits(e.compress_residual), _bits(res))
    np.testing.assert_array_equal(_bits(e.global_flat()), _bits(flat))
    assert e.history()["rounds_run"] == h["rounds_run"]


# ---- 3: continuity with dense rounds ----
GROUP_EPS = 1e-4   # the clients' Adam eps (tests/test_server_opt.py: lr / eps amplifies fp32 roundings)


def test_full_topk_group_is_continuous_with_the_dense_group():
    """Top-k at ratio 1 keeps everything and its residual stays 0: the group differs from the dense
    group only by the rounding of fadd(x, fsub(local, x)) against local.  Four clients, six rounds, the
    clients' Adam eps at 1e-4.  The torch pair is measured first: inside the project's 2e-5
    (max|err| / max|ref|) the HIP pair is held to 2e-5, else to four times the torch distance.
    Measured on MI355X: torch pair 0 (x + (local - x) gives local back exactly here), HIP pair 2.3e-7
    (docs/ARCHITECTURE.md)."""
    X, y, _, _, _ = _data("14-50-200-2")
    dist = {}
    for backend in ("torch", "hip"):
        flats = []
        for kw in (dict(compress="topk", compress_ratio=1.0), {}):
            g = ClientGroup(X, y, 4, _cfg("14-50-200-2", eps=GROUP_EPS, **kw), backend=backend)
            g.run(6)
            flats.append(g.global_flat())
            if kw:
                res = [np.asarray(e.compress_residual) for e in g.clients]
                assert not any(r.any() for r in res), backend
        dist[backend] = nerr(flats[0], flats[1])
    bound = 2e-5 if dist["torch"] < 2e-5 else 4 * dist["torch"]
    print("top-k ratio 1 vs dense after 6 rounds: torch pair", dist["torch"], "HIP pair", dist["hip"], "bound", bound)
    assert dist["hip"] <= bound, dist

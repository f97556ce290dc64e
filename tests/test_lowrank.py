"""Low-rank update compression (``compress="powersgd"``) on the GPU: the kernel (fl_lowrank.hip) against the
host model ``lowrank_torch`` on the same inputs, bitwise; graph replays against eager rounds; a client group
against the torch group and a float64 oracle of the same rule; resume through the portable state."""
import functools

import numpy as np
import pytest
import torch

from fedmi.fl.compress import lowrank_layers, lowrank_q0, lowrank_torch
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, image_layout, image_to_dense, init_flat, param_count

from .reference_oracle import DATA_SEED, INIT_SEED, Float64RoundOracle, make_multiclass, nerr

pytestmark = pytest.mark.gpu

# 17-24-3: P = 507, one partial workgroup, odd K; 14-50-200-2: three workgroups that must agree, the last partial
SHAPES = {"small": [17, 24, 3], "14-50-200-2": [14, 50, 200, 2]}
MAX_ROUNDS = 8
GARBAGE = 7.0
cases = lambda f: pytest.mark.parametrize("shape", sorted(SHAPES))(pytest.mark.parametrize("r", [1, 2, 4, 8])(f))


def _same_bits(a, b, msg):
    a, b = (np.ascontiguousarray(np.asarray(t, np.float32)).view(np.uint32) for t in (a, b))
    nan = lambda t: (t & 0x7FFFFFFF) > 0x7F800000      # (a NaN's payload may differ)
    bad = (a != b) & ~(nan(a) & nan(b))
    assert not bad.any(), (msg, int(bad.sum()), np.flatnonzero(bad)[:8])


def _inputs(dims, r, kind):
    """Dense (local, x, e).  The crafted kinds set local = x, so u = e."""
    P, lay = param_count(dims), lowrank_layers(dims, r)["layers"]
    g = np.random.default_rng(P + r)
    x = g.standard_normal(P).astype(np.float32)
    if kind == "gauss":
        return x + 0.05 * g.standard_normal(P).astype(np.float32), x, 0.02 * g.standard_normal(P).astype(np.float32)
    e = (0.02 * g.standard_normal(P)).astype(np.float32)
    first, last = lay[0], [ly for ly in lay if ly["compressed"]][-1]
    blk = slice(first["w_off"], first["b_off"])
    if kind == "zero_layer":      # P = 0: every column is the zero column
        e[blk] = 0.0
    elif kind == "nonfinite":     # a NaN in the first compressed layer, an overflowing norm in the last
        e[first["w_off"] + 5], e[last["w_off"] + 7] = np.nan, 1e30
    elif kind == "rank1":         # the first layer exactly a b^T: the second direction is rounding noise
        e[blk] = (np.outer(g.integers(-4, 5, first["N"]), g.integers(-4, 5, first["K"])) / 64.0).astype(np.float32).reshape(-1)
    return x.copy(), x, e


def _launch(dims, r, local, x, e, q, w, rnd, ef=True, live=True):
    """One fl_lowrank launch on buffers of its own.  Image padding of the inputs holds huge values and every
    output buffer garbage, so whatever the kernel reads or leaves unwritten is seen.  Returns the padding mask
    and host copies of (comm, residual halves, Q halves, stat, local, x), before and after."""
    from fedmi.ops import native
    Pimg, dev = image_layout(dims)[2], torch.device("cuda")
    pad = dense_to_image(np.ones(param_count(dims), np.float32), dims) == 0

    def img(v, fill):
        out = dense_to_image(np.asarray(v, np.float32), dims)
        out[pad] = fill
        return torch.as_tensor(out, device=dev)
    res, qb = torch.full((2, Pimg), GARBAGE, device=dev), torch.full((2, len(q)), GARBAGE, device=dev)
    res[rnd & 1], qb[rnd & 1] = img(e, 5e29), torch.as_tensor(q, device=dev)
    comm, stat = torch.full((Pimg + 5,), GARBAGE, device=dev), torch.full((MAX_ROUNDS,), GARBAGE, device=dev)
    st = np.zeros(1, dtype=_STATE_DTYPE)
    st["live"], st["cur_round"], st["next_round"], st["stop_round"] = int(live), rnd, rnd + 1, -1
    state = torch.as_tensor(st.view(np.uint8).copy()).to(dev)
    rt = np.zeros(4 * MAX_ROUNDS, np.float32)
    rt[4 * rnd] = w
    rtab, loc, xi = torch.as_tensor(rt, device=dev), img(local, 1e30), img(x, -1e30)
    host = lambda: [t.cpu().numpy().copy() for t in (comm, res, qb, stat, loc, xi)]
    before = host()
    torch.cuda.synchronize()
    native().lowrank_launch(list(dims), r, bool(ef), loc.data_ptr(), xi.data_ptr(), comm.data_ptr(), res.data_ptr(),
                            qb.data_ptr(), stat.data_ptr(), state.data_ptr(), rtab.data_ptr(), MAX_ROUNDS,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return pad, before, host()


@cases
@pytest.mark.parametrize("inputs", ["gauss", "zero_layer", "nonfinite", "rank1"])
def test_kernel_is_bitwise_the_host_model(shape, r, inputs):
    dims = SHAPES[shape]
    Pimg = image_layout(dims)[2]
    local, x, e = _inputs(dims, r, inputs)
    q = lowrank_q0(dims, r, 11)
    u = (torch.as_tensor(local) - torch.as_tensor(x)) + torch.as_tensor(e)
    for rnd, ef in ((2, True), (3, True), (3, False)):      # both buffer parities
        pad, old, (comm, res, qb, stat, loc, xi) = _launch(dims, r, local, x, e, q, 0.3, rnd, ef)
        want_c, want_e, want_q, want_s = lowrank_torch(u, q, dims, r, ef)
        for a, b in zip((loc, xi, res[rnd & 1], qb[rnd & 1]), (old[4], old[5], old[1][rnd & 1], q)):
            _same_bits(a, b, "inputs written")
        out = res[(rnd + 1) & 1]
        assert (comm[:Pimg][pad] == GARBAGE).all() and (comm[Pimg:] == GARBAGE).all() and (out[pad] == GARBAGE).all(), "padding"
        assert (np.delete(stat, rnd) == GARBAGE).all()
        want = torch.tensor(np.float32(0.3)) * (torch.as_tensor(x) + want_c)
        _same_bits(image_to_dense(comm[:Pimg], dims), want.numpy(), f"contribution r{rnd} ef{ef}")
        _same_bits(image_to_dense(out, dims), want_e.numpy(), f"residual r{rnd} ef{ef}")
        _same_bits(qb[(rnd + 1) & 1], want_q.numpy(), f"Q r{rnd} ef{ef}")
        _same_bits(stat[rnd:rnd + 1], [want_s], f"stat r{rnd} ef{ef}")
    lay = lowrank_layers(dims, r)["layers"][0]
    if inputs == "nonfinite":   # the layer travelled raw and kept its Q
        assert (want_q.numpy()[:lay["K"] * r] == q[:lay["K"] * r]).all()
        _same_bits(want_c.numpy()[lay["w_off"]:lay["b_off"]], e[lay["w_off"]:lay["b_off"]], "raw layer")
    if inputs == "zero_layer":
        assert not want_q.numpy()[:lay["K"] * r].any()


@cases
def test_unsampled_and_not_live(shape, r):
    dims = SHAPES[shape]
    local, x, e = _inputs(dims, r, "gauss")
    q = lowrank_q0(dims, r, 11)
    for rnd in (2, 3):
        # not sampled: the contribution stays, residual and Q carry over to the half the next round reads
        pad, old, (comm, res, qb, stat, _, _) = _launch(dims, r, local, x, e, q, 0.0, rnd)
        out = res[(rnd + 1) & 1]
        assert (comm == GARBAGE).all() and (out[pad] == GARBAGE).all()
        _same_bits(image_to_dense(out, dims), e, "residual carried")
        _same_bits(qb[(rnd + 1) & 1], q, "Q carried")
        assert stat[rnd] == 0 and (np.delete(stat, rnd) == GARBAGE).all()
        _, old, new = _launch(dims, r, local, x, e, q, 0.3, rnd, live=False)      # not live: nothing at all
        for a, b in zip(old, new):
            _same_bits(a, b, "not live")


# ---- the engine ----
ENGINE = {"small": (96, 17, 3, (24,)), "14-50-200-2": (96, 14, 2, (50, 200))}
GROUP_EPS = 1e-4   # the clients' Adam eps (tests/test_server_opt.py: lr / eps amplifies fp32 roundings)


def _cfg(shape, r, **kw):
    return EngineConfig(**{**dict(hidden=ENGINE[shape][3], max_rounds=8, early_stop=False, graph_rounds=0,
                                  compress="powersgd", compress_rank=r, compress_seed=5), **kw})


def _engine(shape, r, **kw):
    rows, F, C, hidden = ENGINE[shape]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    return HipRoundEngine(X, y, C, _cfg(shape, r, **kw), None, init_flat([F, *hidden, C], INIT_SEED))


def _snap(e):
    return [e.global_flat(), e.local_flat(), e.compress_residual, e.compress_q, e.history()["compress_stat"]]


@cases
def test_graph_replays_and_resume_are_bitwise(shape, r):
    """A two-round captured graph replayed twice against four eager rounds; a portable_state() round trip at
    round 3 against six uninterrupted rounds."""
    eager, graph, first, second = (_engine(shape, r, graph_rounds=g) for g in (0, 2, 0, 0))
    eager.run(4)
    graph.run(4)
    assert graph.engine.graph_captures > 0 and eager.engine.graph_captures == 0
    for a, b in zip(_snap(eager), _snap(graph)):
        _same_bits(a, b, "graph vs eager")
    plan, lay = lowrank_layers(SHAPES[shape], r), eager.layout["compress"]
    assert (lay["kind"], lay["rank"], lay["k"], lay["uplink_bytes"]) == ("powersgd", r, plan["entries"], 4 * plan["entries"])
    assert lay["uplink_bytes"] == eager.uplink_bytes() and (_snap(eager)[4] > 0).all() and np.abs(_snap(eager)[2]).max() > 0
    eager.run(2)
    first.run(3)
    st = first.portable_state()
    assert st["compress_q"].shape == (plan["q_len"],)
    second.load_portable_state(st)
    second.run(3)
    for a, b in zip(_snap(eager), _snap(second)):
        _same_bits(a, b, "resumed vs uninterrupted")
    with pytest.raises(ValueError, match="compress_q"):
        _engine(shape, r, compress="sign").load_portable_state(st)


def _group(backend, shape, r, participation):
    X, y = make_multiclass(1200, ENGINE[shape][1], ENGINE[shape][2], DATA_SEED)
    return ClientGroup(X, y, 4, _cfg(shape, r, eps=GROUP_EPS, participation=participation), backend=backend,
                       shard_mode="iid", seed=2)


@functools.lru_cache(maxsize=None)
def _group_refs(shape, r, participation):
    """Six rounds of the fp32 torch group and of the same rule in float64, once per case (read-only)."""
    torch.set_num_threads(1)
    g = _group("torch", shape, r, participation)
    g.run(6)
    lead, dims, sizes = g.clients[0], g.clients[0].dims, [len(c.y) for c in g.clients]
    # (ClientGroup's seeding: one starting model per (seed, client); from round 1 on the clients share the aggregate)
    xs = [np.asarray(init_flat(dims, 2 * 1000003 + k), np.float64) for k in range(4)]
    os_ = [Float64RoundOracle(c.X.numpy(), c.y.numpy(), ENGINE[shape][2], lead.cfg, x) for c, x in zip(g.clients, xs)]
    es, qs = [np.zeros_like(x) for x in xs], [c._compress_q0.astype(np.float64) for c in g.clients]
    for rnd in range(6):
        part = [int(k) for k in lead.participants(rnd)]
        a = np.zeros_like(xs[0])
        for k, (o, x) in enumerate(zip(os_, xs)):
            with torch.no_grad():
                for p, v in zip(o.params, np.split(x, np.cumsum([p.numel() for p in o.params])[:-1])):
                    p.copy_(torch.as_tensor(v).view_as(p))
            if k in part:
                o.run(1)
                c, e, q, _ = lowrank_torch((o.weights() - x) + es[k], qs[k], dims, r)
                es[k], qs[k] = e.numpy(), q.numpy()
                a += (x + c.numpy()) * (sizes[k] / float(sum(sizes[j] for j in part)))
            else:
                o.scheduler.step()
        xs = [a] * 4
    return g.global_flat(), a


@pytest.mark.parametrize("shape, r, participation", [(s, r, 1.0) for s in sorted(SHAPES) for r in (1, 2, 4, 8)]
                         + [("14-50-200-2", 4, 0.5)])
def test_client_group_against_the_float64_rule(shape, r, participation):
    """Four clients, six fp32 rounds.  The weights' max|err| / max|ref| against the float64 oracle of the same
    rule is held to max(2e-5, 4 x the fp32 torch group's own error against that oracle): the margin the
    server-optimizer tests use for rules that amplify rounding -- here Gram-Schmidt where two singular values
    are close."""
    t_w, o_w = _group_refs(shape, r, participation)
    g = _group("hip", shape, r, participation)
    g.run(6)
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), g.clients[0].global_flat())
    eh, et = nerr(g.global_flat(), o_w), nerr(t_w, o_w)
    print(f"group {shape} r{r} p{participation}: HIP vs float64 {eh:.3g}  torch vs float64 {et:.3g}")
    assert eh <= max(2e-5, 4 * et), (eh, et)

"""Byzantine attack models on the device (fedmi/ops/csrc/fl_attack.hip): the launch alone against the numpy
model ``attack_model`` bit for bit (sign_flip, alie, ipm), the Gaussian client against float64 normals, a
captured graph against eager launches, HIP client groups against the same groups driven through ``tamper``
with ``attack_model`` on host copies of the buffers (bitwise) and against the torch groups, three ranks on
the host gather against the group (bitwise), the refusals.

Measured on the MI355X (HIP group against the torch group, 3 rounds, k = 7, two bad clients; limit 2e-5):
alie + median 1.2e-7, sign_flip + weighted mean 1.8e-7, ipm + multi_krum 1.2e-7; the Gaussian client's normals
lie within 0.64 of their bound (largest error 9.6e-7).

The Gaussian client's bound restates tests/test_dp_fedavg.py's for the same evaluation: 2 pi u1 is off by
<= 5.5e-7 (the fp32 constant and the product's rounding), sincosf by <= 2 ulp, so cos / sin by <= 9e-7
absolute, times the radius ``rad``; logf (2 ulp), sqrtf and the product rad * trig add <= 4 u relative
(u = 2^-24): the device's normal is within ``rad * 9e-7 + 4 u |n|`` of the float64 one.  Then the rule's own
operations: sigma * n (u |sigma n|, counted as 2 u like the DP test does), the addition m + sigma n (u |a|)
and, weighted, the product w a (u |w a|, i.e. u |a| after the division by w); m = div(c, w) is recomputed in
fp32 exactly as the device computes it and adds nothing.
"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.aggregate import mask_bits
from fedmi.fl.attack import ATTACKS, alie_z, attack_model, attack_normals
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_layout, image_to_dense, init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass, nerr

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL, INCOME = [17, 24, 3], [14, 50, 200, 2]
TAILS = 7
SENTINEL = -77.0
U = 2.0 ** -24
SCALE, Z = 0.75, 0.25
BAD_OF = {3: (1,), 8: (1, 4), 9: (1, 4), 64: (1, 4, 40, 63)}


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


@functools.lru_cache(maxsize=None)
def _real(dims):
    return dense_to_image(np.ones(param_count(list(dims)), np.float32), list(dims)) != 0


def _masks(K, bad, seed):
    """Full; with holes (a bad and an honest client stay); B_r empty; H_r empty."""
    rng = np.random.default_rng(seed)
    holes = rng.random(K) < 0.6
    honest = [k for k in range(K) if k not in bad]
    holes[[bad[0], honest[-1]]] = True
    holes[honest[0]] = False
    if len(bad) > 1:
        holes[bad[-1]] = False
    return [np.ones(K, bool), holes, ~np.isin(np.arange(K), bad) & (np.arange(K) % 2 == 0), np.isin(np.arange(K), bad)]


def _tables(masks, K, weighted, seed):
    """(rtab, wtab or None on the device, host weights [rounds, K] or None)."""
    sizes = np.random.default_rng(seed + 1).integers(20, 90, K).astype(np.float64)
    t = np.zeros((len(masks), 4), np.uint32)
    w = np.zeros((len(masks), K), np.float32)
    for r, m in enumerate(masks):
        bits = mask_bits(m)
        w[r, m] = (sizes[m] / sizes[m].sum()).astype(np.float32)
        t[r, 0] = w[r, 0].view(np.uint32) if weighted else np.float32(1.0).view(np.uint32)
        t[r, 1] = np.float32(m.sum()).view(np.uint32)
        t[r, 2], t[r, 3] = bits & 0xFFFFFFFF, bits >> 32
    rtab = torch.as_tensor(t.reshape(-1).view(np.int32)).to(DEV)
    return (rtab, torch.as_tensor(w).to(DEV), w) if weighted else (rtab, None, None)


def _inputs(dims, K, seed, w=None, nan_client=None):
    """([K, Pimg + TAILS] contributions, x): models 1 + 0.3 N(0, I) on the real parameters (times the client's
    weight), a sentinel in every source's image padding and tails; optionally NaN at a few real positions of
    one client."""
    pimg = image_layout(dims)[2]
    real = _real(tuple(dims))
    rng = np.random.default_rng(seed)
    a = np.empty((K, pimg + TAILS), np.float32)
    a[:, :pimg] = (1.0 + 0.3 * rng.standard_normal((K, pimg))).astype(np.float32)
    if nan_client is not None:
        a[nan_client, np.flatnonzero(real)[::37]] = np.nan
    if w is not None:
        a[:, :pimg] *= np.where(w > 0, w, np.float32(1.0))[:, None]
    a[:, :pimg][:, ~real] = SENTINEL
    a[:, pimg:] = SENTINEL
    x = (1.0 + 0.3 * rng.standard_normal(pimg)).astype(np.float32)
    x[~real] = 0.0
    return a, x, real, pimg


def _tab(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


def _launch(m, dims, kind, bufs, x, wtab, bad, state, rtab, rounds, scale=SCALE, z=Z, seed=0, stream=None, tab=None):
    tab = _tab(bufs) if tab is None else tab
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    m.attack_apply(dims, ATTACKS.index(kind), scale, z, seed, tab.data_ptr(), len(bufs), x.data_ptr(),
                   0 if wtab is None else wtab.data_ptr(), mask_bits(k in bad for k in range(len(bufs))),
                   state.data_ptr(), rtab.data_ptr(), rounds, s)
    if stream is None:
        torch.cuda.synchronize()


def _check_kernel(dims, K, kinds, weighted_modes=(False, True)):
    from fedmi.ops import native
    m = native()
    bad = BAD_OF[K]
    masks = _masks(K, bad, K)
    honest = [k for k in range(K) if k not in bad]
    for weighted in weighted_modes:
        rtab, wtab, w = _tables(masks, K, weighted, K)
        for r, mask in enumerate(masks):
            a, x, real, pimg = _inputs(dims, K, 10 * K + r, None if w is None else w[r], nan_client=honest[-1])
            xd = torch.as_tensor(x).to(DEV)
            for kind in kinds:
                tag = f"{kind} K={K} {'weighted' if weighted else 'unweighted'} mask={np.flatnonzero(mask).tolist()}"
                model = attack_model(a, x, mask, bad, kind, SCALE, Z, real, weights=None if w is None else w[r])
                bufs = [torch.as_tensor(row).to(DEV) for row in a]
                _launch(m, dims, kind, bufs, xd, None if wtab is None else wtab, bad, _state(1, r), rtab, len(masks))
                out = np.stack([b.cpu().numpy() for b in bufs])
                _same_bits(out, model, tag)
                changed = [k for k in range(K) if not np.array_equal(out[k].view(np.int32), a[k].view(np.int32))]
                B = [k for k in bad if mask[k]]
                H = [k for k in honest if mask[k]]
                noop = not B or (kind in ("alie", "ipm") and not H)
                assert changed == ([] if noop else B), tag
                # never written: padding and tails of every buffer keep the sentinel (the model says so too;
                # this is the statement on its own)
                assert (out[:, :pimg][:, ~real] == SENTINEL).all() and (out[:, pimg:] == SENTINEL).all(), tag
                if not noop and kind in ("alie", "ipm") and honest[-1] in H:
                    hole = np.flatnonzero(real)[::37]
                    assert np.isnan(out[B[0], hole]).all() and not np.isnan(np.delete(out[B[0], :pimg][real], np.s_[::37])).any(), tag
                if r == 0:
                    # a round that is not live, and a round past max_rounds, write nothing
                    for st, rounds in ((_state(0, r), len(masks)), (_state(1, len(masks)), len(masks))):
                        bufs = [torch.as_tensor(row).to(DEV) for row in a]
                        _launch(m, dims, kind, bufs, xd, None if wtab is None else wtab, bad, st, rtab, rounds)
                        _same_bits(np.stack([b.cpu().numpy() for b in bufs]), a, tag + " not live")


@pytest.mark.parametrize("K", [3, 8, 9])
def test_kernel_equals_the_model_bitwise(K):
    """K = 3 / 8: the float4 buckets (4, 8); K = 9: the first one-float bucket (16)."""
    _check_kernel(SMALL, K, ("sign_flip", "alie", "ipm"))


def test_kernel_equals_the_model_bitwise_64_clients():
    """The widest bucket, on the 14-50-200-2 image."""
    _check_kernel(INCOME, 64, ("sign_flip", "alie", "ipm"))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_gauss_against_float64_normals(weighted):
    from fedmi.ops import native
    m = native()
    K, bad, sigma, seed = 8, (1, 4), 0.5, 0x1234567890ABCDEF
    masks = [np.ones(K, bool), np.ones(K, bool)]
    rtab, wtab, w = _tables(masks, K, weighted, 3)
    P = param_count(SMALL)
    draws = {}
    for r in (0, 1):
        a, x, real, pimg = _inputs(SMALL, K, 50 + r, None if w is None else w[r])
        bufs = [torch.as_tensor(row).to(DEV) for row in a]
        _launch(m, SMALL, "gauss", bufs, torch.as_tensor(x).to(DEV), wtab, bad, _state(1, r), rtab, 2, scale=sigma, seed=seed)
        out = np.stack([b.cpu().numpy() for b in bufs])
        for k in range(K):
            if k not in bad:
                _same_bits(out[k], a[k], f"honest client {k}")
        assert (out[:, :pimg][:, ~real] == SENTINEL).all() and (out[:, pimg:] == SENTINEL).all()
        for k in bad:
            wk = np.float32(1.0) if w is None else w[r, k]
            mk = image_to_dense(a[k, :pimg] / wk if weighted else a[k, :pimg], SMALL).astype(np.float64)   # fp32 division, as the device's
            ak = image_to_dense(out[k, :pimg], SMALL).astype(np.float64) / float(wk)
            xi = (ak - mk) / sigma
            n = attack_normals(P, r, k, seed)
            rad = np.repeat(np.hypot(np.pad(n, (0, -P % 4))[0::2], np.pad(n, (0, -P % 4))[1::2]), 2)[:P]
            tol_n = rad * 9e-7 + 4 * U * np.abs(n)
            bound = (sigma * (tol_n + 2 * U * np.abs(n)) + (2 if weighted else 1) * U * np.abs(ak)) / sigma
            err = np.abs(xi - n)
            print(f"gauss {'weighted' if weighted else 'unweighted'} round {r} client {k}: max err / bound "
                  f"{float((err / bound).max()):.3g}, max err {err.max():.3g}")
            assert (err <= bound).all(), (r, k, float((err / bound).max()))
            draws[r, k] = xi
            # the model draws the same normals (rounded to fp32): within the same bound of the device
            model = attack_model(a, x, masks[r], bad, "gauss", sigma, 0.0, real, weights=None if w is None else w[r],
                                 seed=seed, round=r, dims=SMALL)
            em = np.abs(image_to_dense(model[k, :pimg], SMALL).astype(np.float64) / float(wk) - ak) / sigma
            assert (em <= bound + 2 * U * np.abs(n) + (2 if weighted else 1) * U * np.abs(ak) / sigma).all()
    # fresh draws every round and for every bad client
    for p, q in (((0, 1), (1, 1)), ((0, 1), (0, 4)), ((1, 1), (1, 4))):
        assert np.abs(draws[p] - draws[q]).max() > 1.0


def test_graph_replay_equals_eager_launches():
    """One captured graph per kind, replayed over two state updates whose rtab rows differ: the round -- the
    mask, the weights and gauss's counter -- comes from the state the launch reads."""
    from fedmi.ops import native
    m = native()
    K, bad = 9, BAD_OF[9]
    masks = _masks(K, bad, 4)[:2]
    rtab, wtab, w = _tables(masks, K, True, 4)
    a, x, real, pimg = _inputs(SMALL, K, 77)
    xd = torch.as_tensor(x).to(DEV)
    for kind in ("alie", "gauss"):
        eager = []
        for r in range(2):
            bufs = [torch.as_tensor(row).to(DEV) for row in a]
            _launch(m, SMALL, kind, bufs, xd, wtab, bad, _state(1, r), rtab, 2, seed=9)
            eager.append(np.stack([b.cpu().numpy() for b in bufs]))
        assert not np.array_equal(eager[0], eager[1])
        state = _state(1, 0)
        bufs = [torch.as_tensor(row).to(DEV) for row in a]
        tab = _tab(bufs)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            _launch(m, SMALL, kind, bufs, xd, wtab, bad, state, rtab, 2, seed=9,
                    stream=torch.cuda.current_stream().cuda_stream, tab=tab)
        torch.cuda.synchronize()
        for r in (0, 1, 0):
            state.copy_(_state(1, r))
            for b, row in zip(bufs, a):
                b.copy_(torch.as_tensor(row))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            _same_bits(np.stack([b.cpu().numpy() for b in bufs]), eager[r], f"{kind}: replay of round {r}")
        del tab


# ---- groups ----
ROUNDS = 3
GROUP_EPS = 1e-4   # the clients' Adam eps of the groups held to the torch group (tests/test_server_opt.py)
BAD = (1, 4)
SEED = 2
GROUPS = {
    "alie-median": dict(attack="alie", aggregator="median"),
    "sign_flip-mean": dict(attack="sign_flip", attack_scale=2.0),
    "ipm-multi_krum": dict(attack="ipm", attack_scale=0.5, screen="multi_krum", screen_byzantine=2),
}


def _cfg(**kw):
    base = dict(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, eps=GROUP_EPS)
    return EngineConfig(**{**base, **kw})


@functools.lru_cache(maxsize=None)
def _data():
    return make_multiclass(240, 17, 3, DATA_SEED)


def _group(backend, k=7, rounds=ROUNDS, tamper=None, common=False, **kw):
    X, y = _data()
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, _cfg(**kw), backend=backend, shard_mode="iid", seed=SEED, tamper=tamper)
    if common:   # the common initial model an attacked group starts from
        for c in g.clients:
            c.set_global_flat(init_flat(SMALL, SEED * 1000003))
    g.run(rounds)
    return g


def _assert_clients_agree(g):
    lead = g.clients[0]
    h = lead.history()
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), lead.global_flat())
        for key in ("global", "loss", "per_rank"):
            np.testing.assert_array_equal(c.history()[key], h[key])


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_hip_group_equals_the_group_driven_through_tamper(name):
    kw = GROUPS[name]
    g = _group("hip", attack_clients=BAD, **kw)
    lead = g.clients[0]
    z = float(np.float32(alie_z(7, 2)))
    assert lead.layout["attack"] == {"kind": kw["attack"], "clients": list(BAD),
                                     "scale": float(np.float32(kw.get("attack_scale", 1.0))),
                                     "z": z if kw["attack"] == "alie" else 0.0}
    _assert_clients_agree(g)
    real = _real(tuple(SMALL))
    plain = {k: v for k, v in kw.items() if not k.startswith("attack")}
    holder = {}

    def tamper(r, bufs):
        ref_lead = holder["clients"][0]
        stack = np.stack([b.cpu().numpy() for b in bufs])
        x = ref_lead.params[r & 1][:ref_lead.Pimg].cpu().numpy()
        w = None
        if not ref_lead.robust:   # the weighted mean: n_j / N in fp32, as the clients' per-round tables hold it
            w = np.array([np.float32(float(c.n_local) / float(ref_lead.n_total)) for c in holder["clients"]], np.float32)
        out = attack_model(stack, x, [True] * 7, BAD, kw["attack"], kw.get("attack_scale", 1.0), z, real, weights=w)
        for k in BAD:
            bufs[k].copy_(torch.as_tensor(out[k]))

    X, y = _data()
    torch.set_num_threads(1)
    ref = ClientGroup(X, y, 7, _cfg(**plain), backend="hip", shard_mode="iid", seed=SEED, tamper=tamper)
    holder["clients"] = ref.clients
    for c in ref.clients:
        c.set_global_flat(init_flat(SMALL, SEED * 1000003))
    ref.run(ROUNDS)
    assert "attack" not in ref.clients[0].layout
    np.testing.assert_array_equal(g.global_flat(), ref.global_flat())
    for key in ("global", "loss", "per_rank"):
        np.testing.assert_array_equal(g.history()[key], ref.history()[key])
    img = lead.params[g.rounds & 1][:lead.Pimg].cpu().numpy()
    np.testing.assert_array_equal(img.view(np.int32), ref.clients[0].params[ref.rounds & 1][:lead.Pimg].cpu().numpy().view(np.int32))
    assert (img[~real].view(np.int32) == 0).all()   # the zero-padding invariant
    if "screen" in kw:
        np.testing.assert_array_equal(g.history()["screen_kept"], ref.history()["screen_kept"])
    # the attack did something: the clean group ends elsewhere
    clean = _group("hip", common=True, **plain)
    assert not np.array_equal(clean.global_flat(), g.global_flat())
    # against the torch group
    t = _group("torch", attack_clients=BAD, **kw)
    err = nerr(g.global_flat(), t.global_flat())
    print(f"group {name}: HIP vs torch {err:.3g}")
    assert np.isfinite(g.global_flat()).all() and err <= 2e-5, err
    np.testing.assert_allclose(g.history()["loss"], t.history()["loss"], rtol=1e-4)


def test_hip_group_composes():
    """The stage in front of secure aggregation, with client sampling, a server optimizer, compression, the
    geometric median, gauss and bf16: the groups run, stay finite and their clients agree; under the sampled
    weighted mean the group is also held to the torch group."""
    for kw, held in ((dict(attack="gauss", attack_scale=0.01, secagg=True, secagg_seed=3), False),
                     (dict(attack="ipm", attack_scale=0.5, participation=0.7), True),
                     (dict(attack="alie", aggregator="geomed", server_opt="adam", server_lr=1e-2), False),
                     (dict(attack="sign_flip", compress="topk", dtype="bf16"), False)):
        g = _group("hip", attack_clients=BAD, **kw)
        assert g.history()["rounds_run"] == ROUNDS and np.isfinite(g.global_flat()).all(), kw
        _assert_clients_agree(g)
        if kw.get("dtype") != "bf16":
            err = nerr(g.global_flat(), _group("torch", attack_clients=BAD, **kw).global_flat())
            print(f"group {kw}: HIP vs torch {err:.3g}")
            assert not held or err <= 2e-5, (kw, err)


def test_label_flip_on_the_hip_group():
    clean = _group("hip", k=4, rounds=0)
    g = _group("hip", k=4, rounds=ROUNDS, attack="label_flip", attack_clients=(1,))
    for k, (c, d) in enumerate(zip(g.clients, clean.clients)):
        want = (2 - d.y.cpu().numpy()) if k == 1 else d.y.cpu().numpy()
        np.testing.assert_array_equal(c.y.cpu().numpy(), want)
    assert g.clients[0].layout["attack"]["kind"] == "label_flip" and not g.clients[0].attack_stage
    assert np.isfinite(g.global_flat()).all()


def test_attack_off_is_the_group_as_it_was():
    a = _group("hip", k=4)
    b = _group("hip", k=4, attack="none", attack_scale=3.0, attack_z=1.0, attack_seed=5)
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    ha, hb = a.history(), b.history()
    assert set(ha) == set(hb)
    for key in ("global", "loss", "per_rank"):
        np.testing.assert_array_equal(ha[key], hb[key])
    assert "attack" not in b.clients[0].layout and not hasattr(b, "_agg")


# ---- three ranks sharing one GPU ----
RANK_ROUNDS = 2
RANK_KW = dict(attack="alie", attack_clients=(1,), attack_z=1.0, aggregator="median")


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
        X, y = _data()
        idx = [shard_indices(len(X), r, world, mode="iid", seed=SEED, labels=y, alpha=0.5) for r in range(world)]
        e = HipRoundEngine(X[idx[rank]], y[idx[rank]], 3, _cfg(**RANK_KW), comm, init_flat(SMALL, SEED * 1000003),
                           n_total=sum(len(i) for i in idx))
        agg, lay = e.aggregation, e.layout["attack"]
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
    g = _group("hip", k=3, rounds=RANK_ROUNDS, **RANK_KW)
    lead, h = g.clients[0], g.history()
    ref = (lead.params[RANK_ROUNDS & 1][:lead.Pimg].cpu().numpy(), g.global_flat(), h["global"], h["loss"], h["rounds_run"])
    clean = _group("hip", k=3, rounds=RANK_ROUNDS, common=True, aggregator="median")
    assert not np.array_equal(clean.global_flat(), g.global_flat())
    for rank, res, _ in out:
        assert res[0] == "host-gather" and res[1] == {"kind": "alie", "clients": [1], "scale": 1.0, "z": 1.0}
        for a, b in zip(res[2:], ref):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank}")


# ---- refusals ----
def test_refusals():
    from fedmi.ops import native
    X, y = _data()
    flat = init_flat(SMALL, 0)

    class Rank:   # a rank of its own (not a ClientGroup's); refused before any collective
        def __init__(self, size):
            self.size, self.rank, self.device = size, 0, torch.device(DEV)

    mk = lambda comm, **kw: HipRoundEngine(X, y, 3, _cfg(**kw), comm, flat, n_total=3 * len(X), client_sizes=[len(X)] * 3)
    on = dict(attack="ipm", attack_clients=(1,))
    with pytest.raises(ValueError, match="attack='ipm'.*plain mean"):
        mk(Rank(3), **on)
    with pytest.raises(ValueError, match="attack='ipm'.*secagg"):
        mk(Rank(3), secagg=True, secagg_seed=1, **on)
    with pytest.raises(ValueError, match="attack='ipm'.*gather_plane='xgmi'"):
        mk(Rank(3), aggregator="median", gather_plane="xgmi", **on)
    with pytest.raises(ValueError, match="comm_buffers.*attack='ipm'"):
        HipRoundEngine(X, y, 3, _cfg(**on), SimRank(3, 0, DEV), flat, comm_buffers=(torch.zeros(8), torch.zeros(8)))
    e = mk(SimRank(3, 0, DEV), aggregator="median", **on)
    assert e.aggregation == "host-gather" and e.layout["attack"] == {"kind": "ipm", "clients": [1], "scale": 1.0, "z": 0.0}
    assert "attack" not in mk(SimRank(3, 0, DEV)).layout
    one = HipRoundEngine(X, y, 3, _cfg(attack="ipm", attack_clients=(5,), gather_plane="xgmi"), None, flat)   # one client: off
    assert one.attack == 0 and "attack" not in one.layout
    # the binding names the argument it refuses
    m = native()
    pimg = image_layout(SMALL)[2]
    t = torch.zeros(pimg + TAILS, device=DEV)
    tab = _tab([t] * 65)
    rtab = _tables([np.ones(64, bool)], 64, False, 0)[0]
    st = _state(1, 0)
    s = torch.cuda.current_stream().cuda_stream

    def args(kind=3, scale=1.0, z=1.0, K=4, x=None, bad=2, state=None, rt=None, rounds=1, src=None):
        return (SMALL, kind, scale, z, 0, tab.data_ptr() if src is None else src, K, t.data_ptr() if x is None else x, 0, bad,
                st.data_ptr() if state is None else state, rtab.data_ptr() if rt is None else rt, rounds, s)

    for bad_args, what in ((dict(kind=0), "kind"), (dict(kind=5), "kind"), (dict(K=0), "K must be"), (dict(K=65), "K must be"),
                           (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"), (dict(scale=1e60), "scale"),
                           (dict(z=float("inf")), "z must be"), (dict(bad=1 << 4), "bad_mask"), (dict(rounds=0), "max_rounds"),
                           (dict(src=0), "src"), (dict(x=0), "x "), (dict(state=0), "state"), (dict(rt=0), "rtab")):
        with pytest.raises(RuntimeError, match="attack_apply: " + what):
            m.attack_apply(*args(**bad_args))
    assert m.ATTACK_MAX_K == 64
    from fedmi.privacy.philox import ATTACK_STREAM
    assert m.ATTACK_STREAM == ATTACK_STREAM
    assert len({m.ATTACK_STREAM, m.SECAGG_STREAM, m.QSGD_STREAM, m.RANDK_STREAM, 0x46454450}) == 5

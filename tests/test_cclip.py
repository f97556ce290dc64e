"""Centered clipping on the GPU: fl_cclip bitwise ``cclip_model``, a captured graph, tampered groups, three ranks."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.aggregate import CCLIP_SLOT, cclip_model, cclip_scratch_floats, mask_bits
from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .cclip_oracle import cclip_group_f64
from .geomed_oracle import tamper_two
from .reference_oracle import DATA_SEED, make_multiclass, nerr
from .test_geomed import DEV, TAILS, _free_port, _rtab, _same_bits as _eq, _state, _tab   # (the launch-test plumbing)

pytestmark = pytest.mark.gpu

TAU, SENTINEL = 1.0, -77.0
SHAPES = {"small": (240, [17, 24, 3]), "income": (1200, [14, 50, 200, 2])}   # rows, dims


def _inputs(dims, K, seed):
    """x [Pimg] and [K, Pimg + TAILS]: client i at (0.3 + i % 3) tau from x, a NaN client (K >= 3), an overflow client
    (1e30, squared distance +inf; K >= 5), a 1e12 sign client (K >= 8); padding: 5 in x, NaN / 1e30 / 7 in the clients."""
    pimg, real = image_layout(dims)[2], dense_to_image(np.ones(param_count(dims), np.float32), dims) != 0
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(pimg).astype(np.float32)
    a = rng.standard_normal((K, pimg + TAILS)).astype(np.float32)
    for i in range(K):
        a[i, :pimg] = x + np.float32((0.3 + i % 3) * TAU / np.sqrt(real.sum())) * a[i, :pimg]
    if K >= 3:
        a[K // 2, :pimg] = np.nan
    if K >= 5:
        a[1, :pimg] = 1e30
    if K >= 8:
        a[2, :pimg] = np.float32(1e12) * np.sign(a[2, :pimg])
    a[:, :pimg][:, ~real], x[~real] = 7.0, 5.0
    a[0, :pimg][~real], a[1, :pimg][~real] = np.nan, 1e30
    return x, a, real, pimg


def _launch(dims, T, src, x, dst, state, rtab, rounds, scratch, keep=None, stream=None, tabs=None):
    from fedmi.ops import native
    tabs = tabs or (_tab(src), _tab(dst))
    native().cclip_aggregate(dims, T, TAU, tabs[0].data_ptr(), len(src), x.data_ptr(), tabs[1].data_ptr(), len(dst),
                             state.data_ptr(), rtab.data_ptr(), TAILS, rounds, scratch.data_ptr(),
                             stream or torch.cuda.current_stream().cuda_stream, 0 if keep is None else keep.data_ptr(),
                             dst_addrs=[t.data_ptr() for t in dst])
    stream or torch.cuda.synchronize()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("K", [2, 4, 5, 8, 9, 16, 17, 33, 64])   # every bucket (4 / 8 / 16 / 32 / 64) and its edges
def test_kernel_against_the_model(shape, K):
    from fedmi.ops import native
    dims = SHAPES[shape][1]
    x, a, real, pimg = _inputs(dims, K, 100 + K)
    assert pimg > 256 and pimg % 256 != 0 and not real[pimg - 1]   # several blocks, a partial one, ends in padding
    assert cclip_scratch_floats(pimg, 3) == native().cclip_scratch_floats(dims, 3) and CCLIP_SLOT == native().CCLIP_SLOT
    full, holes, kept = np.ones(K, bool), np.ones(K, bool), np.ones(K, bool)
    holes[np.random.default_rng(K).choice(K, K // 3, replace=False)] = False   # unsampled clients
    kept[[0, K // 2][:K - 1]] = False                                          # a screen's kept word
    nobody = np.where(np.arange(pimg + TAILS) == np.flatnonzero(real)[3], np.float32(np.nan), a)   # no finite distance
    rtab, xd = _rtab([full, holes]), torch.as_tensor(x).to(DEV)
    cases = [(a, 0, None, 3, K), (a, 1, None, 3, 0), (a, 0, kept, 3, 1), (nobody, 0, None, 3, 1), (a, 2, None, 3, 1),
             (a, -1, None, 3, 1)] + ([(a, 0, None, 1, 1)] if K == 5 else [])
    for rows, r, kw, T, n_dst in cases:   # input, round (2, -1: not live), keep word, T, destinations (0: in place)
        tag = f"K={K} round={r} keep={kw is not None} T={T} n_dst={n_dst}"
        stack = torch.as_tensor(rows).to(DEV)
        src = [stack[k] for k in range(K)]     # rows of a gathered stack: dword-aligned only
        dst = [torch.full((pimg + TAILS,), 7.0, device=DEV) for _ in range(n_dst)] or src
        scratch = torch.full((cclip_scratch_floats(pimg, T),), SENTINEL, device=DEV)
        keep = None if kw is None else torch.tensor([mask_bits(kw) - (mask_bits(kw) >> 63 << 64)], dtype=torch.int64, device=DEV)
        _launch(dims, T, src, xd, dst, _state(r >= 0, max(r, 0)), rtab, 2, scratch, keep)
        out = dst[0].cpu().numpy()
        for q in dst[1:]:
            _eq(q.cpu().numpy(), out, tag + ": destinations differ")
        if r in (2, -1):   # not live: the source-order sum of the whole buffer, and no scratch written
            _eq(out, functools.reduce(lambda s, t: s + t, torch.as_tensor(rows)).numpy(), tag)
            assert (scratch.cpu().numpy() == np.float32(SENTINEL)).all(), tag
            continue
        rec = []
        model = cclip_model(rows[:, :pimg], [full, holes][r] & (full if kw is None else kw), real, x, T, TAU, trace=rec)
        assert (rows is nobody) == (rec[0]["mask"] == 0), tag
        assert n_dst != K or (rec[0]["c"][0] == 1 and ((rec[0]["c"] > 0) & (rec[0]["c"] < 1)).any()), tag   # clipped and not
        _eq(out[:pimg], model, tag + ": image, padding exact 0")
        _eq(out[pimg:], functools.reduce(lambda s, t: s + t, torch.as_tensor(rows[:, pimg:])).numpy(), tag + ": tails")
        slots = scratch.cpu().numpy()[-T * CCLIP_SLOT:].reshape(T, CCLIP_SLOT)
        for l in range(T):
            _eq(slots[l, :K], rec[l]["c"], tag + f": c of iteration {l}")
            _eq(slots[l, 64:64 + K], rec[l]["d"], tag + f": d of iteration {l}")
            assert int(slots[l, 128:130].view(np.uint64)[0]) == rec[l]["mask"], (tag, l)
    with pytest.raises(RuntimeError):   # the centre among the destinations
        _launch(dims, 3, src, src[0], src, _state(1, 0), rtab, 2, scratch)


def test_graph_replay_equals_eager_launches():
    K, T, dims = 9, 3, SHAPES["small"][1]
    x, a, _, pimg = _inputs(dims, K, 5)
    masks = [np.ones(K, bool), np.arange(K) % 3 != 1, np.arange(K) == 4, np.arange(K) < 2]
    rtab, xd, stack = _rtab(masks), torch.as_tensor(x).to(DEV), torch.as_tensor(a).to(DEV)
    src, dst = [stack[k] for k in range(K)], [torch.zeros(pimg + TAILS, device=DEV)]
    scratch, eager = torch.zeros(cclip_scratch_floats(pimg, T), device=DEV), []
    for r in range(len(masks)):
        _launch(dims, T, src, xd, dst, _state(1, r), rtab, len(masks), scratch)
        eager.append(dst[0].cpu().numpy())
    assert len({e.tobytes() for e in eager}) == len(masks)
    state, stream, tabs = _state(1, 0), torch.cuda.Stream(), (_tab(src), _tab(dst))
    torch.cuda.synchronize()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        _launch(dims, T, src, xd, dst, state, rtab, len(masks), scratch, stream=torch.cuda.current_stream().cuda_stream, tabs=tabs)
    for r in [*range(len(masks)), 0]:
        state.copy_(_state(1, r))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _eq(dst[0].cpu().numpy(), eager[r], f"replay of round {r}")


def _group(backend, shape, k=7, rounds=6, tampered=True, **kw):
    rows, dims = SHAPES[shape]   # k = 7: clients 1 (NaN) and 4 (1e12 sign) tamper; the clients' Adam eps 1e-4
    cfg = EngineConfig(**{**dict(hidden=tuple(dims[1:-1]), max_rounds=8, early_stop=False, graph_rounds=0,
                                 aggregator="cclip", eps=1e-4), **kw})
    n = image_layout(dims)[2] if backend == "hip" else param_count(dims)
    g = ClientGroup(*make_multiclass(rows, dims[0], dims[-1], DATA_SEED), k, cfg, backend=backend, shard_mode="iid", seed=2,
                    tamper=tamper_two(n, 1, 4) if tampered else None)
    g.run(rounds)
    return g


@pytest.mark.parametrize("shape,kw", [("small", {}), ("income", {}), ("small", dict(server_opt="adam", server_lr=1e-2)),
                                      ("small", dict(dtype="bf16"))], ids=["small", "income", "server-adam", "bf16"])
def test_hip_group_with_two_tamperers(monkeypatch, shape, kw):
    g = _group("hip", shape, **kw)
    lead, w, dims = g.clients[0], g.global_flat(), SHAPES[shape][1]
    assert lead.layout["aggregator"] == "cclip" and lead.layout["cclip"] == {"iters": 3, "tau": 1.0, "launches": 4} \
        and np.isfinite(w).all() and g.history()["rounds_run"] == 6
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), w)
    if "dtype" in kw:
        return   # (bf16: finite, all clients agree; the fp32 groups are held to the torch group)
    t = _group("torch", shape, **kw)
    o_w = cclip_group_f64(monkeypatch, [(c.X.numpy(), c.y.numpy()) for c in t.clients], dims[-1], t.clients[0].cfg,
                          init_flat(dims, 2 * 1000003), 6, tamper_two(param_count(dims), 1, 4))
    cond, et, eo = nerr(t.global_flat(), o_w), nerr(w, t.global_flat()), nerr(w, o_w)
    print(f"group {shape} {kw}: torch vs float64 {cond:.3g}  HIP vs torch {et:.3g}  HIP vs float64 {eo:.3g}")
    assert et <= 2e-5 or eo <= 4 * cond, (et, eo, cond)


def _rank(rank, port, q):   # one of three ranks sharing the GPU
    os.environ.update(RANK=str(rank), WORLD_SIZE="3", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from fedmi.data.sharding import shard_indices
    from fedmi.parallel.comm import Comm
    comm = Comm(backend="xgmi", device="cuda:0", rccl=False)
    X, y = make_multiclass(240, 17, 3, DATA_SEED)
    idx = [shard_indices(len(X), r, 3, mode="iid", seed=2, labels=y, alpha=0.5) for r in range(3)]
    cfg = EngineConfig(hidden=(24,), max_rounds=8, early_stop=False, graph_rounds=0, aggregator="cclip", eps=1e-4)
    e = HipRoundEngine(X[idx[rank]], y[idx[rank]], 3, cfg, comm, init_flat([17, 24, 3], 2 * 1000003), n_total=sum(map(len, idx)))
    e.run(2)
    comm.Barrier()
    q.put((e.aggregation, e.global_flat(), e.history()["loss"]))
    comm.close()


def test_three_ranks_host_gather_equal_the_group_bitwise():
    q = mp.get_context("spawn").SimpleQueue()
    ctx = mp.spawn(_rank, args=(_free_port(), q), nprocs=3, join=False)
    try:   # (join raises with a failed rank's traceback; then nothing more runs on the GPU)
        assert any(ctx.join(10) for _ in range(12)), "the ranks did not finish"
    finally:
        for p in ctx.processes:
            p.terminate() if p.is_alive() else None
    g = _group("hip", "small", k=3, rounds=2, tampered=False)
    for agg, w, loss in (q.get() for _ in range(3)):
        assert agg == "host-gather"
        np.testing.assert_array_equal(w, g.global_flat())
        np.testing.assert_array_equal(loss, g.history()["loss"])

"""SCAFFOLD on the GPU: the capture and fold kernels (fl_scaffold.hip) bitwise their numpy models and against
float64, the identity on equal shards, groups against the torch specification, three ranks, a checkpoint."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.engine import _STATE_DTYPE, EngineConfig, HipRoundEngine
from fedmi.fl.scaffold import scaffold_capture_model, scaffold_fold_model
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass, nerr
from .scaffold_oracle import SCAFFOLD_SHAPES, scaffold_group, scaffold_group_f64
from .test_geomed import DEV, _free_port, _rtab, _same_bits as _eq, _tab

pytestmark = pytest.mark.gpu
U, SENTINEL, ROUNDS = 2.0 ** -24, -77.0, 4


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _st(**kw):
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["stop_round"] = -1
    for k, v in kw.items():
        rec[k] = v
    return torch.as_tensor(rec.view(np.uint8).copy()).to(DEV)


@pytest.mark.parametrize("n_blk", [1, 17, 33])
@pytest.mark.parametrize("shape", sorted(SCAFFOLD_SHAPES))
def test_capture_against_the_model_and_float64(shape, n_blk):
    from fedmi.ops import native
    F, C, hidden = SCAFFOLD_SHAPES[shape]
    P = param_count([F, *hidden, C])
    stride = (((P + 1) + 3) & ~3) + 8
    rng = np.random.default_rng(100 * n_blk + P)
    slab = (rng.standard_normal((n_blk + 1, stride)) * 10.0 ** rng.integers(-3, 2, (n_blk + 1, 1))).astype(np.float32)
    slab[n_blk, P:] = np.nan
    c, ci = rng.standard_normal((2, P)).astype(np.float32)
    rtab = _rtab([np.ones(4, bool)] * ROUNDS)
    dead = rtab.clone()
    dead[4 * 2] = 0   # round 2: this client's weight 0

    def launch(state, tab):
        d_slab, d_c, d_ci = _dev(slab), _dev(c), _dev(ci)
        out = torch.full((2, P), SENTINEL, dtype=torch.float32, device=DEV)
        native().scaffold_capture(P, stride, n_blk, d_slab.data_ptr(), d_c.data_ptr(), d_ci.data_ptr(),
                                  out[0].data_ptr(), out[1].data_ptr(), state.data_ptr(), tab.data_ptr(), ROUNDS,
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_slab.cpu().numpy(), out.cpu().numpy()

    got, (cnew, delta) = launch(_st(next_round=2), rtab)
    g, d_ref, corr = scaffold_capture_model(slab[:n_blk, :P], c, ci)
    rows64 = slab[:n_blk, :P].astype(np.float64)
    _eq(cnew, g, "cnew")
    assert (np.abs(cnew - rows64.sum(0)) <= (n_blk + 16) * U * np.abs(rows64).sum(0)).all()
    _eq(delta, d_ref, "delta")
    _eq(got[n_blk, :P], corr, "correction row")
    assert (got[n_blk, P:].view(np.int32) == 0).all()          # exact +0 over the NaN pre-fill, the loss slot included
    _eq(got[:n_blk], slab[:n_blk], "rows [0, n_blk)")
    for state, tab in ((_st(next_round=2, stopped=1), rtab), (_st(next_round=ROUNDS), rtab), (_st(next_round=2), dead)):
        got, out = launch(state, tab)   # not live, past max_rounds, weight 0: nothing is written
        _eq(got, slab, "slab")
        assert (out == SENTINEL).all()


@pytest.mark.parametrize("K", [2, 5, 64])
def test_fold_against_the_model(K):
    from fedmi.ops import native
    P, rng, on = 507, np.random.default_rng(K), np.ones(K, bool)
    on[1::3] = False                      # clients 1, 4, 7, ... sit the round out
    deltas = rng.standard_normal((K, P)).astype(np.float32)
    deltas[1] = np.inf                    # selected out, never multiplied by 0
    c, ci = rng.standard_normal(P).astype(np.float32), rng.standard_normal((K, P)).astype(np.float32)
    rtab = _rtab([np.ones(K, bool), on])

    def launch(state):
        d_c, d_d, d_i = _dev(np.stack([c, c])), _dev(deltas), _dev(ci)
        tabs = [_tab(list(t)) for t in (d_d, d_c, d_i)]
        native().scaffold_fold(P, tabs[0].data_ptr(), K, K, tabs[1].data_ptr(), 2, tabs[2].data_ptr(), K, 0,
                               state.data_ptr(), rtab.data_ptr(), 2, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_c.cpu().numpy(), d_i.cpu().numpy()

    got_c, got_i = launch(_st(live=1, cur_round=1, next_round=2))
    ref = scaffold_fold_model(c, deltas, on, K)
    assert np.isfinite(ref).all()
    _eq(got_c, np.stack([ref, ref]), "both replicas of c")
    _eq(got_i[on], ci[on] + deltas[on], "sampled clients' c_i: one fp32 addition of their delta")
    _eq(got_i[~on], ci[~on], "unsampled clients' c_i")
    got_c, got_i = launch(_st(live=0, cur_round=1, next_round=2))
    _eq(got_c, np.stack([c, c]), "c of a round that is not live")
    _eq(got_i, ci, "c_i of a round that is not live")


@pytest.mark.parametrize("k", [2, 4])
def test_equal_shards_are_the_plain_group_bitwise(k):
    """k clients on the same 120 rows, 3 local steps, 4 rounds, both groups from one model: every delta_i is equal and
    k a power of two, so c and every c_i take the same addition (the commit is c_i + delta_i, fedmi/fl/scaffold.py),
    the correction row is exact +0, and an added zero row moves no other row in the Adam kernel's order."""
    X, y = make_multiclass(120, 14, 2, DATA_SEED)
    flat = init_flat([14, 50, 200, 2], 2 * 1000003)

    def run(scaffold):
        cfg = EngineConfig(max_rounds=8, early_stop=False, graph_rounds=0, local_steps=3, scaffold=scaffold)
        g = ClientGroup(np.concatenate([X] * k), np.concatenate([y] * k), k, cfg, backend="hip", shard_mode="contiguous", seed=2)
        for e in g.clients:
            e.set_global_flat(flat)   # (the plain group's clients would start from one model each)
        g.run(4)
        return g

    a, b = run(True), run(False)
    assert a.clients[0].layout["scaffold"] and not b.clients[0].layout["scaffold"]
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    c = a.clients[0].scaffold_variates()[0]
    assert np.abs(c).max() > 1e-3
    for e in a.clients:
        np.testing.assert_array_equal(e.scaffold_variates()[1], c)


CASES = {"ls1": (1, 1.0, {}), "ls3": (3, 1.0, {}), "ls3-half": (3, 0.5, {}),
         "ls3-sgd": (3, 1.0, dict(server_opt="sgd", server_lr=1.0, server_momentum=0.0))}


@functools.lru_cache(maxsize=None)
def _references(shape, case):
    torch.set_num_threads(1)   # the torch group's roundings depend on the thread count
    ls, part, kw = CASES[case]
    tg = scaffold_group("torch", shape, ls, part, **kw)
    tg.run(6)
    return tg, scaffold_group_f64(tg, shape, 6)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("shape", sorted(SCAFFOLD_SHAPES))
def test_hip_group_against_the_torch_group(shape, case):
    """Six fp32 rounds of four label-skew clients: weights, c and every c_i within 2e-5 (max|err| / max|ref|) of the
    torch group, or, where the torch group is itself further than that from the float64 oracle, within 4 x its error."""
    ls, part, kw = CASES[case]
    tg, (o_w, o_c, o_ci) = _references(shape, case)
    g = scaffold_group("hip", shape, ls, part, **kw)
    g.run(6)
    hip = [g.global_flat(), g.clients[0].scaffold_variates()[0]] + [e.scaffold_variates()[1] for e in g.clients]
    ref = [tg.global_flat(), tg.clients[0].scaffold_variates()[0]] + [e.scaffold_variates()[1] for e in tg.clients]
    for e in g.clients[1:]:
        np.testing.assert_array_equal(e.scaffold_variates()[0], hip[1])
    np.testing.assert_allclose(g.history()["scaffold_norm"], tg.history()["scaffold_norm"], rtol=1e-5)
    for name, h, t, o in zip(["w", "c", "c_0", "c_1", "c_2", "c_3"], hip, ref, [o_w, o_c] + o_ci):
        et, cond, eo = nerr(h, t), nerr(t, o), nerr(h, o)
        print(f"{shape} {case} {name}: HIP vs torch {et:.3g}  torch vs float64 {cond:.3g}  HIP vs float64 {eo:.3g}")
        assert (et <= 2e-5) if cond <= 2e-5 else (eo <= 4 * cond), (name, et, cond, eo)


def _three():
    X, y = make_multiclass(240, 17, 3, DATA_SEED)
    return X, y, EngineConfig(hidden=(24,), max_rounds=8, early_stop=False, graph_rounds=0, eps=1e-4, local_steps=2,
                              scaffold=True)


def _rank(rank, port, q):   # one of three ranks sharing the GPU
    os.environ.update(RANK=str(rank), WORLD_SIZE="3", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from fedmi.data.sharding import shard_indices
    from fedmi.parallel.comm import Comm
    comm = Comm(backend="xgmi", device="cuda:0", rccl=False)
    X, y, cfg = _three()
    idx = [shard_indices(len(X), r, 3, mode="iid", seed=2, labels=y, alpha=0.5) for r in range(3)]
    e = HipRoundEngine(X[idx[rank]], y[idx[rank]], 3, cfg, comm, init_flat([17, 24, 3], 2 * 1000003), n_total=sum(map(len, idx)))
    e.run(3)
    comm.Barrier()
    q.put((rank, e.aggregation, e.global_flat(), *e.scaffold_variates()))
    comm.close()


def test_three_ranks_over_the_host_plane_equal_the_group_bitwise():
    q = mp.get_context("spawn").SimpleQueue()
    ctx = mp.spawn(_rank, args=(_free_port(), q), nprocs=3, join=False)
    try:   # (join raises with a failed rank's traceback; then nothing more runs on the GPU)
        assert any(ctx.join(10) for _ in range(12)), "the ranks did not finish"
    finally:
        for p in ctx.processes:
            p.terminate() if p.is_alive() else None
    X, y, cfg = _three()
    g = ClientGroup(X, y, 3, cfg, backend="hip", shard_mode="iid", seed=2)
    g.run(3)
    for rank, agg, w, c, ci in (q.get() for _ in range(3)):
        assert agg == "host"
        for got, ref in zip((w, c, ci), (g.global_flat(), *g.clients[rank].scaffold_variates())):
            np.testing.assert_array_equal(got, ref)


def test_checkpoint_after_three_rounds_resumes_to_the_six_round_run_bitwise(tmp_path):
    from fedmi.ckpt.checkpoint import resume, save_checkpoint
    a, b, c = (scaffold_group("hip", "small", 3, 0.5) for _ in range(3))
    a.run(6)
    b.run(3)
    for e in b.clients:
        save_checkpoint(str(tmp_path), e)
    for e in c.clients:
        assert resume(str(tmp_path), e) == 3
    c.rounds = 3
    c.run(3)
    np.testing.assert_array_equal(c.global_flat(), a.global_flat())
    for x, y in zip(c.clients, a.clients):
        for u, v in zip(x.scaffold_variates(), y.scaffold_variates()):
            np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(c.history()["scaffold_norm"], a.history()["scaffold_norm"])
    st = b.clients[0].portable_state()
    del st["scaffold_c"]
    with pytest.raises(ValueError, match="control variates"):
        c.clients[0].load_portable_state(st)

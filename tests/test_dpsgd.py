"""Record-level DP-SGD on MI355X: the per-example clipping train kernel (fl_train_dpsgd.hip) against the
float64 per-row oracle of tests/dpsgd_oracle.py.

Measured on MI355X, worst over all cases (docs/ARCHITECTURE.md 2.9 has the tables): row norms 1.5e-7 (bound 2e-5);
gradient partials 1.1e-5 per slab row and tensor (bound 2e-5) on the one-row last block of 129 rows at R = 16 of
14-50-200-2 with nothing clipped, below 6e-7 on every other case; loss slots 1.3e-7 (1e-4); noise normals at 0.43 of
the per-normal tolerance; six clipped rounds 1.2e-5 on the weights (2e-5), 3.4e-7 on the moments; with noise the HIP
engine is 0.26 to 1.5 times as far from the float64 oracle as the torch fp32 engine (bound 4 x).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.models.mlp import init_flat
from fedmi.privacy.philox import dpsgd_normals

from .dpsgd_oracle import DPSGD_SHAPES, Float64DpSgdOracle, clipped_sum, row_grads_f64
from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr
from .train_stage_oracle import block_slices, fp32_tensor_error, tensor_slices

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
REF = (14, 50, 200, 2)
_id = lambda d: "-".join(map(str, d))


@functools.lru_cache(maxsize=None)
def _case(dims, n):
    """The shard, the start model, the float64 per-row gradients and the median row norm, shared read-only."""
    X, y = make_multiclass(n, dims[0], dims[-1], DATA_SEED)
    flat = init_flat(list(dims), INIT_SEED)
    G, ce = row_grads_f64(flat, dims, X, y)
    for a in (X, y, flat, G, ce):
        a.setflags(write=False)
    return X, y, flat, G, ce, float(np.median(np.sqrt((G * G).sum(1))))


def _engine(dims, R, n, X=None, y=None, **kw):
    X0, y0, flat = _case(dims, n)[:3]
    cfg = EngineConfig(**{"hidden": dims[1:-1], "max_rounds": 8, "graph_rounds": 0, "early_stop": False,
                          "rows_per_block": R, **kw})
    return HipRoundEngine((X0 if X is None else X).copy(), (y0 if y is None else y).copy(), dims[-1], cfg, None, flat.copy())


def _launch(eng):
    """One step_train() over a NaN-filled slab: (partials, loss slots, raw slab rows)."""
    eng.slab.fill_(float("nan"))
    torch.cuda.synchronize()
    eng.step_train()
    eng.stream.synchronize()
    ns, stride = int(eng.engine.layout()["n_slabs"]), int(eng.engine.layout()["slab_stride"])
    return eng.slab_partials().cpu(), eng.slab_losses().cpu(), eng.slab[:ns * stride].view(ns, stride).cpu()


@pytest.mark.parametrize("which", ["above", "median", "tiny"])
@pytest.mark.parametrize("n_of", range(3), ids=["block-3", "2blocks+1", "129"])
@pytest.mark.parametrize("R", [16, 32])
@pytest.mark.parametrize("dims", DPSGD_SHAPES, ids=_id)
def test_one_launch_matches_the_per_row_oracle(dims, R, n_of, which):
    n = (R - 3, 2 * R + 1, 129)[n_of]
    X, y, flat, G, ce, med = _case(dims, n)
    ref_norms = np.sqrt((G * G).sum(1))
    C = {"above": 2.0 * ref_norms.max(), "median": med, "tiny": 1e-3 * ref_norms.min()}[which]
    eng = _engine(dims, R, n, dpsgd_clip=C)
    lay, nb = eng.engine.layout(), (n + R - 1) // R
    assert lay["dpsgd"] is True and lay["shape_spec"] is False and int(lay["n_slabs"]) == nb + 1
    part, loss, raw = _launch(eng)
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(loss).all())   # every slot was written
    e_norm = float(np.max(np.abs(eng.row_grad_norms().astype(np.float64) - ref_norms) / ref_norms))
    g, worst, blocks = part.double().numpy(), 0.0, block_slices(n, R)
    for b, sl in enumerate(blocks):
        ref = clipped_sum(G[sl], C, n)   # the block's rows, over the shard's n
        worst = max([worst] + [fp32_tensor_error(g[b, ts], ref[ts]) for _, ts in tensor_slices(dims)])
        if which == "tiny":   # every real row contributes norm C / n
            assert np.linalg.norm(g[b]) <= (sl.stop - sl.start) * C / n * (1 + 1e-5)
    ref_loss = np.array([ce[sl].sum() / n for sl in blocks])
    print(f"DPSGD {_id(dims)} R{R} n{n} {which}: norms {e_norm:.3e} grad {worst:.3e} "
          f"loss {np.max(np.abs(loss[:nb].double().numpy() - ref_loss) / ref_loss):.3e}")
    assert e_norm < 2e-5 and worst < 2e-5
    np.testing.assert_allclose(loss[:nb].double().numpy(), ref_loss, rtol=1e-4)
    assert not bool(raw[nb].view(torch.int32).bitwise_and(0x7FFFFFFF).any())   # z = 0: the noise row is zeros
    if which == "above":   # nothing is clipped: the option-off engine's partials, to the same bound
        off = _engine(dims, R, n)
        assert off.engine.layout()["dpsgd"] is False and int(off.engine.layout()["n_slabs"]) == nb
        p0, l0, _ = _launch(off)
        assert all(fp32_tensor_error(g[b, ts], p0[b].double().numpy()[ts]) < 2e-5
                   for b in range(nb) for _, ts in tensor_slices(dims))
        np.testing.assert_allclose(loss[:nb].numpy(), l0.numpy(), rtol=1e-4)


def test_noise_row_follows_the_philox_model():
    dims, n, R, C, z = (17, 24, 3), 45, 16, 0.7, 1.5
    nb, sigma, draws = (n + R - 1) // R, z * C / n, {}
    for ls, rounds, seed in itertools.product((1, 2), (1, 2), (5, 2 ** 40 + 9)):   # two ranks' private seeds
        eng = _engine(dims, R, n, dpsgd_clip=C, dpsgd_noise=z, dpsgd_seed=seed, local_steps=ls)
        eng.slab.fill_(float("nan"))
        eng.run(rounds)   # eager rounds: the slab keeps the draw of (rounds - 1, ls - 1)
        eng.stream.synchronize()
        P, stride = eng.P, int(eng.engine.layout()["slab_stride"])
        row = eng.slab[nb * stride:(nb + 1) * stride].cpu().double().numpy()
        assert np.all(np.isfinite(row)) and not np.any(row[P:])   # loss slot and padding: 0
        full = dpsgd_normals(P + (-P % 4), rounds - 1, ls - 1, 0, seed)   # whole blocks: the last pair's radius too
        nrm, rad = full[:P], np.repeat(np.hypot(full[0::2], full[1::2]), 2)[:P]
        # tests/test_dp_fedavg.py's per-normal tolerance tol_n, plus 4 U |normal| for the roundings of sigma
        # (the fp32 C, z C, 1 / n) and of the product
        tol = sigma * (rad * 9e-7 + 4 * U * np.abs(nrm) + 4 * U * np.abs(nrm))
        print(f"DPSGD-NOISE ls {ls} rounds {rounds} seed {seed}: worst err / tol {np.max(np.abs(row[:P] - sigma * nrm) / tol):.3f}")
        assert np.all(np.abs(row[:P] - sigma * nrm) <= tol)
        draws[(ls, rounds, seed)] = row[:P]
    assert all(not np.array_equal(draws[a], draws[b]) for a, b in itertools.combinations(draws, 2))


def test_one_changed_row_changes_its_slab_row_and_norm_only():
    n, row = 95, 40
    X, y, _, _, _, med = _case(REF, n)
    kw = dict(dpsgd_clip=med, dpsgd_noise=1.0, dpsgd_seed=3)
    e0 = _engine(REF, 32, n, **kw)
    base, norms0 = _launch(e0)[2].view(torch.int32), e0.row_grad_norms()
    X2, y2 = X.copy(), y.copy()
    X2[row], y2[row] = -X[row] + 0.25, 1 - y[row]
    e1 = _engine(REF, 32, n, X=X2, y=y2, **kw)
    got, norms1 = _launch(e1)[2].view(torch.int32), e1.row_grad_norms()
    assert [bool(torch.equal(got[b], base[b])) for b in range(4)] == [True, False, True, True]   # (row 3: the noise)
    assert (norms0.view(np.int32) != norms1.view(np.int32)).nonzero()[0].tolist() == [row]


def test_graph_replay_equals_eager_launches_and_seeds_repeat():
    def run(graph_rounds, seed):
        e = _engine(REF, 32, 129, dpsgd_clip=_case(REF, 129)[5], dpsgd_noise=0.8, dpsgd_seed=seed, local_steps=2,
                    max_rounds=16, graph_rounds=graph_rounds)
        e.run(8)
        return e.global_flat(), np.asarray(e.history()["loss"])
    eager, graph, again, other = run(0, 7), run(4, 7), run(0, 7), run(0, 8)
    assert np.array_equal(eager[0], graph[0]) and np.array_equal(eager[1], graph[1])   # 8 rounds: replay == eager
    assert np.array_equal(eager[0], again[0]) and not np.array_equal(eager[0], other[0])


@pytest.mark.parametrize("z", [0.0, 0.5], ids=["clip-only", "noise"])
@pytest.mark.parametrize("dims", [REF, (17, 24, 3)], ids=_id)
def test_six_rounds_follow_the_float64_dp_adam_oracle(dims, z):
    n, rounds = 97, 6
    X, y, flat, _, _, med = _case(dims, n)
    kw = dict(max_rounds=rounds + 2, early_stop=False, local_steps=2, dpsgd_clip=med, dpsgd_noise=z, dpsgd_seed=21)
    cfg = EngineConfig(hidden=dims[1:-1], **kw)
    oracle = Float64DpSgdOracle(X, y, dims[-1], cfg, flat, 21)
    oracle.run(rounds)
    w, m, v, loss = oracle.result()

    def distances(eng):
        eng.run(rounds)
        st = eng.portable_state()
        return (nerr(st["global"], w), nerr(st["exp_avg"], m), nerr(st["exp_avg_sq"], v),
                float(np.max(np.abs(np.asarray(eng.history()["loss"][:rounds], np.float64) - loss) / loss)))
    d_hip = distances(_engine(dims, 32, n, **kw))
    if z == 0.0:
        print(f"DPSGD-ROUNDS {_id(dims)} clip-only: hip {d_hip}")
        assert max(d_hip[:3]) < 2e-5 and d_hip[3] < 1e-4
        return
    d_ref = distances(TorchRoundEngine(X, y, dims[-1], cfg, None, flat))   # the fp32 specification's own distance
    print(f"DPSGD-ROUNDS {_id(dims)} z={z}: hip {d_hip} torch-fp32 {d_ref}")
    assert all(h <= 4 * t for h, t in zip(d_hip, d_ref)), (d_hip, d_ref)


def test_off_is_off():
    a, b = _engine(REF, 32, 129, dpsgd_clip=0.0), _engine(REF, 32, 129)
    lay = a.engine.layout()
    assert lay["dpsgd"] is False and lay["shape_spec"] is True and int(lay["n_slabs"]) == 5
    assert a.slab.numel() == b.slab.numel()
    a.run(4)
    b.run(4)
    assert np.array_equal(a.global_flat(), b.global_flat())
    with pytest.raises(RuntimeError, match="dpsgd_clip"):
        a.row_grad_norms()

"""Coalition utilities on the GPU: fl_coalition's build bitwise the numpy model, its scores against a float64 forward of
the device's own images, a captured graph against eager launches, and ClientGroup's contribution scores against torch."""
import numpy as np
import pytest
import torch

from fedmi.fl.contribution import (coalition_images_model, coalition_masks, coalition_slices, logits_f64, utility_f64)
from fedmi.fl.engine import _STATE_DTYPE, EngineConfig
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, image_layout, image_to_dense, init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL, INCOME, DEEP = [17, 24, 3], [14, 50, 200, 2], [11, 20, 36, 18, 4]
# K, dims, rows per block R, held-out rows, table: both bucket edges and the mask's width; a short last block (R - 3),
# several slices (2 R + 1), several blocks per slice (129 rows: 9 blocks in 8 slices / 5 blocks in 3 slices)
# The last entry seeds the inputs: chosen on the CPU so that in the float64 forward of the model's images every row's
# top-two logit margin exceeds 1e-4 max|logit| for every coalition of both rounds (the test asserts it)
CASES = [(2, SMALL, 16, 13, ("shapley", 0), 0), (5, INCOME, 16, 129, ("shapley", 0), 2), (9, DEEP, 16, 33, ("shapley", 2), 0),
         (64, SMALL, 32, 129, ("shapley", 1), 12)]


def _eq(a, b, msg=""):
    """Equal bit for bit (no NaN is expected on either side)."""
    np.testing.assert_array_equal(*(np.ascontiguousarray(t, np.float32).view(np.int32) for t in (a, b)), err_msg=msg)


def _state(live, r):
    rec = np.zeros(1, dtype=_STATE_DTYPE)
    rec["live"], rec["cur_round"], rec["next_round"], rec["stop_round"] = int(live), r, r + 1, -1
    return torch.as_tensor(rec.view(np.uint8).copy()).to(DEV)


def _rtab(sampled):
    """The round table of the sampled masks: weight 1, the count, the 64-bit mask in two words."""
    t = np.zeros((len(sampled), 4), np.uint32)
    for r, m in enumerate(sampled):
        bits = sum(1 << int(k) for k in np.flatnonzero(m))
        t[r] = np.float32(1.0).view(np.uint32), np.float32(m.sum()).view(np.uint32), bits & 0xFFFFFFFF, bits >> 32
    return torch.as_tensor(t.reshape(-1).view(np.int32)).to(DEV)


def _tab(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


def _case(K, dims, n, table, seed=0):
    """Sources [K, Pimg] = w_i (a common model + the client's own noise), x, the weights of a full and a half-sampled
    round (participation 0.5), held-out rows; padding tampered in the sources and x, the unsampled clients NaN."""
    rng = np.random.default_rng([seed, K, n])
    real = dense_to_image(np.ones(param_count(dims), np.float32), dims) != 0
    base = dense_to_image(init_flat(dims, 7 + seed), dims)
    sizes = rng.integers(20, 60, K).astype(np.float64)
    half = np.isin(np.arange(K), rng.choice(K, max(1, K // 2), replace=False))
    cw = np.stack([sizes / sizes.sum(), np.where(half, sizes / sizes[half].sum(), 0.0)]).astype(np.float32)
    models = base[None] + (0.05 * rng.standard_normal((K, len(base)))).astype(np.float32) * real
    v = [cw[r][:, None] * models for r in (0, 1)]
    v[1][~half] = np.nan                    # a NaN in a non-member never reaches a coalition's image
    for r in (0, 1):
        v[r][:, ~real] = 7.0
        v[r][0, ~real] = np.nan             # tampered padding
    x = np.where(real, base + np.float32(0.01), np.float32(5.0)).astype(np.float32)
    X, y = make_multiclass(n, dims[0], dims[-1], DATA_SEED + K)
    return v, cw, x, real, [np.ones(K, bool), half], coalition_masks(table[0], K, table[1], 3), X.astype(np.float32), y


def _bufs(K, dims, R, n, M, rounds=2):
    from fedmi.ops import native
    scratch = torch.full((native().coalition_scratch_floats(dims, M, n, R),), -77.0, device=DEV)
    return scratch, torch.full((rounds * M,), float("nan"), device=DEV), torch.full((rounds * M,), -1, dtype=torch.int32, device=DEV)


def _launch(dims, R, src_tab, K, x, masks_d, M, cw, scratch, Xd, yd, n, loss, correct, state, rtab, rounds, stream=None, slices=0):
    from fedmi.ops import native
    s = stream or torch.cuda.current_stream().cuda_stream
    native().coalition_build(dims, src_tab.data_ptr(), K, x.data_ptr(), masks_d.data_ptr(), M, cw.data_ptr(),
                             scratch.data_ptr(), state.data_ptr(), rtab.data_ptr(), rounds, s)
    native().coalition_score(dims, R, K, M, scratch.data_ptr(), Xd.data_ptr(), yd.data_ptr(), n, loss.data_ptr(),
                             correct.data_ptr(), state.data_ptr(), rounds, s, slices)
    stream or torch.cuda.synchronize()


@pytest.mark.parametrize("K,dims,R,n,table,seed", CASES, ids=[f"K{c[0]}" for c in CASES])
def test_build_bitwise_and_scores_against_float64(K, dims, R, n, table, seed):
    v, cw, x, real, sampled, masks, X, y = _case(K, dims, n, table, seed)
    M, pimg = len(masks), image_layout(dims)[2]
    assert 0 in masks and (1 << K) - 1 in [int(m) for m in masks] and any(bin(int(m)).count("1") == 1 for m in masks)
    n_blk = -(-n // R)
    assert (n % R != 0) and (K == 2 or coalition_slices(M, n_blk) > 1) and (n != 129 or n_blk > coalition_slices(M, n_blk))
    rtab, cwd, xd = _rtab(sampled), torch.as_tensor(cw).to(DEV), torch.as_tensor(x).to(DEV)
    md = torch.as_tensor(masks.view(np.int64).copy()).to(DEV)
    Xd, yd = torch.as_tensor(X).to(DEV), torch.as_tensor(y.astype(np.int32)).to(DEV)
    scratch, loss, correct = _bufs(K, dims, R, n, M)
    for r in (0, 1):
        stack = torch.as_tensor(v[r]).to(DEV)
        _launch(dims, R, _tab([stack[k] for k in range(K)]), K, xd, md, M, cwd, scratch, Xd, yd, n, loss, correct,
                _state(1, r), rtab, 2)
        bits = sum(1 << int(k) for k in np.flatnonzero(sampled[r]))
        img = scratch.cpu().numpy()[:M * pimg].reshape(M, pimg)
        _eq(img, coalition_images_model(v[r], cw[r], x, real, masks, bits), f"K={K} round {r}: images, padding exact 0")
        assert not np.isnan(img).any() and (img[:, ~real] == 0).all()   # round 1: the NaN clients are unsampled
        # the scoring stage against a float64 forward of the device's own images: the full round (every coalition is
        # what its mask says) and the half-sampled one
        got_l, got_c = loss.cpu().numpy()[r * M:(r + 1) * M], correct.cpu().numpy()[r * M:(r + 1) * M]
        for m in range(M):
            z = logits_f64(image_to_dense(img[m], dims), dims, X)
            top = np.sort(z, 1)
            assert ((top[:, -1] - top[:, -2]) > 1e-4 * np.abs(z).max()).all(), f"round {r} coalition {m}: a row's margin is too small"
            ref_l, ref_c = utility_f64(z, y)
            assert abs(got_l[m] - ref_l) <= 1e-4 * abs(ref_l) and got_c[m] == ref_c, (r, m, got_l[m], ref_l, got_c[m], ref_c)
    # one workgroup per (coalition, row block): other partial sums, the same counts
    _launch(dims, R, _tab([stack[k] for k in range(K)]), K, xd, md, M, cwd, scratch, Xd, yd, n, loss, correct,
            _state(1, 1), rtab, 2, slices=n_blk)
    np.testing.assert_array_equal(correct.cpu().numpy()[M:], got_c)
    np.testing.assert_allclose(loss.cpu().numpy()[M:], got_l, rtol=1e-5)


def test_graph_replay_equals_eager_and_a_dead_round_writes_nothing():
    K, dims, R, n, rounds = 5, SMALL, 16, 33, 4
    v, cw, x, _, _, masks, X, y = _case(K, dims, n, ("shapley", 0))
    M = len(masks)
    sampled = [np.ones(K, bool), np.arange(K) % 2 == 0, np.arange(K) == 3, np.arange(K) < 2]
    cw4 = np.stack([np.where(s, cw[0], 0) / cw[0][s].sum() for s in sampled]).astype(np.float32)
    rtab, cwd, xd = _rtab(sampled), torch.as_tensor(cw4).to(DEV), torch.as_tensor(x).to(DEV)
    md, stack = torch.as_tensor(masks.view(np.int64).copy()).to(DEV), torch.as_tensor(v[0]).to(DEV)
    Xd, yd, tab = torch.as_tensor(X).to(DEV), torch.as_tensor(y.astype(np.int32)).to(DEV), _tab([stack[k] for k in range(K)])
    scratch, loss, correct = _bufs(K, dims, R, n, M, rounds)
    args = (dims, R, tab, K, xd, md, M, cwd, scratch, Xd, yd, n)
    _launch(*args, loss, correct, _state(0, 1), rtab, rounds)   # not live: no row, no scratch
    _launch(*args, loss, correct, _state(1, rounds), rtab, rounds)   # past max_rounds
    assert np.isnan(loss.cpu().numpy()).all() and (correct.cpu().numpy() == -1).all() and (scratch.cpu().numpy() == -77.0).all()
    for r in range(rounds):
        _launch(*args, loss, correct, _state(1, r), rtab, rounds)
    eager = (loss.cpu().numpy().copy(), correct.cpu().numpy().copy())
    assert len({eager[0][r * M:(r + 1) * M].tobytes() for r in range(rounds)}) == rounds
    _, gl, gc = _bufs(K, dims, R, n, M, rounds)
    state, stream = _state(1, 0), torch.cuda.Stream()
    torch.cuda.synchronize()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        _launch(*args, gl, gc, state, rtab, rounds, stream=torch.cuda.current_stream().cuda_stream)
    for r in [*range(rounds), 0]:
        state.copy_(_state(1, r))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
    _eq(gl.cpu().numpy(), eager[0], "replayed loss rows")
    np.testing.assert_array_equal(gc.cpu().numpy(), eager[1])


def _group(backend, dims, rows, contribution="shapley", f64=False):
    cfg = EngineConfig(hidden=tuple(dims[1:-1]), max_rounds=8, early_stop=False, graph_rounds=0, attack="sign_flip",
                       attack_clients=(2,), attack_scale=3.0, contribution=contribution)
    X, y = make_multiclass(rows + 61, dims[0], dims[-1], DATA_SEED)
    g = ClientGroup(X[:rows], y[:rows], 4, cfg, backend=backend, shard_mode="iid", seed=2, heldout=(X[rows:], y[rows:]))
    if f64:
        g.contribution_dtype = torch.float64
    g.run(6)
    return g


@pytest.mark.parametrize("dims,rows", [(SMALL, 400), (INCOME, 1200)], ids=["small", "income"])
def test_group_scores_against_torch_and_leaves_the_round_alone(dims, rows):
    """Measured (docs/ARCHITECTURE.md 2.11): torch fp32 against the float64 oracle and HIP against torch, max|err| / max|ref|
    per round; the HIP group is held to 4 x the former, the rule for quantities that amplify image rounding."""
    hip, t, o = _group("hip", dims, rows), _group("torch", dims, rows), _group("torch", dims, rows, f64=True)
    plain = _group("hip", dims, rows, contribution="none")
    np.testing.assert_array_equal(hip.global_flat(), plain.global_flat())   # scoring must not disturb the round
    h, ht, ho = hip.history(), t.history(), o.history()
    assert set(h) - set(plain.history()) == {"coalition_masks", "coalition_loss_sum", "coalition_correct", "contribution",
                                             "contribution_acc"}
    assert hip.clients[0].layout["contribution"] == {"mode": "shapley", "coalitions": 16, "launches": 3}
    nerr = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for r in range(6):
        cond, err = nerr(ht["contribution"][r], ho["contribution"][r]), nerr(h["contribution"][r], ht["contribution"][r])
        print(f"group {dims} round {r}: torch vs float64 {cond:.3g}  HIP vs torch {err:.3g}")
        assert err <= 4 * cond, (r, err, cond)
        assert np.argmin(h["contribution"][r]) == 2 and np.argmin(ht["contribution"][r]) == 2   # the attacker ranks last

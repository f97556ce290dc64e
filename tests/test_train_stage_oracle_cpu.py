"""The per-workgroup train-launch oracle (tests/train_stage_oracle.py) against float64 autograd, and
the conditions under which tests/test_train_stage.py may hold the HIP kernels to it (CPU only).

* The block partials sum to float64 autograd of the full-batch mean cross-entropy (1e-12 relative),
  the loss slots to that cross-entropy; a partial block equals the oracle run on its live rows alone;
  changing one row changes the partial and loss slot of the block that owns it and of no other.
* Mask condition: every GPU case has a ReLU margin of at least 1e-5 on the model it is compared with,
  so no row or element is excluded from any comparison there.  Measured (data seed 3, init seed 1):
  exact 1.8e-5 (95x14-50-200-2) to 1.3e-3 (33x14-7-3), split-bf16 model 1.8e-5 to 1.3e-3; the plain
  bf16 model of 33x14-50-200-2 5.5e-5 (the 95-row shard has 6.2e-7 there and is not used plain).
* Yardstick: fp32 torch autograd of each block against the ``exact`` oracle, per tensor and slab row
  in the GPU test's metric, stays at or under 5e-6 -- a quarter of the 2e-5 asserted on the device --
  and the fp32 loss slot at or under 1e-5 relative, a tenth of its 1e-4.  Measured: gradients at most
  4.4e-7, loss at most 1.5e-7.
* The bf16 model of each block stays within 1e-2 relative L2 per tensor of the ``exact`` oracle
  wherever the GPU test asserts that bound on the device."""
import functools

import numpy as np
import pytest
import torch

from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, _dense_layers, make_multiclass
from .train_stage_oracle import (BF16_R64_CASE, LOCAL2_CASES, MIN_MARGIN, PLAIN_CASE, STAGE_CASES, block_slices, case_id,
                                 fp32_tensor_error, rel_l2, stage_oracle, tensor_slices)

ALL_CASES = STAGE_CASES + [BF16_R64_CASE]
IDS = [case_id(c) for c in ALL_CASES]


@functools.lru_cache(maxsize=None)
def _case(case):
    rows, F, C, hidden, R = case
    dims = [F, *hidden, C]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    flat = init_flat(dims, INIT_SEED)
    for a in (X, y, flat):
        a.setflags(write=False)
    return dims, X, y, flat


def _autograd(flat, X, y, dims, dtype, n=None):
    """(sum of the rows' CE / n, its gradient in dense order) by torch autograd in ``dtype``."""
    params = []
    for W, b in _dense_layers(flat, dims, dtype):
        params += [W.requires_grad_(), b.requires_grad_()]
    a = torch.as_tensor(np.asarray(X, np.float32)).to(dtype)
    for l in range(0, len(params), 2):
        a = a @ params[l].T + params[l + 1]
        if l + 2 < len(params):
            a = torch.relu(a)
    n = len(y) if n is None else n
    loss = torch.nn.functional.cross_entropy(a, torch.as_tensor(np.asarray(y), dtype=torch.long), reduction="sum") / n
    loss.backward()
    return float(loss.detach()), torch.cat([p.grad.reshape(-1) for p in params]).double().numpy()


def test_cases_cover_every_class_and_more_than_one_block_somewhere():
    for case in ALL_CASES + [PLAIN_CASE] + LOCAL2_CASES:
        rows, F, C, hidden, R = case
        assert rows <= 129
        y = _case(case)[2]
        assert sorted(set(y.tolist())) == list(range(C)), case
    assert any(c[0] % c[4] for c in ALL_CASES) and any(c[0] > c[4] for c in ALL_CASES)


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_block_partials_sum_to_float64_autograd(case):
    dims, X, y, flat = _case(case)
    ref = stage_oracle(flat, X, y, dims, case[4])
    loss, grad = _autograd(flat, X, y, dims, torch.float64)
    assert ref.grad.shape == ((case[0] + case[4] - 1) // case[4], len(flat)) and ref.loss.shape == ref.grad.shape[:1]
    assert abs(ref.loss.sum() - loss) <= 1e-12 * loss
    for name, sl in tensor_slices(dims):
        assert rel_l2(ref.grad[:, sl].sum(0), grad[sl]) <= 1e-12, name


@pytest.mark.parametrize("model,slab", [("exact", "fp32"), ("bf16", "fp32"), ("bf16", "fp16")])
@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_block_equals_the_oracle_on_its_rows_alone(case, model, slab):
    """Every block (the partial last one among them), run alone with the shard's n: bitwise its slab row."""
    dims, X, y, flat = _case(case)
    R, n = case[4], case[0]
    ref = stage_oracle(flat, X, y, dims, R, model, slab=slab)
    for b, s in enumerate(block_slices(n, R)):
        one = stage_oracle(flat, X[s], y[s], dims, R, model, slab=slab, n=n)
        assert one.grad.shape[0] == 1
        np.testing.assert_array_equal(one.grad[0], ref.grad[b])
        np.testing.assert_array_equal(one.loss[0], ref.loss[b])


@pytest.mark.parametrize("model,slab", [("exact", "fp32"), ("bf16", "fp16")])
@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[0] > c[4]], ids=[case_id(c) for c in ALL_CASES if c[0] > c[4]])
def test_changing_one_row_changes_exactly_its_block(case, model, slab):
    dims, X, y, flat = _case(case)
    R, n, C = case[4], case[0], case[2]
    ref = stage_oracle(flat, X, y, dims, R, model, slab=slab)
    for row in (n - 1, R, 0):
        X2, y2 = X.copy(), y.copy()
        X2[row] = -X[row] + 0.25
        y2[row] = (y[row] + 1) % C
        out = stage_oracle(flat, X2, y2, dims, R, model, slab=slab)
        for b in range(len(ref.loss)):
            same = np.array_equal(out.grad[b], ref.grad[b]) and out.loss[b] == ref.loss[b]
            assert same == (b != row // R), (row, b)
            assert (out.loss[b] != ref.loss[b]) == (b == row // R), (row, b)


def test_bf16_fp16_slab_rows_are_unscaled_sums():
    """The fp16 slab's rows are n times the mean's partials up to the delta's bf16 rounding point
    (before or after the 1/n), and the existing helper's full-batch result is the rows' sum / n."""
    from .reference_oracle import _split_bf16_reference_grad
    case = (95, 14, 2, (50, 200), 32)
    dims, X, y, flat = _case(case)
    h = stage_oracle(flat, X, y, dims, 32, "bf16", slab="fp16")
    f = stage_oracle(flat, X, y, dims, 32, "bf16", slab="fp32")
    np.testing.assert_allclose(h.grad.sum(0) / 95, _split_bf16_reference_grad(flat, X, y, dims), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(f.grad.sum(0), _split_bf16_reference_grad(flat, X, y, dims, scaled_delta=True),
                               rtol=1e-12, atol=1e-18)
    for name, sl in tensor_slices(dims):
        assert rel_l2(h.grad[:, sl] / 95, f.grad[:, sl]) <= 2.0 ** -7, name
    np.testing.assert_array_equal(h.loss, f.loss)


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_relu_margin_of_every_gpu_case(case):
    """The mask condition, on every model a GPU case is compared with within a bound."""
    dims, X, y, flat = _case(case)
    m = {"exact": stage_oracle(flat, X, y, dims, case[4]).margin,
         "bf16": stage_oracle(flat, X, y, dims, case[4], "bf16", slab="fp16").margin}
    if case == PLAIN_CASE:
        m["plain"] = stage_oracle(flat, X, y, dims, case[4], "bf16", plain=True, slab="fp16").margin
    print("MARGIN", case_id(case), m)
    assert min(m.values()) >= MIN_MARGIN, m


def test_plain_case_is_a_stage_case():
    assert PLAIN_CASE in STAGE_CASES and all(c in STAGE_CASES for c in LOCAL2_CASES)


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_fp32_autograd_is_within_a_quarter_of_the_gpu_bound(case):
    dims, X, y, flat = _case(case)
    R, n = case[4], case[0]
    ref = stage_oracle(flat, X, y, dims, R)
    worst_g = worst_l = 0.0
    for b, s in enumerate(block_slices(n, R)):
        loss, grad = _autograd(flat, X[s], y[s], dims, torch.float32, n=n)
        worst_l = max(worst_l, abs(loss - ref.loss[b]) / ref.loss[b])
        for name, sl in tensor_slices(dims):
            if np.any(ref.grad[b, sl]):
                worst_g = max(worst_g, fp32_tensor_error(grad[sl], ref.grad[b, sl]))
            else:
                assert not np.any(grad[sl]), (b, name)
    print("YARDSTICK", case_id(case), f"grad {worst_g:.2e} loss {worst_l:.2e}")
    assert worst_g <= 5e-6, worst_g
    assert worst_l <= 1e-5, worst_l


@pytest.mark.parametrize("slab", ["fp32", "fp16"])
@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_bf16_model_blocks_track_the_exact_oracle(case, slab):
    """Per tensor and slab row the bf16 model sits within the 1e-2 the device is held to against the
    ``exact`` oracle (measured: 2.6e-3 to 5.9e-3, and 8.8e-3 on the fp16 slab's rows of 95x14-50-200-2)."""
    dims, X, y, flat = _case(case)
    R, n = case[4], case[0]
    ex = stage_oracle(flat, X, y, dims, R)
    bf = stage_oracle(flat, X, y, dims, R, "bf16", slab=slab)
    scale = n if slab == "fp16" else 1
    worst = 0.0
    for b in range(len(ex.loss)):
        for name, sl in tensor_slices(dims):
            worst = max(worst, rel_l2(bf.grad[b, sl] / scale, ex.grad[b, sl]))
    print("BF16-VS-EXACT", case_id(case), slab, f"{worst:.2e}")
    assert worst <= 1e-2, worst

"""The fused round kernels against the oracle off the income shape: more than two classes (the
general softmax-CE epilogue, the device metric fold), feature widths other than 14, shards
around one workgroup, Adam with weight decay / non-default betas and eps / an LR schedule that
steps inside the run, and the Adam moments themselves.  tests/test_oracle_noise.py bounds the
fp32 oracle's own distance from float64 on the same cases at a quarter of the bounds used here."""
import functools

import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.fl.metrics import metric_vector, metrics_from_confusion
from fedmi.models.mlp import init_flat

from .reference_oracle import (BF16_GRAD_CASES, BF16_TRACK_CASES, BF16_TRACK_ROWS, DATA_SEED, INIT_SEED, OPT_CASES,
                               SHAPE_CASES, _split_bf16_reference_grad, float64_logits, make_multiclass, nerr)

pytestmark = pytest.mark.gpu

ROUNDS = 6


def _cfg(hidden, kw, **extra):
    # two rounds of head room: the schedule table is longer than the run
    return EngineConfig(hidden=hidden, max_rounds=ROUNDS + 2, graph_rounds=0, early_stop=False, **kw, **extra)


@functools.lru_cache(maxsize=None)
def _oracle_run(rows, F, C, hidden, kw_items):
    """ROUNDS rounds of the fp32 torch oracle, computed once per case and shared (read-only)."""
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    ref = TorchRoundEngine(X, y, C, _cfg(hidden, dict(kw_items)), None, init_flat([F, *hidden, C], INIT_SEED))
    ref.run(ROUNDS)
    st = ref.portable_state()
    out = {"w": ref.global_flat(), "m": st["exp_avg"], "v": st["exp_avg_sq"], "loss": ref.history()["loss"],
           "global": ref.history()["global"]}
    for a in out.values():
        a.setflags(write=False)
    return out


def _check_round_vs_oracle(rows, F, C, hidden, R, kw):
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    hip = HipRoundEngine(X, y, C, _cfg(hidden, kw, rows_per_block=R), None, init_flat([F, *hidden, C], INIT_SEED))
    assert hip.R == R
    hip.run(ROUNDS)
    ref = _oracle_run(rows, F, C, tuple(hidden), tuple(sorted(kw.items())))
    st = hip.portable_state()
    h = hip.history()
    err = {"weights": nerr(hip.global_flat(), ref["w"]), "exp_avg": nerr(st["exp_avg"], ref["m"]),
           "exp_avg_sq": nerr(st["exp_avg_sq"], ref["v"]),
           "loss": float(np.max(np.abs(h["loss"].astype(np.float64) - ref["loss"]) / np.abs(ref["loss"]))),
           "acc": float(np.max(np.abs(h["global"][:, 0] - ref["global"][:, 0])))}
    print((rows, F, C, hidden, R, kw), err)
    assert err["weights"] < 2e-5, err
    assert err["exp_avg"] < 2e-5, err
    assert err["exp_avg_sq"] < 2e-5, err
    np.testing.assert_allclose(h["loss"], ref["loss"], rtol=1e-4)
    if rows < 500:  # 2e-3 is less than one row here: at most one row's prediction may differ
        np.testing.assert_allclose(h["global"][:, 0], ref["global"][:, 0], rtol=0, atol=1.0 / rows + 1e-12)
    else:
        np.testing.assert_allclose(h["global"], ref["global"], atol=2e-3)


# ---- A: fp32 round vs torch, shapes ----
@pytest.mark.parametrize("R", [16, 32])
@pytest.mark.parametrize("rows,F,C,hidden", SHAPE_CASES)
def test_round_matches_torch_off_the_income_shape(rows, F, C, hidden, R):
    """Six fp32 rounds vs the torch oracle: weights, Adam moments (2e-5 of the largest entry),
    loss (rtol 1e-4) and accuracy (one row) on C > 2 (general CE epilogue), C = 16, F = 1 / 17 / 33
    and shards of fewer than R, exactly R and R + 1 rows."""
    _check_round_vs_oracle(rows, F, C, hidden, R, {})


# ---- B: fp32 round vs torch, optimizer ----
@pytest.mark.parametrize("name,rows,F,C,hidden,kw", OPT_CASES, ids=[c[0] for c in OPT_CASES])
def test_round_matches_torch_optimizer_settings(name, rows, F, C, hidden, kw):
    """Weight decay, a StepLR that steps three times inside the run, non-default betas / eps / lr,
    and all of them with local steps and the FedProx term: the same bounds as the shape cases."""
    _check_round_vs_oracle(rows, F, C, hidden, 32, kw)


STEP3 = dict(step_size=3, gamma=0.3)


def _step3_engine(**kw):
    X, y = make_multiclass(300, 14, 2, DATA_SEED)
    cfg = EngineConfig(max_rounds=12, early_stop=False, rows_per_block=32, **STEP3, **kw)
    return HipRoundEngine(X, y, 2, cfg, None, init_flat([14, 50, 200, 2], INIT_SEED))


def test_graph_replay_across_lr_boundary_bitwise_equals_eager():
    """A captured 4-round graph that holds an LR boundary (rounds 3 and 6 of 8) replays the same
    schedule slots as eager launches: weights and history bit for bit."""
    out = []
    for g in (0, 4):
        e = _step3_engine(graph_rounds=g)
        e.run(8)
        out.append((e.global_flat(), e.history()))
    assert out[0][1]["rounds_run"] == out[1][1]["rounds_run"] == 8
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1]["global"], out[1][1]["global"])
    np.testing.assert_array_equal(out[0][1]["loss"], out[1][1]["loss"])


def test_resume_across_lr_boundary_is_exact(tmp_path):
    """A checkpoint at round 4 (one LR step taken, one to come) resumed into a fresh engine
    continues bit for bit like the uninterrupted run through round 8."""
    from fedmi.ckpt.checkpoint import resume, save_checkpoint
    full = _step3_engine(graph_rounds=0)
    full.run(8)
    a = _step3_engine(graph_rounds=0)
    a.run(4)
    save_checkpoint(str(tmp_path), a)
    b = _step3_engine(graph_rounds=0)
    assert resume(str(tmp_path), b) == 4
    b.run(4)
    hf, hb = full.history(), b.history()
    assert hf["rounds_run"] == hb["rounds_run"] == 8
    np.testing.assert_array_equal(full.global_flat(), b.global_flat())
    np.testing.assert_array_equal(hf["global"], hb["global"])
    np.testing.assert_array_equal(hf["loss"], hb["loss"])


# ---- C: device metric fold, multi-class ----
@pytest.mark.parametrize("C,mode", [(3, "mean"), (16, "mean"), (16, "pooled")])
def test_device_metric_fold_multiclass(C, mode):
    """The device's weighted P/R/F1 fold (fl_device.h metrics_from_cm) is metrics_from_confusion
    of the confusion matrix the evaluation kernel produced, to rounding -- with a class of zero
    support (recall's zero_division) and a class that is never predicted (precision's)."""
    rows = 300 if C == 3 else 400
    X, y = make_multiclass(rows, 14, C, DATA_SEED)
    y = np.where(y == C - 1, 0, y)
    cfg = EngineConfig(hidden=(40,), max_rounds=4, graph_rounds=0, early_stop=False, fused_eval=False, metric_mode=mode)
    # init seed 4 at C = 3: the seeds 1..3 still predict the empty class for a few rows in all of
    # the three rounds (checked on the torch oracle), seed 4 stops doing so in round 1
    e = HipRoundEngine(X, y, C, cfg, None, init_flat([14, 40, C], 4 if C == 3 else INIT_SEED))
    cms = []
    for _ in range(3):
        e.step_train()
        cms.append(e.step_eval())
        e.step_aggregate()
    e.sync_history()
    h = e.history()
    assert h["rounds_run"] == 3
    for r, cm in enumerate(cms):
        assert cm.sum() == rows and cm[C - 1].sum() == 0
        exp = metric_vector(metrics_from_confusion(cm))
        np.testing.assert_allclose(h["per_rank"][r, 0], exp, rtol=0, atol=1e-12)
        np.testing.assert_allclose(h["global"][r], exp, rtol=0, atol=1e-12)
    assert any((cm.sum(0) == 0).any() for cm in cms)
    # not the degenerate all-one-class prediction either
    assert all((cm.sum(0) > 0).sum() >= 2 for cm in cms)


# ---- D: stand-alone confusion kernel ----
@pytest.mark.parametrize("F,C,hidden", [(33, 16, (65,)), (1, 3, (16,))])
def test_confusion_kernel_small_sets(F, C, hidden):
    """fl_confusion on evaluation sets of 1, 31, 32 and 33 rows (around one workgroup of 32):
    every row whose float64 top-2 logit margin is above 1e-5 max|logit| lands in the cell of its
    float64 argmax, and in the fp32 torch oracle's.  The model is trained for 40 rounds first (on
    the oracle): a fresh one predicts one or two classes only."""
    dims = [F, *hidden, C]
    X, y = make_multiclass(300, F, C, DATA_SEED)
    cfg = EngineConfig(hidden=hidden, max_rounds=40, early_stop=False, lr=0.02)
    ref = TorchRoundEngine(X, y, C, cfg, None, init_flat(dims, INIT_SEED))
    ref.run(40)
    flat = ref.global_flat()
    hip = HipRoundEngine(X, y, C, cfg, None, flat)
    preds = set()
    for n in (1, 31, 32, 33):
        Xt, yt = make_multiclass(n, F, C, DATA_SEED + n)
        z = float64_logits(flat, dims, Xt)
        top = np.sort(z, 1)
        unsure = (top[:, -1] - top[:, -2]) < 1e-5 * np.abs(z).max()
        assert unsure.mean() <= 0.01, (n, unsure.sum())
        cm = hip.confusion(Xt, yt, flat=flat)
        assert cm.sum() == n
        sure = np.zeros((C, C), np.int64)
        np.add.at(sure, (yt[~unsure], np.argmax(z, 1)[~unsure]), 1)
        rest = cm - sure  # the unsure rows: anywhere in the row of their own label
        assert (rest >= 0).all(), (n, rest)
        np.testing.assert_array_equal(rest.sum(1), np.bincount(yt[unsure], minlength=C))
        if not unsure.any():
            np.testing.assert_array_equal(cm, ref.confusion(Xt, yt, flat=flat))
        preds |= set(np.flatnonzero(cm.sum(0)).tolist())
    assert len(preds) >= 2, preds


# ---- E: bf16 train kernel gradient, shapes ----
def _check_bf16_train_gradient(rows, F, C, hidden, R, slab):
    """The body of test_hip_engine.test_bf16_train_kernel_gradient at any shape: the slab-reduced
    gradient of one fl_train_bf16 launch vs the float64 host model of the kernel's arithmetic
    (<= 1e-3 per tensor) and vs fp32 autograd (<= 1e-2 per tensor)."""
    dims = [F, *hidden, C]
    X, y = make_multiclass(rows, F, C, DATA_SEED)
    flat = init_flat(dims, INIT_SEED)
    try:
        e = HipRoundEngine(X, y, C, EngineConfig(hidden=hidden, max_rounds=4, early_stop=False, rows_per_block=R,
                                                 dtype="bf16", graph_rounds=0, grad_slab=slab), None, flat)
    except RuntimeError as err:  # split-bf16 layout of a big model at R = 64 exceeds the CU's LDS
        assert "LDS" in str(err) and R == 64
        pytest.skip(str(err))
    assert e.R == R
    e.step_train()
    e.stream.synchronize()
    lay = e.engine.layout()
    assert lay["slab_f16"] == (slab == "fp16") == e.slab_f16
    assert int(lay["n_slabs"]) == (rows + R - 1) // R
    g = e.slab_partials().double().sum(0).cpu().numpy()
    if slab == "fp16":
        g /= len(X)
    ref = _split_bf16_reference_grad(flat, X, y, dims, scaled_delta=slab == "fp32")
    model = TorchRoundEngine(X, y, C, EngineConfig(hidden=hidden, max_rounds=2), None, flat)
    out = model.model(torch.as_tensor(X))
    torch.nn.functional.cross_entropy(out, torch.as_tensor(y, dtype=torch.long)).backward()
    auto = torch.cat([p.grad.reshape(-1) for p in model.model.parameters()]).double().numpy()
    off = 0
    for l in range(len(dims) - 1):
        for n in (dims[l] * dims[l + 1], dims[l + 1]):
            sl = slice(off, off + n)
            err_k = np.linalg.norm(g[sl] - ref[sl]) / np.linalg.norm(ref[sl])
            err_a = np.linalg.norm(g[sl] - auto[sl]) / np.linalg.norm(auto[sl])
            print((rows, F, C, hidden, R, slab), l, n, err_k, err_a)
            assert err_k <= 1e-3, (l, n, err_k)
            assert err_a <= 1e-2, (l, n, err_a)
            off += n


@pytest.mark.parametrize("rows,F,C,hidden,R,slab", BF16_GRAD_CASES)
def test_bf16_train_kernel_gradient_shapes(rows, F, C, hidden, R, slab):
    """C = 3 / 5 / 16 (general CE epilogue of the bf16 body), F = 1, F = 33 / 40 (second bf16
    k-step of layer 0), a 5-row shard and R + 1 rows, on both slab formats."""
    _check_bf16_train_gradient(rows, F, C, hidden, R, slab)


# ---- F: bf16 engine vs oracle, multi-class and weight decay ----
@pytest.mark.parametrize("C,kw", BF16_TRACK_CASES, ids=["C3", "C2-weight_decay"])
def test_bf16_engine_tracks_fp32_oracle_multiclass_and_weight_decay(C, kw):
    """test_bf16_engine_tracks_fp32_oracle's assertions with three classes, and with two classes
    and weight decay: first-step update signs agree, final accuracy and loss within 0.02 after 60
    rounds.  3000 rows: on 600 the fp32 oracle's own final accuracy moves by more than 0.01
    between init seeds (tests/test_oracle_noise.py), which would make the 0.02 bound meaningless."""
    X, y = make_multiclass(BF16_TRACK_ROWS, 14, C, DATA_SEED)
    flat = init_flat([14, 50, 200, C], 3)
    mk = lambda cls, **k: cls(X, y, C, EngineConfig(max_rounds=60, early_stop=False, **kw, **k), None, flat)
    hb = mk(HipRoundEngine, dtype="bf16")
    ref = mk(TorchRoundEngine)
    hb.run(1)
    ref.run(1)
    upd_b, upd_r = hb.global_flat() - flat, ref.global_flat() - flat
    agree = np.mean(np.sign(upd_b) == np.sign(upd_r))
    assert agree > 0.97, agree
    hb.run(59)
    ref.run(59)
    acc_b, acc_r = hb.history()["global"][:, 0], ref.history()["global"][:, 0]
    print(C, kw, agree, acc_b[-1], acc_r[-1], hb.history()["loss"][-1], ref.history()["loss"][-1])
    assert abs(acc_b[-1] - acc_r[-1]) < 0.02, (acc_b[-1], acc_r[-1])
    assert abs(hb.history()["loss"][-1] - ref.history()["loss"][-1]) < 0.02

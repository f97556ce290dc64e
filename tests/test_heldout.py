"""Held-out scoring of the global model inside the round (fedmi/ops/csrc/fl_heldout.hip) and the row-wise
inference API, on the GPU.

The row kernel's counts must be the existing scoring exactly (``confusion`` of the global weights after
each round, on a twin that never heard of a held-out set), its loss a float64 log-sum-exp forward of the
same fp32 weights, and nothing else of a run may move: weights, metrics, loss history and stop round
are compared bitwise with the twin's.

Probabilities: the largest |predict_proba - float64 softmax of the same fp32 weights| observed on the
MI355X for the shapes and seeds below is written at PROBA_OBSERVED (and in
profiles/heldout_trace.jsonl); the bound is 8 x that (headroom for other seeds), capped at 1e-4.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.data.synthetic import make_income_like
from fedmi.fl.engine import EngineConfig, HipRoundEngine, heldout_metrics
from fedmi.fl.metrics import confusion_matrix
from fedmi.fl.simulate import ClientGroup
from fedmi.models.mlp import dense_to_image, init_flat

from .reference_oracle import float64_logits, make_multiclass

pytestmark = pytest.mark.gpu

MODELS = {"income": [14, 50, 200, 2], "odd": [5, 7, 3], "deep": [6, 9, 4, 3]}
ROUNDS = 6
# largest |proba - float64 softmax| seen on the MI355X over test_predict_matches_float64_softmax's cases
PROBA_OBSERVED = 7.9e-8
PROBA_BOUND = min(8 * PROBA_OBSERVED, 1e-4)


def _data(name, n, seed):
    dims = MODELS[name]
    X, y = make_multiclass(n, dims[0], dims[-1], seed)
    return np.ascontiguousarray(X, np.float32), np.asarray(y).astype(np.int64)


def _cfg(name, **kw):
    kw.setdefault("max_rounds", 12)
    return EngineConfig(hidden=tuple(MODELS[name][1:-1]), **kw)


def _engine(name, cfg, n_train=150, seed=3):
    X, y = _data(name, n_train, seed)
    return HipRoundEngine(X, y, MODELS[name][-1], cfg, None, init_flat(MODELS[name], 1))


def _z64(flat, dims, X) -> torch.Tensor:
    return torch.as_tensor(np.asarray(float64_logits(flat, dims, X), np.float64))


def _ce64(flat, dims, X, y):
    """Mean softmax cross-entropy of the dense fp32 weights ``flat``, every operation in float64."""
    z = _z64(flat, dims, X)
    return float((torch.logsumexp(z, 1) - z.gather(1, torch.as_tensor(y).view(-1, 1)).squeeze(1)).mean())


_TWINS = {}


def _twin(name, rpb, dtype, n_val):
    """(history and final weights of engine A, which scores the held-out set in ONE run(); per-round
    confusion counts and float64 losses of twin B, which has no held-out set, runs one round at a time
    and is scored with the existing ``confusion`` after each).  Computed once per case."""
    key = (name, rpb, dtype, n_val)
    if key not in _TWINS:
        Xv, yv = _data(name, n_val, 11)
        cfg = _cfg(name, rows_per_block=rpb, dtype=dtype)
        a = _engine(name, cfg)
        a.set_heldout(Xv, yv, keep_best=True)
        a.run(ROUNDS)
        b = _engine(name, cfg)
        cms, losses, flats = [], [], []
        for _ in range(ROUNDS):
            b.run(1)
            g = b.global_flat()
            flats.append(g)
            cms.append(b.confusion(Xv, yv, flat=g))
            losses.append(_ce64(g, MODELS[name], Xv, yv))
        _TWINS[key] = dict(a=a, ha=a.history(), b=b, hb=b.history(), cms=np.stack(cms), losses=np.asarray(losses),
                           flats=flats)
    return _TWINS[key]


CASES = [(m, rpb, dt, nv) for m in MODELS for rpb in (16, 32) for dt in ("fp32", "bf16") for nv in (1, 17, 33, 100)]


# ---- 1. rows are the existing scoring, and nothing else moves ----
@pytest.mark.parametrize("name,rpb,dtype,n_val", CASES)
def test_rows_are_the_existing_scoring_and_nothing_else_moves(name, rpb, dtype, n_val):
    t = _twin(name, rpb, dtype, n_val)
    ha, hb = t["ha"], t["hb"]
    assert ha["rounds_run"] == hb["rounds_run"] == ROUNDS
    assert ha["heldout_cm"].dtype == np.int64 and ha["heldout_cm"].shape == (ROUNDS,) + (MODELS[name][-1],) * 2
    np.testing.assert_array_equal(ha["heldout_cm"], t["cms"])
    assert (ha["heldout_cm"].sum((1, 2)) == n_val).all()
    np.testing.assert_array_equal(t["a"].global_flat(), t["b"].global_flat())
    np.testing.assert_array_equal(t["a"].local_flat(), t["b"].local_flat())
    for k in ("global", "per_rank", "loss"):
        np.testing.assert_array_equal(ha[k], hb[k], err_msg=k)
    assert ha["stop_round"] == hb["stop_round"] and ha["stop_trigger"] == hb["stop_trigger"]
    assert "heldout_cm" not in hb and set(ha) - set(hb) == {"heldout_cm", "heldout_loss", "heldout_loss_sum",
                                                            "heldout_best_round"}
    assert heldout_metrics(ha).shape == (ROUNDS, 4)
    np.testing.assert_allclose(heldout_metrics(ha)[:, 0], t["cms"].trace(axis1=1, axis2=2) / n_val)


# ---- 2. loss ----
@pytest.mark.parametrize("name,rpb,dtype,n_val", CASES)
def test_loss_matches_float64_forward(name, rpb, dtype, n_val):
    """rtol 1e-4: the project's bound for the fp32 loss (tests/test_hip_engine.py)."""
    t = _twin(name, rpb, dtype, n_val)
    got = t["ha"]["heldout_loss"]
    print(name, rpb, dtype, n_val, "max rel", float(np.max(np.abs(got - t["losses"]) / t["losses"])))
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, t["losses"], rtol=1e-4)
    np.testing.assert_array_equal(got, t["ha"]["heldout_loss_sum"].astype(np.float64) / n_val)


# ---- 4. best round (on the same twins) ----
@pytest.mark.parametrize("name,rpb,dtype,n_val", [c for c in CASES if c[3] in (17, 100)])
def test_best_round_is_the_first_argmin_and_its_model_is_kept(name, rpb, dtype, n_val):
    t = _twin(name, rpb, dtype, n_val)
    sums = t["ha"]["heldout_loss_sum"]
    best = int(np.argmin(sums))    # (the first of equal minima)
    assert t["ha"]["heldout_best_round"] == best
    np.testing.assert_array_equal(t["a"].best_flat(), t["flats"][best])


def test_best_flat_raises_without_keep_best_or_before_a_win():
    Xv, yv = _data("odd", 17, 11)
    e = _engine("odd", _cfg("odd"))
    with pytest.raises(RuntimeError, match="keep_best"):
        e.best_flat()
    e.set_heldout(Xv, yv)
    e.run(1)
    with pytest.raises(RuntimeError, match="keep_best"):
        e.best_flat()
    f = _engine("odd", _cfg("odd"))
    f.set_heldout(Xv, yv, keep_best=True)
    with pytest.raises(RuntimeError, match="no round has won"):
        f.best_flat()
    assert f.history()["heldout_best_round"] == -1


def test_nan_aggregate_never_wins_in_a_client_group():
    """A tampered group whose aggregate is NaN from round 2 on: NaN loss rows from there, the best round
    is one of the first two and its kept model is finite."""
    name = "deep"
    X, y = _data(name, 240, 3)
    Xv, yv = _data(name, 33, 11)
    Pimg = len(dense_to_image(init_flat(MODELS[name], 0), MODELS[name]))

    def tamper(r, bufs):
        if r >= 2:
            for b in bufs:
                b[:Pimg] = float("nan")

    g = ClientGroup(X, y, 3, _cfg(name, early_stop=False), backend="hip", shard_mode="iid", tamper=tamper,
                    heldout=(Xv, yv), keep_best=True)
    g.run(5)
    h = g.history()
    assert h["rounds_run"] == 5
    assert np.isfinite(h["heldout_loss"][:2]).all() and np.isnan(h["heldout_loss"][2:]).all()
    assert 0 <= h["heldout_best_round"] <= 1
    assert np.isfinite(g.best_flat()).all() and not np.isfinite(g.global_flat()).all()
    assert (h["heldout_cm"][2:, :, 1:] == 0).all()   # NaN logits: the first-maximum rule answers class 0


# ---- 3. determinism and capture ----
def _run_income(graph_rounds, rounds, **kw):
    X, y = make_income_like(2000, seed=7)
    Xv, yv = make_income_like(333, seed=8)
    cfg = EngineConfig(graph_rounds=graph_rounds, **kw)
    e = HipRoundEngine(X, y, 2, cfg, None, init_flat(MODELS["income"], 9))
    e.set_heldout(Xv, yv, keep_best=True)
    e.run(rounds)
    return e, e.history()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_runs_and_graph_replays_are_bit_identical(dtype):
    kw = dict(max_rounds=20, early_stop=False, dtype=dtype)
    (e0, h0), (e1, h1), (e2, h2) = _run_income(4, 13, **kw), _run_income(4, 13, **kw), _run_income(0, 13, **kw)
    assert e0.engine.graph_captures >= 1 and e2.engine.graph_captures == 0
    for h in (h1, h2):
        np.testing.assert_array_equal(h["heldout_cm"], h0["heldout_cm"])
        np.testing.assert_array_equal(h["heldout_loss_sum"].view(np.uint32), h0["heldout_loss_sum"].view(np.uint32))
        assert h["heldout_best_round"] == h0["heldout_best_round"]
    np.testing.assert_array_equal(e0.best_flat(), e2.best_flat())
    assert h0["rounds_run"] == 13 and (h0["heldout_cm"].sum((1, 2)) == 333).all()


def test_streaming_run_reports_the_same_rows():
    """run_streaming (the console path) mirrors the held-out buffers chunk by chunk: every history it hands
    out has one row per finished round, and the run ends with run()'s rows."""
    kw = dict(max_rounds=20, early_stop=False)
    e0, h0 = _run_income(4, 13, **kw)
    X, y = make_income_like(2000, seed=7)
    Xv, yv = make_income_like(333, seed=8)
    e = HipRoundEngine(X, y, 2, EngineConfig(graph_rounds=4, **kw), None, init_flat(MODELS["income"], 9))
    e.set_heldout(Xv, yv, keep_best=True)
    seen = []
    e.run_streaming(13, chunk=4, on_history=lambda h: seen.append((h["rounds_run"], len(h["heldout_cm"]),
                                                                   h["heldout_cm"].sum())))
    assert seen and all(n == rows and total == 333 * n for n, rows, total in seen) and seen[-1][0] == 13
    h = e.history()
    np.testing.assert_array_equal(h["heldout_cm"], h0["heldout_cm"])
    np.testing.assert_array_equal(h["heldout_loss_sum"], h0["heldout_loss_sum"])
    assert h["heldout_best_round"] == h0["heldout_best_round"]


def test_early_stop_leaves_no_row_past_the_stop():
    e, h = _run_income(4, 80, max_rounds=80, patience=4, tolerance=1e-3)
    n = h["rounds_run"]
    assert 0 < h["stop_round"] < 80 and 0 < n < 80, (h["stop_round"], n)
    assert len(h["heldout_cm"]) == len(h["heldout_loss"]) == n
    assert (h["heldout_cm"].sum((1, 2)) == 333).all()
    # the device history past the stop was never written
    assert int(e.ho_cm[n * 4:].abs().sum()) == 0 and float(e.ho_loss[n:].abs().sum()) == 0.0
    assert 0 <= h["heldout_best_round"] < n
    # ... and the rounds before it are the run's without a held-out set
    X, y = make_income_like(2000, seed=7)
    b = HipRoundEngine(X, y, 2, EngineConfig(graph_rounds=4, max_rounds=80, patience=4, tolerance=1e-3), None,
                       init_flat(MODELS["income"], 9))
    b.run(80)
    assert b.history()["stop_round"] == h["stop_round"]
    np.testing.assert_array_equal(b.global_flat(), e.global_flat())


def test_set_heldout_between_runs_and_checkpoint_continue(tmp_path):
    from fedmi.ckpt.checkpoint import resume, save_checkpoint
    name = "odd"
    Xv, yv = _data(name, 33, 11)

    def mk():
        e = _engine(name, _cfg(name, early_stop=False, graph_rounds=2))
        e.set_heldout(Xv, yv, keep_best=True)
        return e

    full = mk()
    full.run(8)
    a = mk()
    a.run(3)
    save_checkpoint(str(tmp_path / "c"), a)
    b = mk()
    assert resume(str(tmp_path / "c"), b) == 3
    b.run(5)
    hf, hb = full.history(), b.history()
    np.testing.assert_array_equal(hf["heldout_cm"], hb["heldout_cm"])
    np.testing.assert_array_equal(hf["heldout_loss_sum"], hb["heldout_loss_sum"])
    assert hf["heldout_best_round"] == hb["heldout_best_round"]
    np.testing.assert_array_equal(full.best_flat(), b.best_flat())
    with pytest.raises(ValueError, match="held-out"):
        resume(str(tmp_path / "c"), _engine(name, _cfg(name, early_stop=False)))
    # between run() calls: rounds before the call have all-zero rows, later ones are scored
    c = _engine(name, _cfg(name, early_stop=False, graph_rounds=2))
    c.run(4)
    c.set_heldout(Xv, yv)
    c.run(4)
    hc = c.history()
    assert (hc["heldout_cm"][:4] == 0).all()
    np.testing.assert_array_equal(hc["heldout_cm"][4:], hf["heldout_cm"][4:])
    np.testing.assert_array_equal(c.global_flat(), full.global_flat())


# ---- 5. composition in a client group ----
@pytest.mark.parametrize("kw,flip", [
    (dict(server_opt="adam"), False),
    (dict(aggregator="median"), True),
    (dict(secagg=True), False),
    (dict(dp_clip=0.2, dp_noise=1.0, dp_seed=1), False),
    (dict(participation=0.67), False),
], ids=["server_adam", "median_signflip", "secagg", "dp", "participation"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_rows_follow_every_aggregation_family_in_a_client_group(kw, flip, dtype):
    name = "deep"
    X, y = _data(name, 300, 3)
    Xv, yv = _data(name, 100, 11)
    Pimg = len(dense_to_image(init_flat(MODELS[name], 0), MODELS[name]))

    def sign_flip(r, bufs):   # client 2 sends the negative of its model
        bufs[2][:Pimg].neg_()

    g = ClientGroup(X, y, 3, _cfg(name, early_stop=False, dtype=dtype, **kw), backend="hip", shard_mode="iid",
                    tamper=sign_flip if flip else None, heldout=(Xv, yv))
    for r in range(3):
        assert g.run(1) == 1
        want = g.clients[0].confusion(Xv, yv, flat=g.global_flat())
        h = g.history()
        assert h["rounds_run"] == r + 1
        np.testing.assert_array_equal(h["heldout_cm"][r], want)
        assert h["heldout_cm"][r].sum() == 100
        np.testing.assert_allclose(h["heldout_loss"][r], _ce64(g.global_flat(), MODELS[name], Xv, yv), rtol=1e-4)


# ---- 6. inference ----
@pytest.fixture(scope="module")
def trained():
    out = {}
    for name in MODELS:
        e = _engine(name, _cfg(name, early_stop=False))
        e.run(3)
        out[name] = e
    return out


@pytest.mark.parametrize("n", [1, 17, 1000])
@pytest.mark.parametrize("name", list(MODELS))
def test_predict_matches_float64_softmax(trained, name, n):
    e = trained[name]
    C = MODELS[name][-1]
    X, y = _data(name, n, 21)
    worst = 0.0
    for which, flat in (("global", e.global_flat()), ("local", e.local_flat())):
        p = e.predict_proba(X, which=which)
        assert p.shape == (n, C) and p.dtype == np.float32
        assert np.abs(p.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
        z = _z64(flat, MODELS[name], X)
        dev = float(np.abs(p - torch.softmax(z, 1).numpy()).max())
        worst = max(worst, dev)
        pred = e.predict(X, which=which)
        assert pred.shape == (n,) and pred.dtype == np.int64
        np.testing.assert_array_equal(confusion_matrix(y, pred, C), e.confusion(X, y, flat=flat))
        # the prediction is the row's largest probability (ties aside: none of these rows has one)
        top = np.sort(p, 1)
        if (top[:, -1] > top[:, -2]).all():
            np.testing.assert_array_equal(pred, p.argmax(1))
    print(name, n, "max |proba - float64 softmax|", worst, "bound", PROBA_BOUND)
    assert worst <= PROBA_BOUND


def test_local_and_global_models_are_told_apart():
    """In a client group the lead's local model is not the global one: which= picks the image."""
    name = "odd"
    X, y = _data(name, 240, 3)
    Xq, _ = _data(name, 50, 21)
    g = ClientGroup(X, y, 3, _cfg(name, early_stop=False), backend="hip", shard_mode="iid")
    g.run(2)
    e = g.clients[0]
    assert not np.array_equal(e.global_flat(), e.local_flat())
    for which, flat in (("global", e.global_flat()), ("local", e.local_flat())):
        want = torch.softmax(_z64(flat, MODELS[name], Xq), 1).numpy()
        assert np.abs(e.predict_proba(Xq, which=which) - want).max() <= PROBA_BOUND
    assert np.abs(e.predict_proba(Xq, which="global") - e.predict_proba(Xq, which="local")).max() > 1e-4
    with pytest.raises(ValueError, match="which"):
        e.predict(Xq, which="server")
    with pytest.raises(ValueError, match=r"\[n, 5\]"):
        e.predict(np.zeros((3, 4), np.float32))


@pytest.mark.parametrize("name", list(MODELS))
def test_all_zero_model_predicts_class_0_with_equal_probabilities(name):
    e = _engine(name, _cfg(name))
    e.set_global_flat(np.zeros(e.P, np.float32))
    X, _ = _data(name, 37, 21)
    C = MODELS[name][-1]
    np.testing.assert_array_equal(e.predict(X), np.zeros(37, np.int64))
    np.testing.assert_array_equal(e.predict_proba(X), np.full((37, C), np.float32(1.0) / np.float32(C)))
    assert e.predict(np.zeros((0, MODELS[name][0]), np.float32)).shape == (0,)


def test_refusals_on_the_gpu():
    name = "odd"
    X, y = _data(name, 64, 3)
    e = _engine(name, _cfg(name))
    for bad_X, bad_y, msg in ((X[:, :4], y, "held-out X"), (X, y[:-1], "held-out y"), (X, y + 2, "labels"),
                              (X, y.astype(np.float32), "integers"), (X[:0], y[:0], "rows")):
        with pytest.raises(ValueError, match=msg):
            e.set_heldout(bad_X, bad_y)
    assert not e.heldout and "heldout_cm" not in e.history()
    from fedmi.fl.engine import comm_len
    bufs = [torch.zeros(comm_len(MODELS[name], 1), device="cuda") for _ in range(2)]
    p = HipRoundEngine(X, y, 3, _cfg(name), None, init_flat(MODELS[name], 1), comm_buffers=bufs)
    with pytest.raises(ValueError, match="trial packing"):
        p.set_heldout(X, y)
    e.set_heldout(X, y)
    with pytest.raises(RuntimeError, match="held-out"):
        e.m.TrialBatch([e.engine])


# ---- 7. two ranks sharing the GPU ----
WORLD = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shared():
    name = "deep"
    X, y = _data(name, 400, 3)
    Xv, yv = _data(name, 100, 11)
    return name, X, y, Xv, yv


def _worker(rank, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(WORLD), LOCAL_RANK="0",
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    try:
        from fedmi.data.sharding import shard_indices
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="xgmi", device="cuda:0", rccl=False)
        comm.peer_allreduce = True
        name, X, y, Xv, yv = _shared()
        idx = shard_indices(len(X), rank, WORLD, mode="iid", seed=0, labels=y, alpha=0.5)
        res = {}
        for dtype in ("fp32", "bf16"):
            cfg = _cfg(name, early_stop=False, graph_rounds=2, dtype=dtype)
            e = HipRoundEngine(X[idx], y[idx], 3, cfg, comm, init_flat(MODELS[name], rank))
            assert e.aggregation.startswith("xgmi-oneshot"), e.aggregation
            e.set_heldout(Xv, yv, keep_best=True)
            assert not e.engine.lagged   # (bf16: lagged by default; never with a held-out set)
            e.run(4)
            h = e.history()
            res[dtype] = dict(cm=h["heldout_cm"], loss=h["heldout_loss_sum"], best=h["heldout_best_round"],
                              flat=e.global_flat(), best_flat=e.best_flat(), captures=int(e.engine.graph_captures),
                              own=e.confusion(Xv, yv, flat=e.global_flat()))
        torch.cuda.synchronize()
        comm.Barrier()
        q.put((rank, res, None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_two_ranks_sharing_the_gpu_report_the_group_rows():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=110) for _ in range(WORLD)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=30)
    for rank, res, err in out:
        assert err is None, f"rank {rank}:\n{err}"
    name, X, y, Xv, yv = _shared()
    for dtype in ("fp32", "bf16"):
        r0, r1 = out[0][1][dtype], out[1][1][dtype]
        for k in ("cm", "loss", "flat", "best_flat"):
            np.testing.assert_array_equal(r0[k], r1[k], err_msg=f"{dtype} {k}")
        assert r0["best"] == r1["best"] and r0["captures"] >= 1
        np.testing.assert_array_equal(r0["cm"][-1], r0["own"])
        g = ClientGroup(X, y, WORLD, _cfg(name, early_stop=False, dtype=dtype), backend="hip", shard_mode="iid",
                        seed=0, heldout=(Xv, yv), keep_best=True)
        g.run(4)
        h = g.history()
        np.testing.assert_array_equal(r0["cm"], h["heldout_cm"], err_msg=dtype)
        np.testing.assert_array_equal(r0["loss"], h["heldout_loss_sum"], err_msg=dtype)
        assert r0["best"] == h["heldout_best_round"]
        np.testing.assert_array_equal(r0["flat"], g.global_flat(), err_msg=dtype)
    for p in procs:
        assert p.exitcode == 0

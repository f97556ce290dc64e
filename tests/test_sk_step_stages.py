"""The float64 sklearn step kernels stage by stage against the longdouble host model
(sk_step_oracle.py): mlp_fused_f64.hip (skf_rowpass, skf_cs_fwd, skf_cs_bwd, skf_wgrad_adam) and,
under FEDMI_SK_FUSED=0, mlp_f64.hip (gemm_f64, gather_rows_f64, xent_f64, colsum_f64, adam_f64).

Harness: estimators built by hand with seeded weights that differ per trial, ``_fit_hip_prepare``
for the job and its device buffers, ``xb`` / ``acts`` / ``deltas`` pre-filled with NaN, then one
graph-replayed epoch at a time (``job.tr.run(1, stream, 1, True)``: the production path) with every
buffer read back after it.  With n <= B an epoch is one step, so every intermediate of that step is
in memory: gathered rows, activations, deltas, moments, weights, the transposed weight copy, the
step counter and the epoch loss are each held to the model's bound ON THE DEVICE'S OWN INPUTS OF
THAT STAGE (sk_step_oracle.check_step; the bounds are derived from the operands, never measured),
no element left out; every element of ``acts`` / ``deltas`` past a layer's width or in a row the
step did not own keeps its NaN bits.  Three epochs per case: Adam t = 1..3.

Cases (sk_step_oracle.CASES): F = 1 and width 1; chunk lengths 4 / 8 / 16; widths 16, 17, 272;
narrow softmax C = 3; the wide head on the matrix cores C = 5, 9, 16; forward k-splits; four
layers; C = 17 (must fall back to the layered path); the tile split with one tile per slice and
with a one-column last tile; the [S] shape.  Every fused case again on the layered path, every
tile-split case again unsplit.  Then: an epoch of a 16-row and a 1-row step; an inactive trial
inside a packed job; packed trials that stop at different epochs against the numpy backend.

Measured on MI355X, worst error / bound over all cases and epochs (the requirement is <= 1), fused
kernels / layered kernels: gather 0 / 0, forward 0.17 / 0.17, head 0.040 / 0.12, backward 0.18 /
0.18, gradient 0.33 / 0.29, m 0.33 / 0.47, v 0.44 / 0.47, params 0.18 / 0.18, epoch loss 0.026 /
0.034; wt bit-equal in every case.  Every test printed its own figures (``STAGES ...`` with -s)."""
import numpy as np
import pytest
import torch

from fedmi.models.sklearn_mlp import MLPClassifier, _fit_hip_prepare, fit_packed

from . import sk_step_oracle as so

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not so.HAVE_LONGDOUBLE, reason="numpy longdouble has no 64-bit mantissa here")]

NAN_BUFS = ("xb", "acts", "deltas")
STATE = ("params", "m", "v", "step", "wt", "loss_acc", "xb", "acts", "deltas", "grads", "curve", "active", "n_iter")
# expected (fused, split) of the default path
SPLIT = {(14, 32, 32, 1): 2, (20, 33, 17, 3): 2, (14, 50, 400, 1): 4}
WORST = {}


def _env(monkeypatch, mode):
    for k in ("FEDMI_SK_FUSED", "FEDMI_SK_SPLIT", "FEDMI_SK_WT", "FEDMI_SK_WTHRU", "FEDMI_SK_STAMPS"):
        monkeypatch.delenv(k, raising=False)
    if mode == "layered":
        monkeypatch.setenv("FEDMI_SK_FUSED", "0")
    if mode == "unsplit":
        monkeypatch.setenv("FEDMI_SK_SPLIT", "1")


class Job:
    """A packed job of hand-built estimators, driven one epoch at a time."""

    def __init__(self, dims, X, y, perms, ps, lrs, batch, mode, inactive=(), m=None, v=None, step=None):
        self.dims, self.X, self.y, self.perms, self.mode = tuple(dims), X, y, perms, mode
        self.T, self.n, self.L = len(ps), len(X), len(dims) - 1
        self.lrs = list(lrs[:self.T])
        ests = so.make_estimators(dims, ps, self.lrs, batch, "hip", max_iter=len(perms))
        self.B = ests[0]._batch(self.n)
        self.job = _fit_hip_prepare(ests, X, y, list(dims), perms, incremental=False)
        self.fused, self.split = ests[0]._hip_fused, ests[0]._hip_split
        b = self.job.bufs_t
        for k in NAN_BUFS:
            b[k].fill_(float("nan"))
        for t in inactive:
            b["active"][t] = 0
        if m is not None:
            b["m"].copy_(torch.as_tensor(m)), b["v"].copy_(torch.as_tensor(v)), b["step"].copy_(torch.as_tensor(step))
        torch.cuda.synchronize()
        self.epoch = 0

    def snap(self):
        torch.cuda.synchronize()
        return {k: self.job.bufs_t[k].cpu().numpy().copy() for k in STATE if k in self.job.bufs_t}

    def run_epoch(self):
        assert self.job.tr.run(1, self.job.stream.cuda_stream, 1, True) == 1
        self.job.stream.synchronize()
        self.epoch += 1

    def obs(self, s, tr, r0, rows):
        """Trial tr's stage values of rows [r0, r0 + rows) of the last step, from snapshot s."""
        d, L, B = self.dims, self.L, self.B
        if self.fused:
            xb = s["xb"][tr, r0:r0 + rows]
        else:   # one [B][F] block shared by the trials
            xb = s["xb"].reshape(-1)[:B * d[0]].reshape(B, d[0])[r0:r0 + rows]
        o = {"xb": xb, "acts": [s["acts"][l, tr, r0:r0 + rows, :d[l + 1]] for l in range(L - 1)],
             "deltas": [s["deltas"][l, tr, r0:r0 + rows, :d[l + 1]] for l in range(L)],
             "p": s["params"][tr], "m": s["m"][tr], "v": s["v"][tr]}
        if self.fused:
            o["wt"] = s["wt"][tr]
        else:
            o["logits"] = s["acts"][L - 1, tr, r0:r0 + rows, :d[L]]
            o["grads"] = s["grads"][tr]
        return o

    def owned(self, s, rows, trials):
        """Masks of the elements of acts / deltas / xb that a step of `rows` rows of `trials` owns."""
        d, L = self.dims, self.L
        acts, deltas, xb = (np.zeros(s[k].shape, bool) for k in ("acts", "deltas", "xb"))
        for tr in trials:
            for l in range(L):
                deltas[l, tr, :rows, :d[l + 1]] = True
                if l < L - 1 or not self.fused:
                    acts[l, tr, :rows, :d[l + 1]] = True
            if self.fused:
                xb[tr, :rows] = True
        if not self.fused:
            xb.reshape(-1)[:rows * d[0]] = True
        return {"acts": acts, "deltas": deltas, "xb": xb}


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def assert_kept(what, before, after, keys, where=None):
    for k in keys:
        if k not in before:
            continue
        same = bits(before[k]) == bits(after[k])
        w = np.ones(same.shape, bool) if where is None or k not in where else where[k]
        bad = ~same & w
        assert not bad.any(), f"{what}: {k} changed at {np.argwhere(bad)[:4].tolist()} ({int(bad.sum())} elements)"


def check_epoch_loss(what, job, tr, e, got, model_sums, model_bounds, sqs, rows_l, worst):
    ref = so.epoch_loss(model_sums, sqs, so.ALPHA, job.n)
    bnd = so.loss_bound(rows_l, job.dims, so.ALPHA, sum(abs(x) for x in model_sums), sum(model_bounds), sum(sqs)) / job.n
    so._worst(f"{what} epoch loss", np.float64(got), ref, bnd, worst, "loss")


def run_stage_epochs(job, what, trials, worst):
    """Three one-step epochs of `job`; every active trial's every stage against the model."""
    assert job.n <= job.B
    kind = so.kind_of(job.dims)
    s0 = job.snap()
    nan_bits = {k: bits(s0[k]) for k in NAN_BUFS}
    for k in NAN_BUFS:
        assert np.isnan(s0[k]).all()
    for e in range(so.EPOCHS):
        job.run_epoch()
        s1 = job.snap()
        t = e + 1
        own = job.owned(s1, job.n, trials)
        for k in NAN_BUFS:   # what the step does not own keeps its NaN bits
            bad = (bits(s1[k]) != nan_bits[k]) & ~own[k]
            assert not bad.any(), f"{what} epoch {e}: {k} written outside the step's rows / widths at " \
                                  f"{np.argwhere(bad)[:4].tolist()} ({int(bad.sum())} elements)"
        for tr in trials:
            w = f"{what} trial {tr} epoch {e}"
            assert int(s1["step"][tr]) == t, (w, s1["step"])
            before = {"p": s0["params"][tr], "m": s0["m"][tr], "v": s0["v"][tr]}
            _, ml, mb, sq = so.check_step(w, job.X, job.y, job.perms[e], 0, job.n, job.dims, kind, so.ALPHA, job.lrs[tr], t,
                                          before, job.obs(s1, tr, 0, job.n), worst)
            check_epoch_loss(w, job, tr, e, s1["curve"][tr, e], [ml], [mb], [sq], [job.n], worst)
            assert int(s1["n_iter"][tr]) == t and s1["loss_acc"][tr] == 0.0
        s0 = s1
    return s0


def modes_of(case):
    dims = case[0]
    if dims[-1] > 16:
        return ["default"]
    return ["default", "layered"] + (["unsplit"] if dims in SPLIT else [])


def expect_path(job, mode):
    dims = job.dims
    if mode == "layered" or dims[-1] > 16:
        assert not job.fused and job.split == 1, (dims, mode, job.fused, job.split)
    elif mode == "unsplit" or dims not in SPLIT:
        assert job.fused and job.split == 1, (dims, mode, job.fused, job.split)
    else:
        assert job.fused and job.split == SPLIT[dims] >= 2, (dims, mode, job.fused, job.split)


def report(what, worst):
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("STAGES", what, {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("case,mode", [(c, m) for c in so.CASES for m in modes_of(c)],
                         ids=lambda x: so.case_id(x) if isinstance(x, tuple) else x)
def test_step_stages_match_the_host_model(case, mode, monkeypatch):
    dims, n, batch, T = case
    _env(monkeypatch, mode)
    X, y, perms, ps = so.make_case(dims, n, T)
    job = Job(dims, X, y, perms, ps, so.LRS, batch, mode)
    expect_path(job, mode)
    what = f"{so.case_id(case)} {mode}"
    worst = {}
    run_stage_epochs(job, what, range(T), worst)
    want = {"gather", "forward", "head", "gradient", "m", "v", "params", "loss"} | ({"wt"} if job.fused else set()) | \
        ({"backward"} if len(dims) > 2 else set())
    assert set(worst) == want, (set(worst), want)
    report(what, worst)


@pytest.mark.parametrize("mode", ["default", "layered"])
@pytest.mark.parametrize("case", so.CASES_B1, ids=so.case_id)
def test_epoch_of_a_full_and_a_one_row_step(case, mode, monkeypatch):
    """batch_size 16, 17 rows: the second step of every epoch has one row (three of the four wgrad
    waves without rows, a row block of one row).  The first step of each epoch is established by a
    second job -- the 16 rows alone, started from the main job's weights, moments and step counter
    -- which gets the full stage check itself (non-zero moments) and must leave rows 1..15 of the
    main job's activations and deltas bit for bit; the main job's one-row step is then checked stage
    by stage from that state, and the epoch loss over both steps."""
    dims, n, batch, T = case
    _env(monkeypatch, mode)
    X, y, perms, ps = so.make_case(dims, n, T)
    main = Job(dims, X, y, perms, ps, so.LRS, batch, mode)
    expect_path(main, mode)
    assert main.B == 16 == n - 1
    kind = so.kind_of(dims)
    what = f"{so.case_id(case)} {mode}"
    worst = {}
    s0 = main.snap()
    nanb = bits(s0["acts"]).flat[0]
    assert np.isnan(s0["acts"]).all() and np.isnan(s0["deltas"]).all()
    for e in range(so.EPOCHS):
        idx = perms[e][:16]
        first = Job(dims, X[idx], y[idx], np.arange(16, dtype=np.int32)[None], s0["params"], so.LRS, batch, mode,
                    m=s0["m"], v=s0["v"], step=s0["step"])
        f0 = first.snap()
        # (the layered path does not keep the transposed copy)
        assert_kept(what, s0, f0, ("params", "m", "v", "step") + (("wt",) if main.fused else ()))
        first.run_epoch()
        f1 = first.snap()
        main.run_epoch()
        s1 = main.snap()
        for k in ("acts", "deltas"):   # rows 1..15: the 16-row step's values; row 0: the one-row step's
            a, b = bits(s1[k])[:, :, 1:], bits(f1[k])[:, :, 1:]
            assert (a == b).all(), f"{what} epoch {e}: {k} rows 1..15 are not the first step's"
        own = main.owned(s1, 16, range(T))
        for k in ("acts", "deltas"):
            assert (bits(s1[k])[~own[k]] == nanb).all(), f"{what} epoch {e}: {k} written outside the rows / widths"
        for tr in range(T):
            w = f"{what} trial {tr} epoch {e}"
            assert int(f1["step"][tr]) == 2 * e + 1 and int(s1["step"][tr]) == 2 * e + 2, (w, f1["step"], s1["step"])
            before = {"p": s0["params"][tr], "m": s0["m"][tr], "v": s0["v"][tr]}
            _, l1, b1, q1 = so.check_step(w + " rows 0+16", first.X, first.y, first.perms[0], 0, 16, dims, kind, so.ALPHA,
                                          so.LRS[tr], 2 * e + 1, before, first.obs(f1, tr, 0, 16), worst)
            mid = {"p": f1["params"][tr], "m": f1["m"][tr], "v": f1["v"][tr]}
            _, l2, b2, q2 = so.check_step(w + " rows 16+1", X, y, perms[e], 16, 1, dims, kind, so.ALPHA, so.LRS[tr],
                                          2 * e + 2, mid, main.obs(s1, tr, 0, 1), worst)
            check_epoch_loss(w, main, tr, e, s1["curve"][tr, e], [l1, l2], [b1, b2], [q1, q2], [16, 1], worst)
        s0 = s1
    report(what, worst)


@pytest.mark.parametrize("mode", ["default", "layered"])
@pytest.mark.parametrize("dims,n", [((33, 17, 15, 5), 40), ((14, 32, 32, 1), 17)], ids=["33-17-15-5", "14-32-32-1"])
def test_inactive_trial_inside_a_packed_job(dims, n, mode, monkeypatch):
    """Three trials, the middle one switched off before the first epoch: every buffer of it keeps its
    bits over three epochs (weights, moments, step, transposed copy, loss accumulator, its NaN
    slices of the gathered rows, activations and deltas); its neighbours pass the stage checks."""
    _env(monkeypatch, mode)
    X, y, perms, ps = so.make_case(dims, n, 3)
    job = Job(dims, X, y, perms, ps, so.LRS, None, mode, inactive=(1,))
    expect_path(job, mode)
    what = f"{'-'.join(map(str, dims))} inactive {mode}"
    worst = {}
    s0 = job.snap()
    s1 = run_stage_epochs(job, what, (0, 2), worst)
    row = {k: np.zeros(s0[k].shape, bool) for k in ("params", "m", "v", "step", "wt", "loss_acc", "grads", "curve", "n_iter")
           if k in s0}
    for k in row:
        row[k][1] = True
    assert_kept(what, s0, s1, row.keys(), row)
    for k in ("acts", "deltas"):
        assert np.isnan(s1[k][:, 1]).all(), k
    if job.fused:
        assert np.isnan(s1["xb"][1]).all()
    assert int(s1["active"][1]) == 0 and int(s1["step"][1]) == 0
    report(what, worst)


def test_packed_trials_stop_at_different_epochs_like_numpy():
    """Three packed trials whose stop rule fires at epochs 41, 34 and 25 under the numpy backend
    (tests/test_sk_step_oracle_cpu.py asserts the separation and the margin to the threshold): the
    device job gives each trial the same n_iter_, loss curve (rtol 1e-9) and weights (rtol 1e-7 /
    atol 1e-9: test_hip_float64_matches_numpy's tolerances), and a trial that stopped while others
    went on has the weights of its single-estimator fit bit for bit."""
    X, y = so.stop_case()
    kw = dict(hidden_layer_sizes=so.STOP_DIMS[1:-1], max_iter=so.STOP_MAX_ITER, tol=so.STOP_TOL, random_state=42)
    host = [MLPClassifier(learning_rate_init=lr, backend="numpy", **kw).fit(X, y) for lr in so.STOP_LRS]
    packed = fit_packed([MLPClassifier(learning_rate_init=lr, backend="hip", dtype="float64", **kw) for lr in so.STOP_LRS],
                        X, y)
    stops = [e.n_iter_ for e in host]
    assert len(set(stops)) == 3 and max(stops) < so.STOP_MAX_ITER, stops
    for a, b, lr in zip(host, packed, so.STOP_LRS):
        assert b._hip_fused and b.n_iter_ == a.n_iter_, (lr, a.n_iter_, b.n_iter_)
        np.testing.assert_allclose(b.loss_curve_, a.loss_curve_, rtol=1e-9)
        for u, v in zip(a.coefs_ + a.intercepts_, b.coefs_ + b.intercepts_):
            np.testing.assert_allclose(v, u, rtol=1e-7, atol=1e-9)
        single = MLPClassifier(learning_rate_init=lr, backend="hip", dtype="float64", **kw).fit(X, y)
        assert single.n_iter_ == b.n_iter_
        for u, v in zip(single.coefs_ + single.intercepts_, b.coefs_ + b.intercepts_):
            np.testing.assert_array_equal(u, v)

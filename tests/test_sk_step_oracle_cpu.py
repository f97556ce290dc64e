"""The stage oracle of the float64 sklearn step (sk_step_oracle.py) on the CPU: its bounds hold for a
correct float64 implementation and reject wrong ones.

For every case of the GPU table (tests/test_sk_step_stages.py) the step runs in numpy float64 with
ordinary ``@`` -- a correct implementation with BLAS's summation order -- and must sit inside every
bound of ``check_step``; the longdouble model, chained over 3 epochs, must be ``_fit_numpy``'s
algorithm to 1e-13.  Then eleven wrong implementations (a dropped row, 1 / B on a short minibatch, no
L2 term, a missing or shifted bias, swapped or zeroed output columns, a mask from the wrong layer,
another trial's weights, Adam's step off by one, a stale transposed copy) must each be rejected by
the same checker at every case where they can occur."""
import numpy as np
import pytest

from fedmi.models.sklearn_mlp import _fit_numpy

from . import sk_step_oracle as so

pytestmark = pytest.mark.skipif(not so.HAVE_LONGDOUBLE, reason="numpy longdouble has no 64-bit mantissa here")

ALL = so.CASES + so.CASES_B1


class NotApplicable(Exception):
    pass


def np_step(X, y, perm_row, off, rows, B, dims, kind, alpha, lr, t, p, m, v, bug=None, p_other=None):
    """One step in float64 numpy; ``bug`` makes it wrong in one named way.  Returns (obs, p, m, v,
    row-loss sum, sum W^2)."""
    L = len(dims) - 1
    Ws, bs = so.unflat(p_other if bug == "trial_prev" else p, dims)
    idx = perm_row[off:off + rows]
    acts = [X[idx]]
    done = bug not in ("bias_omitted", "bias_shifted", "swap_cols", "zero_last_col")
    for l in range(L):
        N = dims[l + 1]
        act = (lambda z: np.maximum(z, 0)) if l + 1 < L else (lambda z: z)
        good = act(acts[-1] @ Ws[l] + bs[l])
        z = good.copy()
        if not done:
            if bug == "bias_omitted":
                z = act(acts[-1] @ Ws[l])
            elif bug == "bias_shifted" and N >= 2:
                z = act(acts[-1] @ Ws[l] + np.roll(bs[l], 1))
            elif bug == "swap_cols" and N >= 2:
                z[:, [0, N - 1]] = z[:, [N - 1, 0]]
            elif bug == "zero_last_col" and N % 16:
                z[:, N - 1] = 0.0
            done = not np.array_equal(z, good)   # the first layer where the slip shows
        acts.append(z)
    if not done:
        raise NotApplicable(bug)
    yb = y[idx]
    if kind == "logistic":
        pr = 1.0 / (1.0 + np.exp(-acts[-1][:, 0]))
        pc = np.clip(pr, so.EPS64, 1 - so.EPS64)
        loss = np.where(yb == 1, -np.log(pc), -np.log(1 - pc))
        d = (pr - yb)[:, None]
    else:
        e = np.exp(acts[-1] - acts[-1].max(axis=1, keepdims=True))
        pr = e / e.sum(axis=1, keepdims=True)
        loss = -np.log(np.clip(pr[np.arange(rows), yb], so.EPS64, 1 - so.EPS64))
        d = pr.copy()
        d[np.arange(rows), yb] -= 1.0
    if bug == "inv_B":
        if rows == B:
            raise NotApplicable(bug)
        d = d / B
    else:
        d = d / rows
    deltas = [None] * L
    deltas[L - 1] = d
    for l in range(L - 1, 0, -1):
        src = acts[l]
        if bug == "mask_wrong_layer":
            if L < 3:
                raise NotApplicable(bug)
            other = acts[l - 1] if l > 1 else acts[l + 1]     # another hidden layer's activation
            src = other[:, np.arange(dims[l]) % other.shape[1]]
            if l == 1 and np.array_equal(src > 0, acts[l] > 0):
                raise NotApplicable(bug)
        deltas[l - 1] = (deltas[l] @ Ws[l].T) * (src > 0)
    own_Ws, _ = so.unflat(p, dims)
    gWs, gbs, dWs = [], [], []
    for l in range(L):
        a, dl = acts[l], deltas[l]
        if bug == "drop_last_row":
            a, dl = a[:-1], dl[:-1]
        dWs.append(a.T @ dl)
        gWs.append(dWs[-1] + (0.0 if bug == "no_alpha" else alpha * own_Ws[l] / rows))
        gbs.append(dl.sum(axis=0))
    g = so.flat(gWs, gbs)
    ta = t - 1 if bug == "adam_prev_step" and t >= 2 else t   # (t = 1 would divide by 1 - beta^0: not subtle)
    m1 = so.BETA1 * m + (1 - so.BETA1) * g
    v1 = so.BETA2 * v + (1 - so.BETA2) * g * g
    with np.errstate(divide="ignore", invalid="ignore"):
        lrt = lr * np.sqrt(1 - so.BETA2 ** ta) / (1 - so.BETA1 ** ta)
        p1 = p - lrt * m1 / (np.sqrt(v1) + so.ADAM_EPS)
    wt = so.flat_t(*so.unflat(p if bug == "wt_stale" else p1, dims))
    obs = {"xb": acts[0], "acts": acts[1:L], "deltas": deltas, "p": p1, "m": m1, "v": v1, "wt": wt,
           "logits_kept": acts[L], "grads_kept": so.flat(dWs, gbs)}
    return obs, p1, m1, v1, loss.sum(), sum((W * W).sum() for W in own_Ws)


def run_case(case, bug=None, layered_view=False):
    """3 epochs of every trial of a case through np_step and check_step.  Returns the worst
    error / bound per stage; raises so.StageError at the first stage outside its bound."""
    dims, n, batch, T = case
    X, y, perms, ps = so.make_case(dims, n, T)
    B = min(200, n) if batch is None else batch
    kind = so.kind_of(dims)
    worst, applied = {}, False
    for tr in range(T):
        p, m, v = ps[tr].copy(), np.zeros_like(ps[tr]), np.zeros_like(ps[tr])
        t = 0
        for e in range(so.EPOCHS):
            rl, rb, sqs, rows_l, got = so.LD(0), so.LD(0), [], [], 0.0
            for off, rows in so.steps_of(n, B):
                t += 1
                try:
                    if bug is None or (bug == "trial_prev" and tr == 0):
                        raise NotApplicable(bug)
                    obs, p1, m1, v1, ls, sq = np_step(X, y, perms[e], off, rows, B, dims, kind, so.ALPHA, so.LRS[tr], t,
                                                      p, m, v, bug, ps[tr - 1] if tr else None)
                except NotApplicable:
                    p1 = None
                if p1 is None:   # the slip cannot occur in this step: the correct step instead
                    obs, p1, m1, v1, ls, sq = np_step(X, y, perms[e], off, rows, B, dims, kind, so.ALPHA, so.LRS[tr], t,
                                                      p, m, v)
                else:
                    applied = True
                if layered_view:
                    obs["logits"], obs["grads"] = obs["logits_kept"], obs["grads_kept"]
                _, ml, mb, msq = so.check_step(f"{so.case_id(case)} trial {tr} epoch {e} rows {off}+{rows}", X, y, perms[e],
                                               off, rows, dims, kind, so.ALPHA, so.LRS[tr], t, {"p": p, "m": m, "v": v},
                                               obs, worst)
                p, m, v = p1, m1, v1
                rl, rb = rl + ml, rb + mb
                sqs.append(msq), rows_l.append(rows)
                got += ls + 0.5 * so.ALPHA * sq
            ref = so.epoch_loss([rl], sqs, so.ALPHA, n)
            bnd = so.loss_bound(rows_l, dims, so.ALPHA, abs(rl), rb, sum(sqs)) / n
            so._worst(f"{so.case_id(case)} trial {tr} epoch {e} loss", np.float64(got / n), ref, bnd, worst, "loss")
    if bug is not None and not applied:
        raise NotApplicable(bug)
    return worst


@pytest.mark.parametrize("layered_view", [False, True], ids=["fused-view", "layered-view"])
@pytest.mark.parametrize("case", ALL, ids=so.case_id)
def test_float64_numpy_step_is_inside_every_bound(case, layered_view):
    worst = run_case(case, layered_view=layered_view)
    print("BOUNDS", so.case_id(case), {k: f"{v:.3g}" for k, v in worst.items()})
    assert set(worst) >= {"gather", "forward", "head", "m", "v", "gradient", "params", "wt", "loss"}
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("case", ALL, ids=so.case_id)
def test_longdouble_model_is_fit_numpy(case):
    dims, n, batch, T = case
    X, y, perms, ps = so.make_case(dims, n, T)
    B = min(200, n) if batch is None else batch
    ests = so.make_estimators(dims, ps, so.LRS, batch, "numpy", max_iter=so.EPOCHS)
    for tr, est in enumerate(ests):
        assert est._batch(n) == B
        _fit_numpy(est, X, y, perms, False)
        assert est.n_iter_ == so.EPOCHS
        p, curve = so.model_fit(X, y, perms, B, dims, so.kind_of(dims), so.ALPHA, so.LRS[tr], ps[tr])
        got = so.flat(est.coefs_, est.intercepts_)
        Ws, bs = so.unflat(p, dims)
        for a, b in zip(est.coefs_ + est.intercepts_, Ws + bs):
            assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), (tr, float(np.abs(a - b).max()), float(np.abs(b).max()))
        assert got.shape == p.shape
        np.testing.assert_allclose(np.asarray(est.loss_curve_), np.asarray(curve, np.float64), rtol=1e-13)


BUGS = ["drop_last_row", "inv_B", "no_alpha", "bias_omitted", "bias_shifted", "swap_cols", "zero_last_col",
        "mask_wrong_layer", "trial_prev", "adam_prev_step", "wt_stale"]
# where a slip cannot occur: 1 / B needs a short last minibatch; a shifted bias or swapped columns a layer
# of two columns; a zeroed last column a width off the tile; the wrong layer's mask two hidden layers;
# another trial's weights a second trial
APPLIES = {
    "inv_B": lambda c: c in so.CASES_B1,
    "bias_shifted": lambda c: max(c[0][1:]) >= 2,
    "swap_cols": lambda c: max(c[0][1:]) >= 2,
    "zero_last_col": lambda c: any(w % 16 for w in c[0][1:]),
    "mask_wrong_layer": lambda c: len(c[0]) >= 4,
    "trial_prev": lambda c: c[3] >= 2,
}


@pytest.mark.parametrize("bug", BUGS)
@pytest.mark.parametrize("case", ALL, ids=so.case_id)
def test_checker_rejects_wrong_implementations(case, bug):
    if not APPLIES.get(bug, lambda c: True)(case):
        with pytest.raises(NotApplicable):
            run_case(case, bug)
        return
    with pytest.raises(so.StageError) as ei:
        run_case(case, bug)
    print("REJECTED", so.case_id(case), bug, "--", str(ei.value)[:160])


def test_stop_case_separates_the_stop_epochs():
    """The packed early-stop case of the GPU test: under the numpy backend the three trials stop at
    epochs at least 3 apart, all before max_iter, and no epoch's loss comes within 1e-6 relative of
    the stop rule's threshold best - tol, so 1e-9 of device noise cannot move a stop."""
    X, y = so.stop_case()
    stops = []
    for lr in so.STOP_LRS:
        from fedmi.models.sklearn_mlp import MLPClassifier
        e = MLPClassifier(hidden_layer_sizes=so.STOP_DIMS[1:-1], learning_rate_init=lr, max_iter=so.STOP_MAX_ITER,
                          tol=so.STOP_TOL, random_state=42, backend="numpy").fit(X, y)
        best = np.inf
        for loss in e.loss_curve_:
            assert abs(loss - (best - so.STOP_TOL)) >= 1e-6 * loss, (lr, loss, best)
            best = min(best, loss)
        stops.append(e.n_iter_)
    print("STOPS", stops)
    assert so.STOP_MAX_ITER <= 60 and max(stops) < so.STOP_MAX_ITER, stops
    s = sorted(stops)
    assert s[1] - s[0] >= 3 and s[2] - s[1] >= 3, stops

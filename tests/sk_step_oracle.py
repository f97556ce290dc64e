"""Host model of ONE minibatch step of the float64 sklearn-compatible trainer, stage by stage, in
numpy ``longdouble`` (64-bit mantissa on x86), with error bounds derived from the operands.

Each function models one stage of the step (mlp_fused_f64.hip / mlp_f64.hip) and takes that
stage's operands as arguments, so a test can feed it the device's own stage inputs: the forward of
layer l is checked on the activations the device wrote for layer l - 1, the gradient on the
device's activations and deltas, the parameter update on the device's moments.  Every stage is
then isolated from the rounding of the one before.

Bounds.  A float64 sum of n terms, in any order and with any fma contraction, differs from the
exact sum by at most ``bound(n, mag) = (n + 2) eps64 sum|terms|`` (each rounding is eps64 / 2
relative to a partial sum no larger than sum|terms|, and there are at most n + a few of them: the
factor two is the whole margin).  ``mag`` always comes from the operands, never from the result
under test.  The other stages: see :func:`check_step`.

The weights are handled in sklearn's layout (``W`` [in, out]); :func:`unflat` / :func:`flat` map
them to the trainer's flat buffers ([out][in] weights, then the bias, per layer)."""
import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps < 1e-18)
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def ld(x):
    return np.asarray(x, dtype=LD)


def bound(n, mag):
    return (n + 2) * LD(EPS64) * ld(mag)


# ------------------------------------------------------------------------------ flat layout
def n_params(dims):
    return sum(k * n + n for k, n in zip(dims[:-1], dims[1:]))


def unflat(p, dims):
    """Trainer layout [P] -> (Ws [in, out], bs), copies in the dtype of ``p``."""
    Ws, bs, off = [], [], 0
    for K, N in zip(dims[:-1], dims[1:]):
        Ws.append(p[off:off + N * K].reshape(N, K).T.copy())
        off += N * K
        bs.append(p[off:off + N].copy())
        off += N
    return Ws, bs


def flat(Ws, bs):
    return np.concatenate([np.concatenate([np.asarray(W).T.reshape(-1), np.asarray(b).reshape(-1)])
                           for W, b in zip(Ws, bs)])


def flat_t(Ws, bs):
    """The transposed weight copy ``wt``: each layer's [in][out] at the weights' offset, zeros at the
    bias's."""
    return np.concatenate([np.concatenate([np.asarray(W).reshape(-1), np.zeros(np.asarray(b).size, np.asarray(W).dtype)])
                           for W, b in zip(Ws, bs)])


# ------------------------------------------------------------------------------ the stages
def gather(X, perm_row, off, rows):
    return np.asarray(X)[np.asarray(perm_row)[off:off + rows]]


def forward_layer(a_in, W, b, relu):
    a, W, b = ld(a_in), ld(W), ld(b)
    z = a @ W + b
    mag = np.abs(a) @ np.abs(W) + np.abs(b)
    return (np.maximum(z, 0) if relu else z), mag


def head(z, y, kind, rows):
    """(row losses, delta = (p - onehot) / rows, sensitivity of p to each logit).  ``kind``
    "logistic": one logit, sklearn's binary log-loss on p clipped to [eps64, 1 - eps64] (the clip is
    on the loss only); "softmax": the row maximum subtracted, p_y clipped."""
    z = ld(z)
    y = np.asarray(y)
    eps = LD(EPS64)
    if kind == "logistic":
        p = 1 / (1 + np.exp(-z[:, 0]))
        pc = np.clip(p, eps, 1 - eps)
        loss = np.where(y == 1, -np.log(pc), -np.log(1 - pc))
        delta = ((p - y) / rows)[:, None]
    else:
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        onehot = np.zeros_like(p)
        onehot[np.arange(len(y)), y] = 1
        loss = -np.log(np.clip(p[np.arange(len(y)), y], eps, 1 - eps))
        delta = (p - onehot) / rows
    return loss, delta, 1.0


def backward_layer(delta_out, W, mask):
    d, W = ld(delta_out), ld(W)
    mask = np.asarray(mask, dtype=bool)
    return (d @ W.T) * mask, (np.abs(d) @ np.abs(W).T) * mask


def wgrad(delta, a_in, W_before, alpha, rows):
    """``delta`` carries the 1 / rows already (the kernels' form; ``_fit_numpy`` divides after the
    product): gW = a_in^T delta + alpha W / rows, gb = column sums.  mag = (|a_in|^T |delta|,
    sum |delta|, |alpha W / rows|)."""
    d, a, W = ld(delta), ld(a_in), ld(W_before)
    l2 = LD(alpha) * W / rows
    return a.T @ d + l2, d.sum(axis=0), (np.abs(a).T @ np.abs(d), np.abs(d).sum(axis=0), np.abs(l2))


def lr_t(lr, t, b1=BETA1, b2=BETA2):
    return LD(lr) * np.sqrt(1 - LD(b2) ** t) / (1 - LD(b1) ** t)


def pow_kappa(t, b1=BETA1, b2=BETA2):
    """Relative error of a float64 ``lr_t`` in units of eps64 from the subtraction 1 - beta^t alone: a
    pow() within one ulp leaves beta^t wrong by eps64 beta^t, which 1 - beta^t (exact: Sterbenz) turns
    into eps64 beta^t / (1 - beta^t) relative -- 250 at t = 2 for beta2 = 0.999, halved by the square
    root.  numpy's and sklearn's own float64 steps show it (32 eps64 at t = 2), so the 8 eps64 that cover
    the roundings of pow, sqrt and the division cannot hold the update without this term."""
    return float(0.5 * LD(b2) ** t / (1 - LD(b2) ** t) + LD(b1) ** t / (1 - LD(b1) ** t))


def adam(p, m, v, g, t, lr, b1=BETA1, b2=BETA2, eps=ADAM_EPS):
    p, m, v, g = ld(p), ld(m), ld(v), ld(g)
    m = LD(b1) * m + (1 - LD(b1)) * g
    v = LD(b2) * v + (1 - LD(b2)) * g * g
    return p - lr_t(lr, t, b1, b2) * m / (np.sqrt(v) + LD(eps)), m, v


def epoch_loss(row_loss_sums, sq_sums, alpha, n):
    """(sum of the row losses + 0.5 alpha sum over the steps of sum W^2 (pre-update)) / n."""
    return (sum(ld(x) for x in row_loss_sums) + LD(0.5) * LD(alpha) * sum(ld(x) for x in sq_sums)) / n


# ------------------------------------------------------------------------------ one step, chained
def model_step(X, y, perm_row, off, rows, dims, kind, alpha, lr, t, p, m, v):
    """The whole step in longdouble on its own intermediates (the algorithm, not a check):
    returns (p, m, v, sum of row losses, sum W^2 before the update)."""
    L = len(dims) - 1
    Ws, bs = unflat(ld(p), dims)
    idx = np.asarray(perm_row)[off:off + rows]
    acts = [ld(gather(X, perm_row, off, rows))]
    for l in range(L):
        acts.append(forward_layer(acts[-1], Ws[l], bs[l], l + 1 < L)[0])
    loss, delta, _ = head(acts[-1], np.asarray(y)[idx], kind, rows)
    gWs, gbs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        gWs[l], gbs[l], _ = wgrad(delta, acts[l], Ws[l], alpha, rows)
        if l > 0:
            delta = backward_layer(delta, Ws[l], acts[l] > 0)[0]
    p1, m1, v1 = adam(p, m, v, flat(gWs, gbs), t, lr)
    return p1, m1, v1, loss.sum(), sum((W * W).sum() for W in Ws)


def model_fit(X, y, perms, B, dims, kind, alpha, lr, p0):
    """``_fit_numpy`` without its stop rule, in longdouble: (p, loss curve)."""
    n = len(X)
    p, m, v = ld(p0), np.zeros(len(p0), LD), np.zeros(len(p0), LD)
    t, curve = 0, []
    for e in range(len(perms)):
        ls, sq = [], []
        for off in range(0, n, B):
            t += 1
            p, m, v, l, s = model_step(X, y, perms[e], off, min(B, n - off), dims, kind, alpha, lr, t, p, m, v)
            ls.append(l)
            sq.append(s)
        curve.append(epoch_loss(ls, sq, alpha, n))
    return p, curve


# ------------------------------------------------------------------------------ the checker
class StageError(AssertionError):
    pass


def _worst(what, got, ref, bnd, worst, stage):
    """max (error / bound) over EVERY element; a NaN, or an error where the bound is zero, fails."""
    got, ref, bnd = ld(got), ld(ref), ld(bnd)
    assert got.shape == ref.shape == bnd.shape, (what, got.shape, ref.shape, bnd.shape)
    if got.size == 0:
        return
    err = np.abs(got - ref)
    bad = ~(err <= bnd)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, LD(0), err / bnd)
    ratio = np.where(bad & ~(ratio > 1), np.inf, ratio)
    worst[stage] = max(worst.get(stage, 0.0), float(ratio.max()))
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, ratio, -1))), got.shape)
        raise StageError(f"{what}: stage {stage}, shape {got.shape}, element {tuple(int(x) for x in i)}: got "
                         f"{float(got[i])!r}, model {float(ref[i])!r}, error {float(err[i]):.3e} > bound "
                         f"{float(bnd[i]):.3e}; {int(bad.sum())} of {got.size} elements outside")


def check_step(what, X, y, perm_row, off, rows, dims, kind, alpha, lr, t, before, obs, worst=None):
    """One trial's observed step against the model, each stage on the OBSERVED inputs of that stage.

    before: p, m, v (flat, float64) before the step.  obs: ``xb`` [rows][F]; ``acts`` the L - 1
    hidden activations; ``deltas`` the L deltas; ``p``, ``m``, ``v`` after; optional ``logits``
    (the layered path keeps them), ``grads`` (flat, without the L2 term: the layered path),
    ``wt`` (flat transposed copy).  Returns (worst error / bound per stage, sum of the model's row
    losses on the observed activations, its bound, sum W^2).  Bounds:

    gather exact; forward bound(K, mag); head delta (logit bound (the row's largest: a softmax
    output moves by at most the largest logit error) + 8 eps64) / rows; backward bound(N, mag) under
    the mask of the observed activation; gradient bound(rows, mag) + 2 eps64 |alpha W / rows|;
    m: (1 - b1) dg + 2 eps64 |m|; v: (1 - b2)(2 |g| dg + dg^2) + 2 eps64 |v|; the update recomputed
    from the observed m, v: 8 eps64 (|p| + |update|) + eps64 kappa_t |update| (:func:`pow_kappa`: the
    cancellation in 1 - beta^t that every float64 Adam has, sklearn's included); wt bit-equal to the
    observed weights."""
    worst = {} if worst is None else worst
    L = len(dims) - 1
    eps = LD(EPS64)
    Ws, bs = unflat(np.asarray(before["p"], np.float64), dims)
    idx = np.asarray(perm_row)[off:off + rows]
    yb = np.asarray(y)[idx]
    xb = np.asarray(obs["xb"], np.float64)
    _worst(what, xb, gather(X, perm_row, off, rows), np.zeros(xb.shape), worst, "gather")
    ins = [xb] + [np.asarray(a, np.float64) for a in obs["acts"]]
    assert len(ins) == L and len(obs["deltas"]) == L
    for l in range(L - 1):
        z, mag = forward_layer(ins[l], Ws[l], bs[l], True)
        _worst(f"{what} layer {l}", ins[l + 1], z, bound(dims[l], mag), worst, "forward")
    z, mag = forward_layer(ins[L - 1], Ws[L - 1], bs[L - 1], False)
    bz = bound(dims[L - 1], mag)
    if obs.get("logits") is not None:
        _worst(f"{what} layer {L - 1} (logits)", obs["logits"], z, bz, worst, "forward")
        z, bz = ld(np.asarray(obs["logits"], np.float64)), np.zeros(z.shape, LD)
    loss, delta, sens = head(z, yb, kind, rows)
    bzr = np.broadcast_to(bz.max(axis=1, keepdims=True), z.shape)
    deltas = [np.asarray(d, np.float64) for d in obs["deltas"]]
    _worst(f"{what} head", deltas[L - 1], delta, (sens * bzr + 8 * eps) / rows, worst, "head")
    # the loss of a row moves by at most sum_j |p_j - onehot_j| |dz_j| <= 2 max |dz|; exp / log: 8 eps64
    loss_bound = (2 * bzr[:, 0] + 8 * eps * (1 + np.abs(loss))).sum()
    for l in range(L - 1, 0, -1):
        d, mag = backward_layer(deltas[l], Ws[l], ins[l] > 0)
        _worst(f"{what} layer {l} -> {l - 1}", deltas[l - 1], d, bound(dims[l + 1], mag), worst, "backward")
    gWs, gbs, bWs, bbs, dWs, bdWs = [], [], [], [], [], []
    for l in range(L):
        gW, gb, (mW, mb, l2) = wgrad(deltas[l], ins[l], Ws[l], alpha, rows)
        gWs.append(gW), gbs.append(gb)
        bWs.append(bound(rows, mW) + 2 * eps * l2), bbs.append(bound(rows, mb))
        dWs.append(wgrad(deltas[l], ins[l], Ws[l], 0.0, rows)[0]), bdWs.append(bound(rows, mW))
    g, bg = flat(gWs, gbs), flat(bWs, bbs)
    if obs.get("grads") is not None:   # the products alone: the layered Adam adds the L2 term itself
        _worst(f"{what} grads", obs["grads"], flat(dWs, gbs), flat(bdWs, bbs), worst, "gradient")
    p1, m1, v1 = adam(before["p"], before["m"], before["v"], g, t, lr)
    b1, b2 = LD(BETA1), LD(BETA2)
    _worst(f"{what} m (t = {t})", obs["m"], m1, (1 - b1) * bg + 2 * eps * np.abs(m1), worst, "m")
    _worst(f"{what} v (t = {t})", obs["v"], v1, (1 - b2) * (2 * np.abs(g) * bg + bg * bg) + 2 * eps * np.abs(v1), worst, "v")
    if t == 1:   # from zero moments m / (1 - b1) is the gradient itself: the m bound in units of g
        assert not np.any(before["m"]) and not np.any(before["v"])
        _worst(f"{what} m / (1 - b1) (t = 1)", ld(np.asarray(obs["m"], np.float64)) / (1 - b1), g,
               bg + 2 * eps * np.abs(g), worst, "gradient")
    upd = lr_t(lr, t) * ld(np.asarray(obs["m"], np.float64)) / (np.sqrt(ld(np.asarray(obs["v"], np.float64))) + LD(ADAM_EPS))
    p0 = ld(np.asarray(before["p"], np.float64))
    _worst(f"{what} params (t = {t})", obs["p"], p0 - upd, 8 * eps * (np.abs(p0) + np.abs(upd)) + eps * pow_kappa(t) * np.abs(upd),
           worst, "params")
    if obs.get("wt") is not None:
        want = flat_t(*unflat(np.asarray(obs["p"], np.float64), dims))
        got = np.asarray(obs["wt"], np.float64)
        same = got.view(np.int64) == want.view(np.int64)
        worst["wt"] = 0.0 if same.all() else float("inf")
        if not same.all():
            i = int(np.argmin(same))
            raise StageError(f"{what}: stage wt, shape {got.shape}, element {i}: the transposed copy holds {got[i]!r}, "
                             f"params {want[i]!r}; {int((~same).sum())} of {got.size} differ")
    sq = sum((ld(W) * ld(W)).sum() for W in Ws)
    return worst, loss.sum(), loss_bound, sq


def loss_bound(rows_per_step, dims, alpha, row_losses_abs, row_bound, sq):
    """Bound of the epoch's loss accumulator (before the division by n): the head's own part plus
    eps64 x (atomic contributions + in-block roundings) x sum |terms| -- the rule for double
    accumulators fed by atomics (tests/test_layered_ops.py).  Contributions per step: at most one per
    16-row block and one per 16 x 16 gradient tile or per 256 parameters; in-block: 16 (an 8-level
    tree, the products and the 0.5 alpha scale)."""
    tiles = sum(((n + 15) // 16) * ((k + 16) // 16) for k, n in zip(dims[:-1], dims[1:]))
    blocks = sum((r + 15) // 16 + tiles + (n_params(dims) + 255) // 256 + 1 for r in rows_per_step)
    return row_bound + LD(EPS64) * (blocks + 16) * (row_losses_abs + LD(0.5) * LD(alpha) * sq)


# ------------------------------------------------------------------------------ the cases
ALPHA = 1e-4
LRS = (0.004, 0.02, 0.009)
EPOCHS = 3
# (dims F-hidden...-outputs (1 output: the logistic head), n, batch (None: one minibatch of n rows), T)
CASES = [
    ((1, 1, 1), 17, None, 2),
    ((5, 16, 3), 1, None, 2),
    ((5, 16, 3), 40, None, 2),
    ((33, 17, 15, 5), 40, None, 2),
    ((14, 272, 9), 33, None, 2),
    ((70, 24, 130, 16), 48, None, 2),
    ((14, 12, 8, 6, 5), 40, None, 2),
    ((14, 20, 17), 40, None, 2),
    ((14, 32, 32, 1), 17, None, 2),
    ((14, 32, 32, 1), 200, None, 2),
    ((20, 33, 17, 3), 40, None, 2),
    ((14, 50, 400, 1), 200, None, 1),
]
# B + 1 rows: an epoch of a 16-row and a 1-row step
CASES_B1 = [((5, 16, 3), 17, 16, 2), ((33, 17, 15, 5), 17, 16, 2)]


def case_id(c):
    dims, n, batch, T = c
    return "-".join(map(str, dims)) + f"-n{n}" + (f"-b{batch}" if batch else "") + f"-T{T}"


def make_case(dims, n, T, seed=0, epochs=EPOCHS):
    """Seeded inputs of a case: X standard normal, labels from a random linear teacher (every class
    occurs once n allows it), one row order per epoch, Glorot-scale weights drawn PER TRIAL (flat,
    trainer layout)."""
    rng = np.random.RandomState(1000 + seed)
    F, C = dims[0], max(2, dims[-1])
    X = rng.standard_normal((n, F))
    score = X @ rng.standard_normal((F, C)) + 0.5 * rng.standard_normal((n, C))
    y = score.argmax(axis=1)
    for c in range(C if n >= C else 0):   # a class the teacher left out takes the row that scores it best
        if not (y == c).any():
            free = np.flatnonzero(np.bincount(y, minlength=C)[y] > 1)
            y[free[score[free, c].argmax()]] = c
    perms = np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int32)
    ps = []
    for _ in range(T):
        Ws, bs = [], []
        for K, N in zip(dims[:-1], dims[1:]):
            s = np.sqrt(6.0 / (K + N))
            Ws.append(rng.uniform(-s, s, (K, N)))
            bs.append(rng.uniform(-s, s, N))
        ps.append(flat(Ws, bs))
    return X, y.astype(np.int64), perms, np.stack(ps)


def steps_of(n, B):
    return [(off, min(B, n - off)) for off in range(0, n, B)]


def kind_of(dims):
    return "logistic" if dims[-1] == 1 else "softmax"


def make_estimators(dims, p_trials, lrs, batch, backend, **kw):
    """Estimators built by hand in the state ``MLPClassifier._fit`` leaves before it trains, with the
    given flat weights per trial."""
    from fedmi.models.sklearn_mlp import MLPClassifier
    ests = []
    for p, lr in zip(p_trials, lrs):
        e = MLPClassifier(hidden_layer_sizes=tuple(dims[1:-1]), learning_rate_init=lr, alpha=ALPHA,
                          batch_size="auto" if batch is None else batch, backend=backend, dtype="float64", **kw)
        e.coefs_, e.intercepts_ = unflat(np.asarray(p, np.float64), dims)
        e.classes_ = np.arange(max(2, dims[-1]))
        e.n_outputs_ = dims[-1]
        e.out_activation_ = kind_of(dims)
        e._adam, e.best_loss_, e._no_improvement_count = None, np.inf, 0
        e.loss_curve_, e.n_iter_, e.t_, e.n_layers_ = [], 0, 0, len(dims)
        ests.append(e)
    return ests


# Packed trials that stop at different epochs (tests/test_sk_step_oracle_cpu.py asserts that these
# values separate the stops; tests/test_sk_step_stages.py runs them on the device)
STOP_DIMS, STOP_N, STOP_MAX_ITER = (14, 20, 6, 1), 240, 60
STOP_LRS, STOP_TOL = (0.01, 0.02, 0.05), 3e-3


def stop_case():
    X, y, _, _ = make_case(STOP_DIMS, STOP_N, 1, seed=77, epochs=1)
    return X, y

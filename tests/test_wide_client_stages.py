"""``WideClient`` (fedmi/fl/wide.py) in situ, bf16: one full-batch step per configuration, every
stage of every micro-batch held to its float64 model (wide_oracle.py) applied to the snapshot of
that stage's own INPUTS, so that no bf16 rounding flip carries from one stage into the next.

The test wraps ``c._backward``: after each micro-batch's backward has run and the stream is
synchronised it copies out the operands, activations, deltas, slabs and gradients (and, before the
backward, the gradients it accumulates onto), then fills every activation / delta / scratch / slab
buffer with NaN again, as it did before the step: a micro-batch may depend on ``grads`` alone, and
a stale element multiplied by a zero delta shows as NaN.

Tolerances.  Conversions, pads and transposed copies are bitwise.  bf16 GEMM outputs (layer
outputs, dgrads) follow the interval rule of test_wide_nt_gemm.py with E = lo.bound(e) * scale, e
the largest transcription error over the GEMM stages of the step; logits, dz_out and the gradients
are within ``lo.bound`` of the largest transcription error of their own group (logits with the
GEMMs; the loss head; weight and bias gradients).  The column-sum slab is held to 34 additions
(derived in test_wide_nt_gemm.py)."""
import numpy as np
import pytest
import torch

from fedmi.data.synthetic import make_income_like
from fedmi.fl.wide import WideClient

from . import layered_oracle as lo
from . import wide_oracle as wo

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")

# dims, micro-batch, rows
CONFIGS = {
    "256_and_128_loops_padded_tail": ([14, 256, 128, 256, 2], 256, 456),
    "mb128_all_128_loop": ([14, 256, 256, 2], 128, 200),
    "no_skinny_ldi64_tail128": ([17, 128, 256, 3], 256, 384),
    "generic_everywhere": ([14, 200, 72, 2], 256, 356),
    "mixed_then_generic_tail": ([14, 256, 192, 256, 2], 256, 356),
}


def _data(dims, n):
    if dims[0] == 14 and dims[-1] == 2:
        X, y = make_income_like(n, seed=3)
        return np.asarray(X, dtype=F32), np.asarray(y)
    rng = np.random.RandomState(n)
    return rng.randn(n, dims[0]).astype(F32), rng.randint(0, dims[-1], n)


def _client(dims, mb, n, **kw):
    dev = torch.device("cuda", 0)
    X, y = _data(dims, n)
    c = WideClient(torch.as_tensor(X, device=dev), torch.as_tensor(y, device=dev), dims, micro_batch=mb, dtype="bf16",
                   seed=5, **kw)
    return c, X, y


def _volatile(c):
    """Every buffer a micro-batch writes before it reads (not the weight copies, not grads)."""
    ts = list(c.hq) + list(c.hT) + list(c.dzq) + list(c.dzT) + [c.xq, c.scratch, c.dz_out, c.wg_slab]
    if c._pad:
        ts += [c.xp, c.dzp, c.logits_p]
    else:
        ts.append(c.logits)
    ts += [t for t in (c.sk_slab, c.cs_slab) if t is not None]
    return ts


def _nan_fill(c):
    for t in _volatile(c):
        t.fill_(NAN)


def _np(t):
    """Device tensor -> (float32 values, bit pattern) on the host."""
    h = t.detach().cpu().contiguous()
    if h.dtype == torch.bfloat16:
        return h.float().numpy(), h.view(torch.int16).numpy().view(np.uint16)
    return h.numpy().copy(), h.numpy().view(np.uint32).copy()


def _snapshot(c):
    s = {"hq": [_np(t) for t in c.hq], "hT": [_np(t) for t in c.hT], "dzq": [_np(t) for t in c.dzq],
         "dzT": [_np(t) for t in c.dzT], "xq": _np(c.xq), "dz_out": _np(c.dz_out), "grads": _np(c.grads)[0],
         "logits": _np(c.logits_p if c._pad else c.logits)}
    if c._pad:
        s["xp"], s["dzp"] = _np(c.xp), _np(c.dzp)
    if c.cs_slab is not None:
        s["cs"] = _np(c.cs_slab)[0]
    return s


def _is_nan(v):
    return bool(np.isnan(v).all())


def _weight_copies_are_bf16_of(c, params, what):
    """Wq, WqT, W0p, WhTp, Whp[:C], bhp[:C] bitwise the bf16 images of ``params`` (host array)."""
    L, dims = c.L, c.dims
    W = [params[off:off + int(np.prod(s))].reshape(s) for _, s, off in c.layout[0::2]]
    b = [params[off:off + int(np.prod(s))].reshape(s) for _, s, off in c.layout[1::2]]
    torch.cuda.synchronize()
    for l in range(L):
        want = lo.bf16_bits(W[l])
        np.testing.assert_array_equal(_np(c.Wq[l])[1], want, err_msg=f"{what}: Wq[{l}]")
        np.testing.assert_array_equal(_np(c.WqT[l])[1], want.T, err_msg=f"{what}: WqT[{l}]")
    if c._pad:
        F, C = dims[0], dims[-1]
        w0p, whtp, whp = _np(c.W0p)[1], _np(c.WhTp)[1], _np(c.Whp)[1]
        np.testing.assert_array_equal(w0p[:, :F], lo.bf16_bits(W[0]), err_msg=f"{what}: W0p")
        np.testing.assert_array_equal(whtp[:, :C], lo.bf16_bits(W[L - 1]).T, err_msg=f"{what}: WhTp")
        np.testing.assert_array_equal(whp[:C], lo.bf16_bits(W[L - 1]), err_msg=f"{what}: Whp")
        assert not w0p[:, F:].any() and not whtp[:, C:].any() and not whp[C:].any(), f"{what}: pad not zero"
        bhp = _np(c.bhp)[1]
        np.testing.assert_array_equal(bhp[:C], b[L - 1].view(np.uint32), err_msg=f"{what}: bhp")
        assert not bhp[C:].any()
    return W, b


class Checks:
    """Collects the comparisons of one step; the bounds come from the transcriptions of all of
    them, so they are asserted at the end."""

    def __init__(self):
        self.items, self.e = [], {"gemm": 0.0, "head": 0.0, "grad": 0.0}

    def value(self, group, what, got, model):
        ref, tr, scale = model[:3]
        self.e[group] = max(self.e[group], lo.nerr(tr, ref, scale))
        self.items.append(("value", group, what, got, ref, scale))

    def interval(self, what, got, model, relu, keep):
        ref, tr, scale, before = model
        self.e["gemm"] = max(self.e["gemm"], lo.nerr(tr, ref, scale))
        self.items.append(("interval", "gemm", what, got, before, scale, relu, keep))

    def finish(self, name):
        tb = {g: lo.bound(e) for g, e in self.e.items()}
        worst = {g: 0.0 for g in self.e}
        for it in self.items:
            kind, group, what, got = it[:4]
            assert np.isfinite(got).all(), f"{what}: not finite"
            if kind == "value":
                err = lo.nerr(got, it[4], it[5])
                worst[group] = max(worst[group], err)
                assert err <= tb[group], f"{what}: err {err:.3e} > bound {tb[group]:.3e}"
            else:
                lo_, hi = wo.bf16_interval(it[4], tb["gemm"] * it[5], it[6], it[7])
                bad = np.flatnonzero(~((got >= lo_) & (got <= hi)).ravel())
                assert bad.size == 0, (f"{what}: {bad.size} elements outside their interval, first {bad[:4]}: got "
                                       f"{got.ravel()[bad[:4]]} lo {lo_.ravel()[bad[:4]]} hi {hi.ravel()[bad[:4]]}")
        for g in self.e:
            print(f"wide stages {name} {g}: worst err {worst[g]:.3e} (transcription {self.e[g]:.3e}) bound {tb[g]:.3e}"
                  + (f", err / bound {worst[g] / tb[g]:.3f}" if tb[g] > 0 else ""))


def _check_micro_batch(ck, c, s, g0, X, y, W, b, r0, rows, beta, tag):
    dims, L, mb, n = c.dims, c.L, c.mb, c.n
    F, C = dims[0], dims[-1]
    p = wo.wide_plan(dims, mb, rows)
    pad, re = p["rp"] is not None, p["rows_eff"]
    Wq = [lo.bf16_round(w) for w in W]
    grad = lambda g, l, k: g[c.layout[2 * l + k][2]:][:int(np.prod(c.layout[2 * l + k][1]))].reshape(c.layout[2 * l + k][1])
    xb = lo.bf16_bits(X[r0:r0 + rows])
    # ---- input conversion / padding
    if pad:
        xv, xbits = s["xp"]
        np.testing.assert_array_equal(xbits[:rows, :F], xb, err_msg=f"{tag}: xp")
        assert not xbits[:rows, F:].any() and not xbits[rows:re].any(), f"{tag}: xp pads are not zero"
        assert _is_nan(xv[re:]), f"{tag}: xp written past rp"
        acts = [xv[:re, :F]]
    else:
        xv, xbits = s["xq"]
        np.testing.assert_array_equal(xbits.ravel()[:rows * F].reshape(rows, F), xb, err_msg=f"{tag}: xq")
        acts = [xv.ravel()[:rows * F].reshape(rows, F)]
    # ---- hidden layers
    for l in range(L - 1):
        hv, hbits = s["hq"][l]
        ck.interval(f"{tag}: hq[{l}]", hv[:re], wo.nt_gemm(acts[l], Wq[l], bias=b[l], relu=True, pre=True), True, None)
        assert _is_nan(hv[re:]), f"{tag}: hq[{l}] written past its rows"
        tv, tbits = s["hT"][l]
        if l + 2 < L:
            np.testing.assert_array_equal(tbits[:, :re], hbits[:re].T, err_msg=f"{tag}: hT[{l}]")
            assert _is_nan(tv[:, re:]), f"{tag}: hT[{l}] written past rp"
        else:
            assert _is_nan(tv), f"{tag}: hT[{l}] has no reader but was written"
        acts.append(hv[:re])
    # ---- logits, loss head
    zv = s["logits"][0]
    ck.value("gemm", f"{tag}: logits", zv[:re, :C], wo.stage_logits(acts[L - 1], Wq[L - 1], b[L - 1]))
    if pad:
        assert not s["logits"][1][:re, C:].any(), f"{tag}: padded logit columns are not zero"
    dzv, dzbits = s["dz_out"]
    ck.value("head", f"{tag}: dz_out", dzv[:rows], wo.stage_head(zv[:rows, :C], y[r0:r0 + rows], n))
    assert _is_nan(dzv[rows:]), f"{tag}: dz_out written past its rows"
    # ---- the head delta as an operand
    if pad:
        dv, dbits = s["dzp"]
        want = lo.bf16_bits(wo.stage_pad_delta(dzv[:rows], re, 64, rnd=lambda v: v))
        np.testing.assert_array_equal(dbits[:re], want, err_msg=f"{tag}: dzp")
        assert not dbits[rows:re].any(), f"{tag}: dzp rows past the micro-batch are not zero"
        delta = dv[:re, :C]
    else:
        dv, dbits = s["dzq"][L - 1]
        np.testing.assert_array_equal(dbits.ravel()[:rows * C].reshape(rows, C), lo.bf16_bits(dzv[:rows]),
                                      err_msg=f"{tag}: dzq[{L - 1}]")
        delta = dv.ravel()[:rows * C].reshape(rows, C)
    # ---- backward, top down
    g1 = s["grads"]
    ck.value("grad", f"{tag}: gb[{L - 1}]", grad(g1, L - 1, 1), wo.stage_bgrad(dzv[:rows], beta, grad(g0, L - 1, 1)))
    last_cs = None
    for l in range(L - 1, -1, -1):
        ck.value("grad", f"{tag}: gW[{l}]", grad(g1, l, 0), wo.stage_wgrad(delta, acts[l], beta, grad(g0, l, 0)))
        if l < L - 1:
            ck.value("grad", f"{tag}: gb[{l}]", grad(g1, l, 1), wo.stage_bgrad(delta, beta, grad(g0, l, 1)))
        if l == 0:
            break
        qv, qbits = s["dzq"][l - 1]
        keep = wo.keep_of(acts[l])
        ck.interval(f"{tag}: dzq[{l - 1}]", qv[:re], wo.nt_gemm(delta, Wq[l].T, mask=acts[l], pre=True), False, keep)
        assert not (qv[rows:re] != 0).any(), f"{tag}: dzq[{l - 1}] rows past the micro-batch are not zero"
        assert _is_nan(qv[re:]), f"{tag}: dzq[{l - 1}] written past its rows"
        tv, tbits = s["dzT"][l - 1]
        if p["dgrad_nt"][l - 1] and l == 1 and p["skinny"]:
            assert _is_nan(tv), f"{tag}: dzT[0] has no reader but was written"
        else:
            np.testing.assert_array_equal(tbits[:, :re], qbits[:re].T, err_msg=f"{tag}: dzT[{l - 1}]")
            assert _is_nan(tv[:, re:]), f"{tag}: dzT[{l - 1}] written past rp"
        if p["csum"][l - 1]:
            last_cs = (l - 1, qv[:re])
        delta = qv[:re]
    if last_cs is not None:   # the slab holds the sums of the last dgrad that emitted them
        l, q = last_cs
        want, sabs = wo.nt_csum(q)
        got = s["cs"][:(re // 128) * dims[l + 1]].reshape(re // 128, dims[l + 1]).astype(np.float64)
        assert (np.abs(got - want) <= 1.001 * 34 * 2.0 ** -24 * sabs).all(), f"{tag}: column sums of dzq[{l}]"
    assert np.isfinite(g1).all(), f"{tag}: non-finite gradient"
    return p["nt_calls"]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_wide_client_stages(name):
    dims, mb, n = CONFIGS[name]
    c, X, y = _client(dims, mb, n)
    params0 = _np(c.params)[0]
    W, b = _weight_copies_are_bf16_of(c, params0, "after construction")
    snaps = []
    inner = c._backward

    def spy(r0, rows, beta):
        c.stream.synchronize()
        g0 = _np(c.grads)[0]
        inner(r0, rows, beta)
        c.stream.synchronize()
        snaps.append((r0, rows, beta, g0, _snapshot(c)))
        _nan_fill(c)

    c._backward = spy
    with torch.cuda.stream(c.stream):
        _nan_fill(c)
    c.stream.synchronize()
    c.run_round(evaluate=True)
    torch.cuda.synchronize()
    assert [(r0, rows) for r0, rows, *_ in snaps] == [(r0, min(mb, n - r0)) for r0 in range(0, n, mb)]
    assert [beta for _, _, beta, *_ in snaps] == [0.0] + [1.0] * (len(snaps) - 1)
    ck, calls = Checks(), 0
    for r0, rows, beta, g0, s in snaps:
        if beta == 0.0:
            g0 = np.zeros_like(g0)        # not read: the model's beta * g0 term is absent
        calls += _check_micro_batch(ck, c, s, g0, X, y, W, b, r0, rows, beta, f"{name} rows {r0}+{rows}")
    ck.finish(name)
    assert c.nt_calls == calls, (c.nt_calls, calls)
    _weight_copies_are_bf16_of(c, _np(c.params)[0], "after the round (fused evaluation)")
    assert not np.array_equal(_np(c.params)[0], params0)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_wide_client_weight_copies_follow_the_step_with_a_separate_evaluation(name):
    """fused_eval False: the evaluation pass re-quantises, aggregate() must not undo or skip it."""
    dims, mb, n = CONFIGS[name]
    c, _, _ = _client(dims, mb, n, fused_eval=False)
    params0 = _np(c.params)[0]
    c.run_round(evaluate=True)
    torch.cuda.synchronize()
    assert not np.array_equal(_np(c.params)[0], params0)
    _weight_copies_are_bf16_of(c, _np(c.params)[0], "after the round (separate evaluation)")
    acc = c.metrics()["accuracy"]
    assert 0.0 <= acc <= 1.0

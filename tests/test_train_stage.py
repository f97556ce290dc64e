"""ONE train launch, workgroup by workgroup: every slab row's loss slot and gradient partial of the
fused train kernels (fl_train_body.inc, fl_train_bf16_body.inc and their shape-specialised
instantiations) against the float64 oracle of tests/train_stage_oracle.py.

One-client engines, ``graph_rounds=0``, one ``step_train()``; the slab is read through
``slab_partials()`` / ``slab_losses()``.  Every case is a single launch on at most 129 rows.  The kernel
variant is chosen before construction through FEDMI_SHAPE_SPEC / FEDMI_ADAM_SPEC / FEDMI_SLAB_BLOCKED
and checked on the engine's ``layout``.  The CPU module tests/test_train_stage_oracle_cpu.py shows
that every case has a ReLU margin of at least 1e-5 (no mask of the device can differ from the
oracle's: nothing is excluded from a comparison), and that fp32 autograd itself sits within a quarter
of the fp32 bound.

(a) every slab row against the oracle, per parameter tensor.  fp32: ``max|g - ref| / max|ref|`` below
    2e-5, loss slot rtol 1e-4, an identically zero reference tensor exactly zero.  bf16: relative L2 at
    most 1e-3 against the bf16 model of the forward that ran and at most 1e-2 against the exact
    oracle, closer to its own forward's model than to the other one, loss slot rtol 1e-4 against that
    model's cross-entropy.
(b) row localisation, bitwise: a shard that differs in one row differs in that row's slab row only.
(c) determinism: two fresh engines give bitwise-equal slabs on every variant that takes the
    barrier-free dgrad / wgrad hand-off (lds_count_arrive / lds_count_wait).
(d) every position is written: the slab is filled with NaN patterns before the launch (in every
    test of this module); all partials and loss slots are finite afterwards, ``sat`` stays 0.
(e) the second local step (``local_steps=2``): the slab against the oracle at the first step's result.

Measured on MI355X, worst over all cases, slab rows and tensors:

    kernels, slab rows                  gradient (bound)                                   loss slot (1e-4)
    ----------------------------------  -------------------------------------------------  ----------------
    fp32, fp32 rows                     4.8e-7 (2e-5)                                      9.0e-8
    bf16, fp32 rows                     5.8e-6 to its model (1e-3), 5.5e-3 to exact (1e-2)  1.6e-7
    bf16, dense fp16 rows               3.8e-4 to its model, 8.8e-3 to exact               1.6e-7
    bf16, blocked fp16 rows             2.7e-4 to its model, 8.8e-3 to exact               1.6e-7
    bf16 plain forward, dense fp16      2.6e-4 to the plain model (the split one: 11.8 x)  7.8e-9
    second step, fp32                   2.9e-7                                             1.3e-7
    second step, bf16 fp16 rows         3.0e-4 to its model, 5.6e-3 to exact               6.7e-8

The fp16 rows' distance to their own model is the fp16 rounding of the stored partial: the host model
rounded to fp16 is 2.2e-4 to 3.8e-4 from itself on these cases, and the device lands on the same figures.
The other forward's model is at least 1.87 times as far as the own one (1.41 in the second step), 3.0
times on the blocked rows.  The 8.8e-3 to the exact oracle (95 rows of 14-50-200-2, fp16 rows) is the host
model's own distance (tests/test_train_stage_oracle_cpu.py), not the device's.

Found by (d): dense fp16 rows of a model whose P is no multiple of 8 -- every shape here but 14-50-200-2
and 14-40-16 -- left the halves [P, roundup8(P)) unwritten, which the Adam kernel reads (16-byte chunks)
and checks for saturation: over the NaN fill ``sat`` became 1.  The train kernel now completes that
chunk with zeros, as the blocked row always did.
"""
import functools

import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass
from .train_stage_oracle import (BF16_R64_CASE, LOCAL2_CASES, MIN_MARGIN, PLAIN_CASE, STAGE_CASES, case_id,
                                 fp32_tensor_error, rel_l2, stage_oracle, tensor_slices)

pytestmark = pytest.mark.gpu

ENV = ("FEDMI_SHAPE_SPEC", "FEDMI_ADAM_SPEC", "FEDMI_SLAB_BLOCKED")
# kernel variants: the switches set before construction
VARIANTS = {
    "default": {},                              # what the engine picks (the reference shape at R = 32: specialised)
    "generic": {"FEDMI_SHAPE_SPEC": "0"},       # generic train and Adam kernels
    "dense": {"FEDMI_SLAB_BLOCKED": "0"},       # specialised kernels, dense fp16 rows
    "adam_off": {"FEDMI_ADAM_SPEC": "0"},       # specialised train kernel, generic Adam kernel (dense rows)
}
REF_DIMS = (14, 50, 200, 2)
FL_WAVES = 16
BLOCKED_ROW_HALVES = 11852   # fl_layout.h FlSlabBlk::P of the reference shape (tests/test_native_slab_map.py)


def _dims(case):
    return (case[1], *case[3], case[2])


def _is_ref(case):
    return _dims(case) == REF_DIMS and case[4] == 32


def fp32_handoff(dims):
    """fl_kernels.hip wgrad_waves_fp32 < FL_WAVES on a layer l > 0: dgrad items = ceil(K / 16) on waves
    of their own when the chains are long (ceil(N / 16) >= 4) and at most half of the waves."""
    return any(-(-dims[l + 1] // 16) >= 4 and 2 * -(-dims[l] // 16) <= FL_WAVES for l in range(1, len(dims) - 1))


def bf16_handoff(dims):
    """fl_kernels_bf16.hip wgrad_waves_bf16 < FL_WAVES on a layer l > 0, on kp = roundup32(dim):
    items = kp[l] / 16, chain length kp[l + 1] / 32 >= 4."""
    kp = [(d + 31) // 32 * 32 for d in dims]
    return any(kp[l + 1] // 32 >= 4 and 2 * (kp[l] // 16) <= FL_WAVES for l in range(1, len(dims) - 1))


@functools.lru_cache(maxsize=None)
def _data(case, data_seed=DATA_SEED, init_seed=INIT_SEED):
    rows, F, C, hidden, R = case
    X, y = make_multiclass(rows, F, C, data_seed)
    flat = init_flat(list(_dims(case)), init_seed)
    for a in (X, y, flat):
        a.setflags(write=False)
    return X, y, flat


@functools.lru_cache(maxsize=None)
def _oracle(case, model, plain=False, slab="fp32"):
    X, y, flat = _data(case)
    return stage_oracle(flat, X, y, _dims(case), case[4], model, plain=plain, slab=slab)


def _launch(monkeypatch, case, dtype, slab="fp32", variant="default", X=None, y=None, flat=None, plain=False, **kw):
    """A fresh engine, its slab filled with NaN patterns, one step_train(): what the launch left."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    rows, F, C, hidden, R = case
    X0, y0, flat0 = _data(case)
    X, y, flat = (X0 if X is None else X), (y0 if y is None else y), (flat0 if flat is None else flat)
    if dtype == "bf16":
        kw["grad_slab"] = slab
    if plain:
        kw.update(fused_eval=False, plain_fwd=True)
    cfg = EngineConfig(hidden=hidden, max_rounds=4, graph_rounds=0, early_stop=False, rows_per_block=R, dtype=dtype, **kw)
    eng = HipRoundEngine(X.copy(), y.copy(), C, cfg, None, flat.copy(), emulate_clients=plain)
    lay = eng.layout
    f16 = dtype == "bf16" and slab == "fp16"
    spec = _is_ref(case) and not plain and variant != "generic"
    assert eng.R == R and lay["dtype"] == (1 if dtype == "bf16" else 0), lay
    assert int(lay["n_slabs"]) == (rows + R - 1) // R
    assert bool(lay["slab_f16"]) == f16 == eng.slab_f16, lay
    assert bool(lay["plain_fwd"]) == plain, lay
    if not plain:
        assert lay["shape_spec"] is spec, lay
    if variant == "adam_off":
        assert lay["adam_spec"] is False, lay
    blocked = bool(eng.engine.layout()["slab_blocked"])
    if int(cfg.local_steps) == 1:
        assert blocked == (spec and f16 and variant == "default"), lay
    if blocked:
        assert max(eng.engine.slab_map()) + 1 == BLOCKED_ROW_HALVES
    # (d): NaN patterns everywhere -- fp32 NaNs, or fp16 NaN halves (0x7E007E00 as a loss slot's float)
    if f16:
        eng.slab.view(torch.int16).fill_(0x7E00)
    else:
        eng.slab.fill_(float("nan"))
    torch.cuda.synchronize()
    eng.step_train()
    eng.stream.synchronize()
    out = {"part": eng.slab_partials().cpu(), "loss": eng.slab_losses().cpu(), "raw": eng.slab.view(torch.int32).cpu(),
           "sat": int(eng.sat.item()), "blocked": blocked, "f16": f16, "local": eng.local_flat(), "n": rows,
           "stride": int(eng.engine.layout()["slab_stride"]),
           "fmt": "fp32 rows" if not f16 else ("blocked fp16 rows" if blocked else "dense fp16 rows")}
    assert out["part"].shape == (int(lay["n_slabs"]), len(flat)) and out["loss"].shape == (int(lay["n_slabs"]),)
    assert out["part"].dtype == (torch.float16 if f16 else torch.float32) and out["loss"].dtype == torch.float32
    return out


_CACHE = {}


def _cached(monkeypatch, case, dtype, slab="fp32", variant="default", plain=False):
    """The first launch of a configuration on the case's own shard, shared by the tests (read-only)."""
    key = (case, dtype, slab, variant, plain)
    if key not in _CACHE:
        _CACHE[key] = _launch(monkeypatch, case, dtype, slab, variant, plain=plain)
    return _CACHE[key]


def _configs():
    """(case, dtype, slab, variant, plain) of every kernel path."""
    out = []
    for case in STAGE_CASES:
        vs = ["default", "generic"] if _is_ref(case) else ["default"]
        out += [(case, "fp32", "fp32", v, False) for v in vs]
        out += [(case, "bf16", "fp32", v, False) for v in vs]
        out += [(case, "bf16", "fp16", v, False) for v in (vs + ["dense"] if _is_ref(case) else vs)]
    out += [(BF16_R64_CASE, "bf16", s, "default", False) for s in ("fp32", "fp16")]
    out.append((PLAIN_CASE, "bf16", "fp16", "default", True))
    return out


def _cid(cfg):
    case, dtype, slab, variant, plain = cfg
    return f"{case_id(case)}-{dtype}-slab_{slab}-{variant}" + ("-plain" if plain else "")


CONFIGS = _configs()
# the specialised train kernel in front of the generic Adam kernel (dense rows)
ADAM_OFF = [(c, "bf16", "fp16", "adam_off", False) for c in STAGE_CASES if _is_ref(c) and c[0] > 32]
HANDOFF = [c for c in CONFIGS + ADAM_OFF if (fp32_handoff if c[1] == "fp32" else bf16_handoff)(_dims(c[0]))]


def _check_fp32(out, ref, dims, what):
    g, loss = out["part"].double().numpy(), out["loss"].double().numpy()
    worst = 0.0
    for b in range(len(loss)):
        for name, sl in tensor_slices(dims):
            if not np.any(ref.grad[b, sl]):
                assert not np.any(g[b, sl]), (what, b, name)
                continue
            err = fp32_tensor_error(g[b, sl], ref.grad[b, sl])
            worst = max(worst, err)
            assert err < 2e-5, (what, b, name, err)
    lerr = float(np.max(np.abs(loss - ref.loss) / ref.loss))
    print(f"STAGE {what} | {out['fmt']} | grad {worst:.3e} loss {lerr:.3e}")
    np.testing.assert_allclose(loss, ref.loss, rtol=1e-4, err_msg=what)


def _check_bf16(out, own, other, exact, dims, what):
    """``own`` / ``other``: the bf16 model of the forward that ran / of the other forward, in the slab's
    scaling.  ``exact`` is None for the plain forward, which is held to its own model only (it rounds every
    layer's input to bf16: 6.6e-2 from the exact oracle on a block of PLAIN_CASE, on the host model itself)."""
    scale = out["n"] if out["f16"] else 1   # fp16 rows: unscaled sums (the exact oracle's partials times n)
    g, loss = out["part"].double().numpy(), out["loss"].double().numpy()
    w_own = w_ex = 0.0
    w_gap = np.inf
    for b in range(len(loss)):
        for name, sl in tensor_slices(dims):
            if not np.any(own.grad[b, sl]):
                assert not np.any(g[b, sl]), (what, b, name)
                continue
            e_own = rel_l2(g[b, sl], own.grad[b, sl])
            e_ex = rel_l2(g[b, sl] / scale, exact.grad[b, sl]) if exact is not None else 0.0
            w_own, w_ex = max(w_own, e_own), max(w_ex, e_ex)
            print(f"STAGE-ROW {what} row {b} {name} own {e_own:.3e} exact {e_ex:.3e}")
            assert e_own <= 1e-3, (what, b, name, e_own)
            assert e_ex <= 1e-2, (what, b, name, e_ex)
            if np.any(own.grad[b, sl] != other.grad[b, sl]):
                e_other = rel_l2(g[b, sl], other.grad[b, sl])
                w_gap = min(w_gap, e_other / e_own if e_own else np.inf)
                assert e_own < e_other, (what, b, name, e_own, e_other)
    lerr = float(np.max(np.abs(loss - own.loss) / own.loss))
    print(f"STAGE {what} | {out['fmt']} | own {w_own:.3e} exact {w_ex:.3e} other/own {w_gap:.2f} loss {lerr:.3e}")
    np.testing.assert_allclose(loss, own.loss, rtol=1e-4, err_msg=what)


def _check(out, case, dtype, slab, plain, what, oracle=_oracle):
    dims = _dims(case)
    if dtype == "fp32":
        _check_fp32(out, oracle(case, "exact"), dims, what)
    else:
        _check_bf16(out, oracle(case, "bf16", plain, slab), oracle(case, "bf16", not plain, slab),
                    None if plain else oracle(case, "exact"), dims, what)


# ---- (a) every slab row against the oracle ----
@pytest.mark.parametrize("cfg", CONFIGS, ids=_cid)
def test_every_slab_row_matches_the_oracle(monkeypatch, cfg):
    case, dtype, slab, variant, plain = cfg
    _check(_cached(monkeypatch, *cfg), case, dtype, slab, plain, _cid(cfg))


# ---- (d) every position is written ----
@pytest.mark.parametrize("cfg", CONFIGS + ADAM_OFF, ids=_cid)
def test_nan_filled_slab_is_overwritten(monkeypatch, cfg):
    out = _cached(monkeypatch, *cfg)
    assert bool(torch.isfinite(out["part"].float()).all()), _cid(cfg)
    assert bool(torch.isfinite(out["loss"]).all()), _cid(cfg)
    if out["f16"]:  # a loss slot still holding the two NaN halves would be a finite float
        assert not bool((out["loss"].view(torch.int32) == 0x7E007E00).any()), _cid(cfg)
        assert out["sat"] == 0
    if out["f16"] and not out["blocked"]:
        # the Adam kernel reads 16-byte chunks: the dense row's halves [P, roundup8(P)) are zeros, not the fill
        ns, P = out["part"].shape
        halves = out["raw"][:ns * out["stride"]].view(ns, out["stride"]).view(torch.int16)
        assert halves.shape == (ns, 2 * out["stride"]) and not bool(halves[:, P:(P + 7) // 8 * 8].any()), _cid(cfg)


# ---- (c) determinism ----
def test_reference_shape_takes_the_barrier_free_handoff():
    """From the shapes, by the documented rules: on the 50 -> 200 layer (l = 1) the 4 dgrad items take
    waves of their own, 12 of 16 waves take wgrad tiles, and the phase ends on the LDS arrival count.
    Every variant of that shape -- specialised and generic, R = 16 and 32, the three row formats, the
    plain forward -- is therefore in the determinism test."""
    assert fp32_handoff(REF_DIMS) and bf16_handoff(REF_DIMS)
    assert not fp32_handoff((14, 50, 48, 2)) and not bf16_handoff((14, 50, 96, 2))      # short chains
    assert not fp32_handoff((14, 130, 200, 2)) and not bf16_handoff((14, 130, 200, 2))  # more than half of the waves
    ref = [c for c in CONFIGS + ADAM_OFF if _dims(c[0]) == REF_DIMS]
    assert all(c in HANDOFF for c in ref) and len(ref) >= 20
    assert {(c[1], c[2], c[3], c[4]) for c in ref} >= {
        ("fp32", "fp32", "default", False), ("fp32", "fp32", "generic", False), ("bf16", "fp32", "default", False),
        ("bf16", "fp32", "generic", False), ("bf16", "fp16", "default", False), ("bf16", "fp16", "generic", False),
        ("bf16", "fp16", "dense", False), ("bf16", "fp16", "adam_off", False), ("bf16", "fp16", "default", True)}


@pytest.mark.parametrize("cfg", HANDOFF, ids=_cid)
def test_two_fresh_engines_give_bitwise_equal_slabs(monkeypatch, cfg):
    a = _cached(monkeypatch, *cfg)
    b = _launch(monkeypatch, cfg[0], cfg[1], cfg[2], cfg[3], plain=cfg[4])
    assert torch.equal(a["raw"], b["raw"]), _cid(cfg)   # (both slabs started from the same NaN fill)
    assert torch.equal(a["part"].view(torch.int16 if a["f16"] else torch.int32),
                       b["part"].view(torch.int16 if b["f16"] else torch.int32))
    assert torch.equal(a["loss"].view(torch.int32), b["loss"].view(torch.int32))
    assert np.array_equal(a["local"], b["local"])


# ---- (b) row localisation ----
def _bits(out):
    return out["part"].view(torch.int16 if out["f16"] else torch.int32), out["loss"].view(torch.int32)


@pytest.mark.parametrize("variant", ["default", "generic"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rows", [33, 95])
def test_one_changed_row_changes_one_slab_row(monkeypatch, rows, dtype, variant):
    case = (rows, 14, 2, (50, 200), 32)
    slab = "fp16" if dtype == "bf16" else "fp32"
    X, y, _ = _data(case)
    base = _bits(_cached(monkeypatch, case, dtype, slab, variant))
    # the last live row of the partial block; the first row of the second block (at 33 rows: the same row)
    for row in sorted({rows - 1, 32}):
        X2, y2 = X.copy(), y.copy()
        X2[row] = -X[row] + 0.25
        y2[row] = 1 - y[row]
        got = _bits(_launch(monkeypatch, case, dtype, slab, variant, X=X2, y=y2))
        for b in range(base[0].shape[0]):
            same_g, same_l = torch.equal(got[0][b], base[0][b]), torch.equal(got[1][b], base[1][b])
            if b == row // 32:
                assert not same_g and not same_l, (row, b)
            else:
                assert same_g and same_l, (row, b)
    if rows == 33:
        # block 1 is one row: its slab row depends on that row and n alone -- another block 0, the same n
        Xo, yo = make_multiclass(32, 14, 2, DATA_SEED + 1)
        X3, y3 = X.copy(), y.copy()
        X3[:32], y3[:32] = Xo, yo
        got = _bits(_launch(monkeypatch, case, dtype, slab, variant, X=X3, y=y3))
        assert torch.equal(got[0][1], base[0][1]) and torch.equal(got[1][1], base[1][1])
        assert not torch.equal(got[0][0], base[0][0]) and not torch.equal(got[1][0], base[1][0])


# ---- (e) the second local step ----
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", LOCAL2_CASES, ids=case_id)
def test_second_local_step_matches_the_oracle_at_the_first_steps_result(monkeypatch, case, dtype):
    slab = "fp16" if dtype == "bf16" else "fp32"
    X, y, flat = _data(case)
    twin = _launch(monkeypatch, case, dtype, slab, local_steps=1, prox_mu=0.0)
    first = _cached(monkeypatch, case, dtype, slab)   # the same first launch on the same inputs
    assert torch.equal(twin["raw"], first["raw"]) and np.array_equal(twin["local"], first["local"])
    w1 = twin["local"]
    assert w1.dtype == np.float32 and np.all(np.isfinite(w1)) and not np.array_equal(w1, flat)
    out = _launch(monkeypatch, case, dtype, slab, local_steps=2, prox_mu=0.0)
    assert not torch.equal(out["raw"], first["raw"])

    @functools.lru_cache(maxsize=None)
    def at_w1(case, model, plain=False, slab="fp32"):
        return stage_oracle(w1, X, y, _dims(case), case[4], model, plain=plain, slab=slab)

    margin = at_w1(case, "exact" if dtype == "fp32" else "bf16", False, slab).margin
    print(f"STAGE-MARGIN local2 {case_id(case)} {dtype} {margin:.3e}")
    assert margin >= MIN_MARGIN, margin
    _check(out, case, dtype, slab, False, f"local2-{case_id(case)}-{dtype}", oracle=at_w1)
    if dtype == "bf16":
        assert out["sat"] == 0

"""The three main loops of gemm_nt_bf16.hip (128x128 variants 0 / 1, 256x256 half-line variant 2,
full-line variants 3 / 10) element by element against the float64 model of wide_oracle.nt_gemm.

Conventions (those of test_layered_ops.py): seeded bf16 operands with lda = K + 8 and ldb = K + 16
whose pads hold NaN; every output over-allocated (ldc = N + 3, ldcb = N + 8, ldct = M + 8,
ldcs = N + 1, a sentinel tail) and pre-filled -- with NaN for an fp32 output that beta = 0 must
not read, with a sentinel otherwise -- and everything a launch does not own keeps its bits.

Tolerances.  fp32 outputs: ``lo.nerr`` against the float64 model, in units of
|alpha| sum_k |a||b| + |bias| + |beta C0|, within ``lo.bound`` (4x) of the error of the k-ordered
fp32 transcription, the largest over ALL of this file's cases (``e_tr``; the fixture computes it
before any kernel runs, so the kernel has no part in it).  A bf16 output written next to an fp32
one is bit-equal to bf16 of that fp32 output.  A bf16 output alone lies in
[bf16(f(ref - E)), bf16(f(ref + E))], E = bound * scale, f the ReLU / mask step: rounding and f are
monotone, so no correct fp32 value within E of the model can leave the interval.  Column sums:
the lane adds its 32 rows in order, then two xor-shuffle adds: 34 fp32 additions on one path, so
|err| <= 34 * 2^-24 * sum |terms| (1.001: second-order terms), against the float64 sums of the
bf16 output read back."""
import numpy as np
import pytest
import torch

from fedmi.ops import native

from . import layered_oracle as lo
from . import wide_oracle as wo
from .test_layered_ops import SENT, TAIL, _s, assert_untouched, bits, dbuf, put2d, region, to_dev

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")

SHAPES_128 = [(128, 128, 64), (256, 128, 64), (128, 384, 128), (384, 384, 192)]
SHAPES_256 = [(256, 256, 64), (256, 256, 128), (256, 256, 192), (512, 256, 256), (768, 768, 64), (1280, 512, 64),
              (1536, 768, 64), (2304, 256, 64)]
ALL_CONFIG_SHAPES = [(256, 256, 128), (512, 256, 256)]

# name -> outputs / epilogue of one launch
CONFIGS = {
    "cb": dict(Cb=1),
    "fwd": dict(Cb=1, CbT=1, bias=1, relu=1),
    "fwd_not": dict(Cb=1, bias=1, relu=1, alpha=0.5),
    "dgrad": dict(Cb=1, CbT=1, mask=1),
    "dgrad_cs": dict(Cb=1, CbT=1, mask=1, csum=1, alpha=0.5),
    "dgrad_not": dict(Cb=1, mask=1),
    "c": dict(C=1),
    "wgrad1": dict(C=1, beta=1.0),
    "wgrad.5": dict(C=1, beta=0.5, alpha=0.5),
    "logits": dict(C=1, bias=1),
    "all": dict(C=1, Cb=1, CbT=1, bias=1, relu=1),          # run-time epilogue
    "c_mask": dict(C=1, mask=1, alpha=0.3),                  # run-time epilogue
}
EVERY_SHAPE = ["fwd", "dgrad_cs", "wgrad1", "wgrad.5"]


def configs_of(shape):
    return list(CONFIGS) if shape in ALL_CONFIG_SHAPES else EVERY_SHAPE


def variants_of(shape):
    M, N, _ = shape
    return (2, 3, 10, 0, 1) if M % 256 == 0 and N % 256 == 0 else (0, 1)


MASK_SPECIALS = np.array([0.0, -0.0, -1.5, 2.0 ** -126, np.inf, -np.inf, np.nan], dtype=F32)


def make_inputs(shape):
    M, N, K = shape
    rng = np.random.RandomState(M * 7 + N * 3 + K)
    A, B = lo.bf16_round(rng.randn(M, K).astype(F32)), lo.bf16_round(rng.randn(N, K).astype(F32))
    mask = lo.bf16_round(rng.randn(M, N).astype(F32))
    where = rng.permutation(M * N)[:8 * len(MASK_SPECIALS)]
    mask.ravel()[where] = np.tile(MASK_SPECIALS, 8)
    mask[0, :7], mask[M - 1, N - 7:] = MASK_SPECIALS, MASK_SPECIALS       # first and last tile corners
    return dict(A=A, B=B, bias=rng.randn(N).astype(F32), mask=mask, C0=rng.randn(M, N).astype(F32))


def model(inp, prod, cfg):
    return wo.nt_gemm(inp["A"], inp["B"], cfg.get("alpha", 1.0), inp["bias"] if cfg.get("bias") else None,
                      bool(cfg.get("relu")), inp["mask"] if cfg.get("mask") else None, cfg.get("beta", 0.0),
                      inp["C0"], prod=prod, pre=True)


@pytest.fixture(scope="module")
def cases():
    """Inputs and the epilogue-independent products of every shape, and e_tr: the largest
    transcription error over every (shape, configuration) this file runs."""
    data, e_tr = {}, 0.0
    for shape in SHAPES_128 + SHAPES_256:
        inp = make_inputs(shape)
        prod = wo.nt_product(inp["A"], inp["B"])
        data[shape] = (inp, prod)
        for name in configs_of(shape):
            ref, tr, scale, _ = model(inp, prod, CONFIGS[name])
            e = lo.nerr(tr, ref, scale)
            assert 0.0 < e < shape[2] * 2.0 ** -24
            e_tr = max(e_tr, e)
    return data, e_tr


@pytest.fixture(scope="module")
def m():
    return native()


class Launch:
    """The device buffers of one launch.  ``mis``: one misalignment of the fallback tests."""

    def __init__(self, inp, shape, cfg, mis=None, lda_extra=8, ldb_extra=16):
        M, N, K = shape
        self.shape, self.cfg = shape, cfg
        self.lda, self.ldb = K + lda_extra, K + ldb_extra
        self.ldc, self.ldcb, self.ldct, self.ldmask, self.ldcs = N + 3, N + 8, M + 8, N + 8, N + 1
        self.off = dict(Cb=0, CbT=0, mask=0)
        if mis == "ldct":
            self.ldct = M + 2
        elif mis == "CbT":
            self.off["CbT"] = 2
        elif mis == "ldmask":
            self.ldmask = N + 4
        elif mis == "mask":
            self.off["mask"] = 4
        elif mis == "ldcb":
            self.ldcb = N + 4
        elif mis == "Cbf16":
            self.off["Cb"] = 4
        self.A = put2d(inp["A"], self.lda, torch.bfloat16)
        self.B = put2d(inp["B"], self.ldb, torch.bfloat16)
        self.bias = to_dev(inp["bias"]) if cfg.get("bias") else None
        self.mask = None
        if cfg.get("mask"):
            o = self.off["mask"]
            self.mask = dbuf(o + M * self.ldmask + TAIL, torch.bfloat16, NAN)
            self.mask[o:o + M * self.ldmask].view(M, self.ldmask)[:, :N] = to_dev(inp["mask"]).to(torch.bfloat16)
        beta = cfg.get("beta", 0.0)
        self.C = self.Cb = self.CbT = self.cs = None
        if cfg.get("C"):
            self.C = put2d(inp["C0"], self.ldc, fill=SENT) if beta != 0.0 else dbuf(M * self.ldc + TAIL, fill=NAN)
        if cfg.get("Cb"):
            self.Cb = dbuf(self.off["Cb"] + M * self.ldcb + TAIL, torch.bfloat16)
        if cfg.get("CbT"):
            self.CbT = dbuf(self.off["CbT"] + N * self.ldct + TAIL, torch.bfloat16)
        if cfg.get("csum"):
            self.cs = dbuf((M // 128) * self.ldcs + TAIL)
        self.before = {k: bits(t) for k, t in self.outputs().items()}

    def outputs(self):
        return {k: t for k, t in (("C", self.C), ("Cb", self.Cb), ("CbT", self.CbT), ("cs", self.cs)) if t is not None}

    def owned(self, k):
        M, N, _ = self.shape
        t = self.outputs()[k]
        rows, ld, cols, off = {"C": (M, self.ldc, N, 0), "Cb": (M, self.ldcb, N, self.off["Cb"]),
                               "CbT": (N, self.ldct, M, self.off["CbT"]), "cs": (M // 128, self.ldcs, N, 0)}[k]
        return region(t.numel(), off, rows, ld, cols), (rows, ld, cols, off)

    def run(self, m, shape=None, lda=None, ldb=None, csum=True):
        M, N, K = shape or self.shape
        p = lambda t, o=0: t[o:].data_ptr() if t is not None else 0
        cs = self.cs if csum else None
        m.gemm_nt(M, N, K, p(self.A), lda or self.lda, p(self.B), ldb or self.ldb, p(self.C), self.ldc,
                  p(self.Cb, self.off["Cb"]), self.ldcb, p(self.CbT, self.off["CbT"]), self.ldct, p(self.bias),
                  p(self.mask, self.off["mask"]), self.ldmask, int(bool(self.cfg.get("relu"))),
                  self.cfg.get("alpha", 1.0), self.cfg.get("beta", 0.0), _s(), p(cs), self.ldcs)

    def read(self, csum=True):
        """Owned regions as bit arrays after the untouched check -> {name: [rows][cols] bits}."""
        got = {}
        for k, t in self.outputs().items():
            own, (rows, ld, cols, off) = self.owned(k)
            if k == "cs" and not csum:
                own = np.zeros_like(own)
            assert_untouched(t, self.before[k], own, f"{k} {self.shape} {self.cfg}")
            got[k] = np.ascontiguousarray(bits(t)[off:off + rows * ld].reshape(rows, ld)[:, :cols])
        return got

    def assert_all_untouched(self):
        for k, t in self.outputs().items():
            assert_untouched(t, self.before[k], np.zeros(t.numel(), dtype=bool), f"{k} after a rejected launch")


def bf16_val(b):
    return (b.view(np.uint16).astype(np.uint32) << 16).view(F32)


def check_against_model(got, inp, prod, cfg, tb, what):
    """Every assertion on one launch's outputs -> the fp32 output's error (None without one)."""
    ref, _, scale, before = model(inp, prod, cfg)
    err = None
    if "C" in got:
        c = got["C"].view(F32)
        assert np.isfinite(c).all(), f"{what}: non-finite fp32 output"
        err = lo.nerr(c, ref, scale)
        assert err <= tb, f"{what}: fp32 output err {err:.3e} > bound {tb:.3e}"
    if "Cb" in got:
        cb = bf16_val(got["Cb"])
        assert np.isfinite(cb).all(), f"{what}: non-finite bf16 output"
        if "C" in got:
            np.testing.assert_array_equal(got["Cb"].view(np.uint16), lo.bf16_bits(got["C"].view(F32)),
                                          err_msg=f"{what}: Cb is not bf16 of C")
        else:
            keep = wo.keep_of(inp["mask"]) if cfg.get("mask") else None
            lo_, hi = wo.bf16_interval(before, tb * scale, bool(cfg.get("relu")), keep)
            bad = np.flatnonzero(~((cb >= lo_) & (cb <= hi)).ravel())
            assert bad.size == 0, (f"{what}: {bad.size} bf16 elements outside their interval, first {bad[:4]}: got "
                                   f"{cb.ravel()[bad[:4]]} lo {lo_.ravel()[bad[:4]]} hi {hi.ravel()[bad[:4]]}")
    if "CbT" in got:
        np.testing.assert_array_equal(got["CbT"], got["Cb"].T, err_msg=f"{what}: CbT is not Cb^T")
    if "cs" in got:
        want, sabs = wo.nt_csum(bf16_val(got["Cb"]))
        cs = got["cs"].view(F32)
        assert np.isfinite(cs).all()
        assert (np.abs(cs.astype(np.float64) - want) <= 1.001 * 34 * 2.0 ** -24 * sabs).all(), f"{what}: column sums"
    return err


def run_shape(m, cases, shape, group):
    (inp, prod), e_tr = cases[0][shape], cases[1]
    tb = lo.bound(e_tr)
    worst = 0.0
    try:
        for name in configs_of(shape):
            cfg = CONFIGS[name]
            first = None
            for v in variants_of(shape):
                m.gemm_nt_set_variant(v)
                csum = v in (2, 3, 10)                      # the 128x128 loop has no column sums
                L = Launch(inp, shape, cfg)
                L.run(m, csum=csum)
                got = L.read(csum=csum)
                if not csum:
                    got.pop("cs", None)
                err = check_against_model(got, inp, prod, cfg, tb, f"{shape} {name} v{v}")
                if err is not None:
                    worst = max(worst, err)
                    print(f"gemm_nt {shape} {name} v{v}: err {err:.3e} (transcription max {e_tr:.3e}) bound {tb:.3e}")
                if first is None:
                    first = (v, got)
                for k, g in got.items():
                    if k in first[1]:
                        np.testing.assert_array_equal(g, first[1][k], err_msg=f"{shape} {name} {k}: v{v} != v{first[0]}")
    finally:
        m.gemm_nt_set_variant(3)
    print(f"gemm_nt {group} {shape}: worst err / bound = {worst / tb:.3f}")


@pytest.mark.parametrize("shape", SHAPES_128, ids=lambda s: "x".join(map(str, s)))
def test_gemm_nt_128_loop(m, cases, shape):
    """Single- and double-buffered 128x128 loops: one tile and one K-tile, two m-tiles, three
    n-tiles over two K-tiles, and 9 tiles (XCD remap with remainder 1) over three K-tiles."""
    run_shape(m, cases, shape, "128x128")


@pytest.mark.parametrize("shape", SHAPES_256, ids=lambda s: "x".join(map(str, s)))
def test_gemm_nt_256_loops(m, cases, shape):
    """Half-line, full-line (buffer and global DMAs) and both 128x128 loops, bit-identical: one,
    two, three and four K-tiles; mt = 3 (one short group), 5 (last group of one), 6 (18 tiles), 9
    with nt = 1."""
    run_shape(m, cases, shape, "256x256")


MISALIGNED = ["ldct", "CbT", "ldmask", "mask", "ldcb", "Cbf16"]


@pytest.mark.parametrize("mis", MISALIGNED)
def test_gemm_nt_fallback_to_128_loop(m, cases, mis):
    """One operand of the 256x256 epilogue's vector accesses misaligned: variant 3 silently takes
    the 128x128 loop -- the same bits as variant 1 on the same buffers, and the model's bounds."""
    shape = (256, 256, 128)
    (inp, prod), e_tr = cases[0][shape], cases[1]
    cfg = CONFIGS["dgrad"]
    got = {}
    try:
        for v in (3, 1):
            m.gemm_nt_set_variant(v)
            L = Launch(inp, shape, cfg, mis=mis)
            L.run(m)
            got[v] = L.read()
            check_against_model(got[v], inp, prod, cfg, lo.bound(e_tr), f"{mis} v{v}")
    finally:
        m.gemm_nt_set_variant(3)
    for k in got[1]:
        np.testing.assert_array_equal(got[3][k], got[1][k], err_msg=f"{mis}: {k}")


@pytest.mark.parametrize("mis", MISALIGNED)
def test_gemm_nt_column_sums_refuse_the_fallback(m, cases, mis):
    """The 128x128 loop has no column sums: the misaligned launch raises and writes nothing."""
    shape = (256, 256, 128)
    L = Launch(cases[0][shape][0], shape, CONFIGS["dgrad_cs"], mis=mis)
    with pytest.raises(RuntimeError):
        L.run(m)
    torch.cuda.synchronize()
    L.assert_all_untouched()


@pytest.mark.parametrize("bad", ["M", "N", "K", "lda", "ldb"])
def test_gemm_nt_guards(m, cases, bad):
    """M % 128, N % 128, K % 64, lda % 8, ldb % 8: RuntimeError, outputs untouched (the buffers are
    those of the valid 256 x 256 x 128 launch, which every rejected size fits in)."""
    shape = (256, 256, 128)
    L = Launch(cases[0][shape][0], shape, CONFIGS["all"])
    kw = {"M": dict(shape=(192, 256, 128)), "N": dict(shape=(256, 192, 128)), "K": dict(shape=(256, 256, 96)),
          "lda": dict(lda=L.lda - 4), "ldb": dict(ldb=L.ldb - 4)}[bad]
    with pytest.raises(RuntimeError):
        L.run(m, **kw)
    torch.cuda.synchronize()
    L.assert_all_untouched()

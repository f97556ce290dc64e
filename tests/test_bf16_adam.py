"""The bf16 engines' Adam kernel against float64 Adam on the kernel's own gradient, and the packed
hi/lo image it writes against the stand-alone pack.

The fp32 engines' Adam step is held to the torch oracle (tests/test_hip_engine_shapes.py); the
bf16 engines' instantiations -- fp16 slab with the 1/n deferred to after the reduction, fp32 slab,
the packed local image written beside the fp32 step -- were only compared with each other
(tests/test_adam_spec.py).  Here each of three step-API rounds reads (w, exp_avg, exp_avg_sq)
before the round, runs the train and Adam kernels, forms g from the gradient slab the Adam kernel
reduced (summed in float64; divided by n for the fp16 slab), applies one float64 torch.optim.Adam
step under a StepLR that steps inside the run (step_size 2, gamma 0.3: the bias correction sees
t = 1..3 and two learning rates) and compares the new weights and moments: nerr = max|a - b| /
max|b| < 2e-5 each, the fp32 engine's bound.  Taking g from the device isolates the Adam kernel from
the bf16 gradient's own noise.

Shards of R + 1, 3 R - 1 and 129 R + 4 rows at R = 32 (130 slab rows: the second 16-byte load of a
wave in the slab reduction), both slab formats; 14-50-200-2 (the specialised Adam kernel, and the
generic one under FEDMI_ADAM_SPEC=0), 14-33-17-9-5 and 1-16-2; weight decay once per slab format.

Measured on MI355X, worst nerr over all cases and rounds: weights 4.6e-7 (fp16 slab) / 3.0e-7 (fp32
slab), exp_avg 1.2e-7 / 1.4e-7, exp_avg_sq 3.1e-7 / 2.2e-7."""
import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.models.mlp import image_to_dense, init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr

pytestmark = pytest.mark.gpu

R = 32
REF = (14, 50, 200, 2)
STEPLR = dict(step_size=2, gamma=0.3)
SHAPES = [(REF, True), (REF, False), ((14, 33, 17, 9, 5), True), ((1, 16, 2), True)]   # (dims, FEDMI_ADAM_SPEC unset)
ROWS = [R + 1, 3 * R - 1, 129 * R + 4]


def _engine(dims, rows, slab, **kw):
    X, y = make_multiclass(rows, dims[0], dims[-1], DATA_SEED)
    cfg = EngineConfig(hidden=tuple(dims[1:-1]), max_rounds=6, early_stop=False, graph_rounds=0, rows_per_block=R,
                       dtype="bf16", grad_slab=slab, **kw)
    e = HipRoundEngine(X, y, dims[-1], cfg, None, init_flat(list(dims), INIT_SEED))
    assert e.R == R and e.slab_f16 == (slab == "fp16") and int(e.layout["n_slabs"]) == (rows + R - 1) // R
    return e


def _moments(e):
    e.stream.synchronize()
    return image_to_dense(e.mom.cpu().numpy(), e.dims), image_to_dense(e.vel.cpu().numpy(), e.dims)


def _check_adam_rounds(e, rows, what, rounds=3):
    cfg = e.cfg
    p = torch.zeros(e.P, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=cfg.lr, betas=tuple(cfg.betas), eps=cfg.eps, weight_decay=cfg.weight_decay)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=cfg.step_size, gamma=cfg.gamma)
    worst = {"weights": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    lrs = []
    for r in range(rounds):
        w = e.global_flat()
        if r:
            st = e.portable_state()
            assert st["opt_steps"] == r and st["history"]["rounds_run"] == r
        else:   # nothing to fold before the first round: the buffers as they were allocated
            st = dict(zip(("exp_avg", "exp_avg_sq"), _moments(e)))
        assert np.array_equal(w, e.local_flat())
        e.step_train()
        e.stream.synchronize()
        g = e.slab_partials().double().sum(0).cpu()
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        if e.slab_f16:   # partial sums of the unscaled gradient: the Adam kernel applies the 1/n
            g = g / rows
        with torch.no_grad():
            p.copy_(torch.as_tensor(w, dtype=torch.float64))
            if r:
                opt.state[p]["exp_avg"].copy_(torch.as_tensor(st["exp_avg"], dtype=torch.float64))
                opt.state[p]["exp_avg_sq"].copy_(torch.as_tensor(st["exp_avg_sq"], dtype=torch.float64))
            else:
                assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
        p.grad = g.clone()
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        m, v = _moments(e)
        err = {"weights": nerr(e.local_flat(), p.detach().numpy()),
               "exp_avg": nerr(m, opt.state[p]["exp_avg"].numpy()),
               "exp_avg_sq": nerr(v, opt.state[p]["exp_avg_sq"].numpy())}
        print("ADAM", what, "round", r, "lr", lrs[-1], err)
        for k in worst:
            worst[k] = max(worst[k], err[k])
            assert err[k] < 2e-5, (what, r, err)
        assert np.abs(e.local_flat() - w).max() > 0.1 * lrs[-1]   # a step was taken
        e.step_eval()
        e.step_aggregate()
    assert len(set(lrs)) == 2, lrs   # the LR changed inside the run
    assert not e.slab_saturated and int(e.sat.item()) == 0
    return worst


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("slab", ["fp16", "fp32"])
@pytest.mark.parametrize("dims,spec", SHAPES, ids=["ref-spec", "ref-generic", "14-33-17-9-5", "1-16-2"])
def test_bf16_adam_step_matches_float64_adam(dims, spec, slab, rows, monkeypatch):
    if spec:
        monkeypatch.delenv("FEDMI_ADAM_SPEC", raising=False)
    else:
        monkeypatch.setenv("FEDMI_ADAM_SPEC", "0")
    e = _engine(dims, rows, slab, **STEPLR)
    assert e.layout["adam_spec"] is (spec and dims == REF), e.layout
    _check_adam_rounds(e, rows, f"{'-'.join(map(str, dims))} spec={spec} {slab} rows={rows}")


@pytest.mark.parametrize("slab", ["fp16", "fp32"])
def test_bf16_adam_step_with_weight_decay(slab):
    e = _engine(REF, 3 * R - 1, slab, weight_decay=1e-2, **STEPLR)
    assert e.layout["adam_spec"] is True
    _check_adam_rounds(e, 3 * R - 1, f"weight_decay {slab}")


def _bf16_bits(x):
    """Bit patterns (uint16) of the fp32 array's round-to-nearest-even bf16 values."""
    return torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("dims", [REF, (14, 33, 17, 9, 5), (33, 65, 3)], ids=["ref", "14-33-17-9-5", "33-65-3"])
def test_adam_packed_image_is_the_standalone_pack(dims):
    """The image a one-client round stages is the one the Adam kernel of the round before packed
    beside its fp32 step (FLEngine.packed_local): after two rounds it is byte for byte what the
    stand-alone pack kernel makes of the same fp32 weights (a fresh engine initialised from
    local_flat(); its first round packs its input, FLEngine.packed_global).  The image is
    [W hi | fp32 biases | W lo] with each lo element layout()["wlo_delta"] bytes behind its hi
    element: the (hi, lo) pairs of the weights are exactly the pairs (bf16(x), bf16(x - bf16(x)))
    of the fp32 weights x, in whatever order the layout holds them, every other pair is padding
    (0, 0), and the bias region holds the fp32 biases."""
    X, y = make_multiclass(3 * R - 1, dims[0], dims[-1], DATA_SEED)
    mk = lambda flat: HipRoundEngine(X, y, dims[-1], EngineConfig(hidden=tuple(dims[1:-1]), max_rounds=4,
                                                                  early_stop=False, graph_rounds=0, rows_per_block=R,
                                                                  dtype="bf16"), None, flat)
    e = mk(init_flat(list(dims), INIT_SEED))
    assert e.engine.fused
    e.run(2)
    w = e.local_flat()
    assert np.abs(w - init_flat(list(dims), INIT_SEED)).max() > 1e-3
    got = e.engine.packed_local(e.stream.cuda_stream)
    f = mk(w)
    f.run(1)   # its first round runs the stand-alone pack of the image it was initialised from
    want = f.engine.packed_global(f.stream.cuda_stream)
    lay = e.layout
    delta, nbytes = int(lay["wlo_delta"]), int(lay["param_bytes"])
    assert len(got) == len(want) == nbytes and 0 < delta < nbytes
    assert got == want
    # hi / lo taken apart: [0, nbytes - delta) hi images, [nbytes - delta, delta) biases, [delta, nbytes) lo images
    raw = np.frombuffer(want, np.uint8)
    hi_bytes = nbytes - delta
    hi, lo = raw[:hi_bytes].view(np.uint16), raw[delta:].view(np.uint16)
    assert hi.shape == lo.shape
    dense_w, dense_b = [], []
    off = 0
    for l in range(len(dims) - 1):
        dense_w.append(w[off:off + dims[l] * dims[l + 1]])
        off += dims[l] * dims[l + 1]
        dense_b.append(w[off:off + dims[l + 1]])
        off += dims[l + 1]
    x = np.concatenate(dense_w)
    x_hi = _bf16_bits(x)
    x_lo = _bf16_bits(x - _bf16_value(x_hi))
    assert (x_lo != 0).mean() > 0.9   # the lo parts are there to be checked
    # per element pair: lo == bf16(x - float(hi)) needs x, so pair by pair as multisets
    pairs = lambda h, l: np.sort((h.astype(np.uint32) << 16) | l.astype(np.uint32))
    packed = pairs(hi, lo)
    packed = packed[packed != 0]
    expect = pairs(x_hi, x_lo)
    np.testing.assert_array_equal(packed, expect[expect != 0])
    # the fp32 biases sit between the images, in layer order, zero-padded
    bias = raw[hi_bytes:delta].view(np.float32)
    b = np.concatenate(dense_b)
    np.testing.assert_array_equal(bias[bias != 0], b[b != 0])

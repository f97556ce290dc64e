"""The exchanged epilogues of the specialised bf16 train kernel (fl_layout.h fl_epi_*) against the generic ones.

The reference 14-50-200-2 MLP at R = 32, bf16: an engine constructed with the switches unset runs the
specialised train kernel with ``layout["epi_exchange"]`` True -- the hidden layers' forward tiles and the dgrad
tiles are computed with the two MFMA operands exchanged, so a lane holds 4 consecutive columns of one row,
rounds them two per hardware conversion and stores 8 bytes to LDS.  Engines under ``FEDMI_EPI_EXCHANGE=0``
(the same kernel with the generic epilogues) and ``FEDMI_SHAPE_SPEC=0`` (generic kernels) keep the 2-byte
stores of software-rounded values.  The LDS images are meant to be the same bytes, so everything must agree
BITWISE (``torch.equal`` / ``np.array_equal``, no tolerance): the gradient partials of one train launch, and
after 3 rounds the local and global weights, both Adam moments, both packed bf16 images and the loss and
metric history.  Shards where row masking and tile edges can go wrong: 5 rows (one partial workgroup), 33
(the second workgroup has one row) and 95 (3 R - 1).  ``grad_slab="fp16"`` runs the blocked-row instantiation
of the kernel, ``grad_slab="fp32"`` the dense fp32 one."""
import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, HipRoundEngine
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass

pytestmark = pytest.mark.gpu

DIMS = (14, 50, 200, 2)
ROWS = [5, 33, 95]
ROUNDS = 3
ENV = ("FEDMI_SHAPE_SPEC", "FEDMI_ADAM_SPEC", "FEDMI_SLAB_BLOCKED", "FEDMI_EPI_EXCHANGE")
# switches of the three engines: exchanged epilogues, the same kernel without them, generic kernels
VARIANTS = {"exchange": {}, "epi_off": {"FEDMI_EPI_EXCHANGE": "0"}, "shape_off": {"FEDMI_SHAPE_SPEC": "0"}}
_DATA = {}


def _engine(monkeypatch, variant, rows, grad_slab):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    if rows not in _DATA:
        _DATA[rows] = make_multiclass(rows, DIMS[0], DIMS[-1], DATA_SEED)
    X, y = _DATA[rows]
    cfg = EngineConfig(hidden=DIMS[1:-1], max_rounds=ROUNDS + 2, rows_per_block=32, graph_rounds=0, dtype="bf16",
                       grad_slab=grad_slab, early_stop=False)
    eng = HipRoundEngine(X, y, DIMS[-1], cfg, None, init_flat(list(DIMS), INIT_SEED))
    lay = eng.engine.layout()
    assert eng.R == 32 and eng.slab_f16 is (grad_slab == "fp16")
    assert lay["shape_spec"] is (variant != "shape_off"), (variant, lay)
    assert lay["epi_exchange"] is (variant == "exchange"), (variant, lay)
    # fp16 rows: blocked under the specialised pair (with or without the exchanged epilogues), else dense
    assert lay["slab_blocked"] is (grad_slab == "fp16" and variant != "shape_off"), (variant, lay)
    return eng


def _state(eng):
    st = eng.portable_state()
    h = eng.history()
    s = eng.stream.cuda_stream
    return {"local": st["local"], "global": st["global"], "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"],
            "local_image": eng.local.cpu().numpy(), "m_image": eng.mom.cpu().numpy(), "v_image": eng.vel.cpu().numpy(),
            "packed_local": np.frombuffer(eng.engine.packed_local(s), np.uint8),
            "packed_global": np.frombuffer(eng.engine.packed_global(s), np.uint8),
            "loss": h["loss"], "hist_global": h["global"], "hist_rank": h["per_rank"],
            "rounds_run": np.asarray(h["rounds_run"]), "sat": np.asarray(int(eng.sat.item()))}


def _compare(monkeypatch, rows, grad_slab):
    part, out = {}, {}
    for v in VARIANTS:
        eng = _engine(monkeypatch, v, rows, grad_slab)
        eng.run(1)  # one train launch (and its Adam launch, which only reads the slab)
        eng.stream.synchronize()
        part[v] = eng.slab_partials()
        assert part[v].shape == ((rows + 31) // 32, eng.P)
        assert part[v].dtype == (torch.float16 if grad_slab == "fp16" else torch.float32)
        eng.run(ROUNDS - 1)
        out[v] = _state(eng)
    assert bool(torch.isfinite(part["exchange"].float()).all()) and bool((part["exchange"] != 0).any())
    for v in ("epi_off", "shape_off"):
        assert torch.equal(part["exchange"], part[v]), v
        for k in out["exchange"]:
            assert np.array_equal(out["exchange"][k], out[v][k]), (v, k, out["exchange"][k], out[v][k])
    assert int(out["exchange"]["rounds_run"]) == ROUNDS and int(out["exchange"]["sat"]) == 0
    assert np.all(np.isfinite(out["exchange"]["global"])) and np.all(np.isfinite(out["exchange"]["loss"]))


@pytest.mark.parametrize("rows", ROWS)
def test_exchanged_epilogues_equal_generic_bitwise_fp16_slab(monkeypatch, rows):
    _compare(monkeypatch, rows, "fp16")


def test_exchanged_epilogues_equal_generic_bitwise_fp32_slab(monkeypatch):
    _compare(monkeypatch, 33, "fp32")

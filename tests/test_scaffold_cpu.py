"""SCAFFOLD on the CPU: the numpy models against float64, the torch group (the specification) against the float64
group oracle, the refusals at construction, the config record, and the planner's record."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, HipRoundEngine, TorchRoundEngine
from fedmi.fl.scaffold import scaffold_capture_model, scaffold_fold_model
from fedmi.fl.simulate import SimRank

from .reference_oracle import nerr
from .scaffold_oracle import scaffold_group, scaffold_group_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
X0, Y0, FLAT0 = np.zeros((40, 14), np.float32), np.zeros(40, np.int64), np.zeros(14 * 4 + 4 + 4 * 2 + 2, np.float32)


@pytest.mark.parametrize("n_blk", [1, 17, 33])
def test_numpy_models_against_float64(n_blk):
    rng = np.random.default_rng(n_blk)
    rows = (rng.standard_normal((n_blk, 507)) * 10.0 ** rng.integers(-3, 2, (n_blk, 1))).astype(np.float32)
    c, ci = rng.standard_normal((2, 507)).astype(np.float32)
    g, delta, corr = scaffold_capture_model(rows, c, ci)
    # n_blk terms through at most n_blk / 16 + 16 additions each: (n_blk + 16) u sum|terms| bounds the sum's error
    assert (np.abs(g - rows.astype(np.float64).sum(0)) <= (n_blk + 16) * U * np.abs(rows).astype(np.float64).sum(0)).all()
    assert g.dtype == np.float32 and np.array_equal(delta, g - ci) and np.array_equal(corr, c - ci)
    deltas = rng.standard_normal((5, 507)).astype(np.float32)
    deltas[1] = np.inf
    on = [True, False, True, True, False]
    ref = c.astype(np.float64) + deltas[on].astype(np.float64).sum(0) / 5.0
    assert np.abs(scaffold_fold_model(c, deltas, on, 5) - ref).max() <= 8 * U * np.abs(ref).max()


@pytest.mark.parametrize("local_steps,participation", [(1, 1.0), (3, 0.5)])
def test_torch_group_against_float64_oracle(local_steps, participation):
    """Six rounds at 17-24-3: weights, c and every c_i within a quarter of the project's 2e-5 (the convention for a
    reference) of the float64 group oracle."""
    torch.set_num_threads(1)
    tg = scaffold_group("torch", "small", local_steps, participation)
    tg.run(6)
    w, c, ci = scaffold_group_f64(tg, "small", 6)
    err = [nerr(tg.global_flat(), w), nerr(tg.clients[0].scaffold_variates()[0], c)]
    err += [nerr(e.scaffold_variates()[1], r) for e, r in zip(tg.clients, ci)]
    assert max(err) <= 5e-6 and np.abs(c).max() > 1e-3 and tg.history()["scaffold_norm"].shape == (6,), err


@pytest.mark.parametrize("kw,word", [
    (dict(dtype="bf16"), "bf16"), (dict(dpsgd_clip=1.0), "dpsgd_clip"), (dict(dp_clip=1.0), "dp_clip"),
    (dict(secagg=True, secagg_seed=1), "secagg"), (dict(aggregator="median"), "aggregator"),
    (dict(screen="multi_krum"), "screen"), (dict(attack="sign_flip", attack_clients=(1,)), "attack"),
    (dict(compress="sign"), "compress")])
def test_construction_refuses_and_names_the_conflict(kw, word):
    cfg = EngineConfig(hidden=(4,), max_rounds=2, scaffold=True, **kw)
    with pytest.raises(ValueError, match=f"scaffold.*{word}"):
        TorchRoundEngine(X0, Y0, 2, cfg, SimRank(4, 0, "cpu"), FLAT0, n_total=160, client_sizes=[40] * 4)


def test_other_refusals_one_client_and_the_config_record():
    from fedmi.fl.wide import WideClient
    from fedmi.hpo.fed_sweep import FedTrialGroup
    cfg = EngineConfig(hidden=(4,), max_rounds=2, scaffold=True)
    with pytest.raises(ValueError, match="64 clients"):
        TorchRoundEngine(X0, Y0, 2, cfg, SimRank(65, 0, "cpu"), FLAT0, n_total=2600)
    with pytest.raises(ValueError, match="comm_buffers.*SCAFFOLD"):   # (refused before anything touches a device)
        HipRoundEngine(X0, Y0, 2, cfg, SimRank(4, 0, "cpu"), FLAT0, n_total=160, comm_buffers=(None, None))
    with pytest.raises(ValueError, match="scaffold"):
        FedTrialGroup(X0, Y0, 2, [], None, cfg)
    with pytest.raises(ValueError, match="scaffold"):
        WideClient(torch.as_tensor(X0), torch.as_tensor(Y0), [14, 50, 200, 2], scaffold=True)
    off = EngineConfig().to_dict()
    assert "scaffold" not in off and EngineConfig(scaffold=True).to_dict() == {**off, "scaffold": True}
    e = TorchRoundEngine(X0, Y0, 2, cfg, None, FLAT0)   # one client: off, nothing refused
    assert not e.scaffold and "scaffold_c" not in e.portable_state()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_planner_record_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_scaffold_plan")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_scaffold_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0 and "failures: 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]

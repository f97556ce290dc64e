"""Host build of the selecting peer engine's round plans under AddressSanitizer + UBSan.

``tests/native/test_select_plan.cpp`` feeds the engine's own planner (fedmi/ops/csrc/fl_round_plan.h) the
traits of an engine that aggregates a robust rule or secure aggregation inside the one-shot xGMI peer
kernel (``gather_plane="xgmi"``: a peer, no lagged rounds, no fused evaluation + FedAvg kernel) and
requires the record sequence the executor relies on: one ALLREDUCE per round, no EVAL_FEDAVG, no PACK
after the first round in bf16, SERVER last when on.  Runs on the CPU (no GPU needed)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_select_plans_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_select_plan")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_select_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # 2 dtypes x 3 worlds x 2 step counts x 6 variants x (5 rounds + 3 rounds of phases)
    assert "select plan rounds checked: 576\n" in r.stdout and "select plan failures: 0\n" in r.stdout

"""Host build of the round planner under AddressSanitizer + UBSan.

``tests/native/test_round_plan.cpp`` includes the engine's own planner (fedmi/ops/csrc/fl_round_plan.h:
which kernels a round launches, with which mode, fold mask and buffers, and what it leaves pending),
replays the call scripts of ``tests/golden/round_plans.json`` -- launch sequences and carry bits
recorded from the engine on the GPU before the planner existed -- and requires equality, then checks
that every issued round's metrics are scored once and folded once.  Runs on the CPU (no GPU needed)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_round_plans_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_round_plan")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_round_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    golden = os.path.join(ROOT, "tests", "golden", "round_plans.json")
    r = subprocess.run([exe, golden], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failures: 0" in r.stdout and "sequences checked: 86" in r.stdout
    from fedmi.fl.engine import MAX_LOCAL_STEPS  # the limit users are told is the planner's
    assert f"max local steps: {MAX_LOCAL_STEPS}\n" in r.stdout

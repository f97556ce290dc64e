"""Host build of the round planner's held-out record under AddressSanitizer + UBSan.

``tests/native/test_round_plan_heldout.cpp`` includes the engine's own planner
(fedmi/ops/csrc/fl_round_plan.h) and walks a grid of engine traits: with ``heldout_on`` every round the
engine aggregates ends with exactly one HELDOUT record on the output parity, no configuration is lagged
or folds late, and with the trait off the plans hold no such record and are otherwise the same.  Runs
on the CPU (no GPU needed)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_heldout_round_plans_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "test_round_plan_heldout")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_round_plan_heldout.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failures: 0" in r.stdout
    n = int(r.stdout.split("configurations: ")[1].split()[0])
    assert n >= 500, r.stdout[-500:]

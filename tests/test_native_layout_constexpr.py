"""The reference shape's compile-time layouts equal the run-time ones (fl_layout.h FlRefShape).

``tests/native/test_layout_constexpr.cpp`` builds the engine's descriptors for 14-50-200-2 with the
run-time layout functions and compares them byte by byte with the constants the shape-specialised
kernels are compiled from; four near-miss shapes must not match.  A stand-alone host program under
AddressSanitizer + UBSan, like tests/test_native_layout.py.  Runs on the CPU (no GPU needed)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_reference_shape_constants_match_runtime_layout(tmp_path):
    exe = str(tmp_path / "test_layout_constexpr")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_layout_constexpr.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "failures: 0" in r.stdout and "R=32: level 1, 160912 LDS bytes, head_split 7" in r.stdout

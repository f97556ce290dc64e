"""The Adam kernels' dense-index lookup (fl_adam_map.h) on the host.

``tests/native/test_adam_map.cpp`` evaluates the arm the shape-specialised Adam kernel compiles, with
the ``FlRefShape<32>`` constants, and the generic arm, with the engine's run-time descriptors, for all
11 352 dense indices of the 14-50-200-2 MLP: image index, packed position and bias flag agree with each
other and with the layouts' definition, inside their buffers, no slot twice.  A stand-alone host program
under AddressSanitizer + UBSan, like tests/test_native_layout_constexpr.py.  Runs on the CPU (no GPU
needed)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_static_lookup_equals_runtime_lookup_for_every_dense_index(tmp_path):
    exe = str(tmp_path / "test_adam_map")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_adam_map.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "indices: 11352" in r.stdout and "failures: 0" in r.stdout

"""The index maps of the exchanged epilogues (fl_layout.h fl_epi_*) on the host.

``tests/native/test_epi_map.cpp`` walks every forward tile of both hidden layers and every dgrad item of the
reference 14-50-200-2 MLP at R = 32: each (row, column) of an output buffer is produced by exactly one
(lane, j), a lane's 4 columns are consecutive and are the outputs of the operand rows the exchanged MFMA
gives it, and every 8-byte store, 8-byte mask read and 16-byte bias read is aligned and inside its buffer's
extent from ``FlRefShape<32>::e``.  A stand-alone host program under AddressSanitizer + UBSan, like
tests/test_native_slab_map.py.  Runs on the CPU (no GPU needed)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_exchanged_epilogue_maps_of_the_reference_shape(tmp_path):
    exe = str(tmp_path / "test_epi_map")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_epi_map.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "failures: 0" in r.stdout
    # forward: (4 + 14) column tiles, dgrad: (14 + 4) items, each 2 row tiles x 64 lanes of 4 values:
    # 32 rows x (64 + 224) padded columns, once forward and once backward
    assert "lane stores: 4608" in r.stdout and "elements: 18432" in r.stdout

"""The blocked fp16 gradient-slab row (fl_layout.h FlSlabBlk) on the host.

``tests/native/test_slab_map.cpp`` walks the reference 14-50-200-2 MLP's row: the map from dense index to
row position is injective and hits every non-pad position exactly once, pads are exactly the ``i >= K``
columns of a block, block offsets are 64-byte aligned, every lane's 4-value store of a wgrad tile is
8-byte aligned, inside its block, and the stores of a launch cover the row exactly once; the inverse map
the specialised Adam kernel evaluates agrees for compile-time and run-time descriptors.  A stand-alone
host program under AddressSanitizer + UBSan, like tests/test_native_adam_map.py.  The row length it
prints is what the engine sizes its slab rows from.  Runs on the CPU (no GPU needed)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_blocked_row_map_of_the_reference_shape(tmp_path):
    exe = str(tmp_path / "test_slab_map")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_slab_map.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "indices: 11352" in r.stdout and "failures: 0" in r.stdout
    # 11 352 parameters + the pad columns: 50 x 2 (layer 0), 200 x 2 (layer 1's last block), none in the head
    assert "row halves: 11852" in r.stdout and "pads: 500" in r.stdout
    # the row length equals what the engine allocates per slab row (fp16 halves + the fp32 loss slot, padded)
    from fedmi.ops import native
    floats = int(re.search(r"row floats: (\d+)", r.stdout).group(1))
    assert floats == ((11852 + 1) + 3) // 4 * 4
    assert native().slab_row_floats([14, 50, 200, 2], 32) == floats
    # any other shape or R keeps the dense row
    assert native().slab_row_floats([14, 50, 200, 2], 16) == ((11352 + 1) + 3) // 4 * 4
    assert native().slab_row_floats([17, 24, 3], 32) == ((17 * 24 + 24 + 24 * 3 + 3 + 1) + 3) // 4 * 4

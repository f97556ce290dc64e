"""The dense-index -> image-position rule of the kernels behind the Adam kernel (fl_image.h) on the host.

``tests/native/test_image_index.cpp`` walks every dense index of seven shapes (14-50-200-2, 17-24-3, 1-16-2,
33-65-3, 14-33-17-9-5, 14-7, 40-40-96-4: 21 687 indices): ``fl_image_index`` equals the Adam kernels' run-time
lookup (``fl_adam_pos<false>``), stays inside the image, hits no slot twice, lands only on floats that
``fl_image_lim`` calls real, and ``fl_image_lim`` calls exactly P floats real.  A stand-alone host program under
AddressSanitizer + UBSan, like tests/test_native_adam_map.py.  Runs on the CPU (no GPU needed)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_image_index_equals_the_adam_lookup_and_inverts_image_lim(tmp_path):
    exe = str(tmp_path / "test_image_index")
    cmd = ["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "fedmi", "ops", "csrc"),
           os.path.join(ROOT, "tests", "native", "test_image_index.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "indices: 21687" in r.stdout and "failures: 0" in r.stdout

"""AddressSanitizer + UBSan over the host half of the overlay rasteriser: tools/sanitize/overlay_fuzz.cpp, a stand-alone
program that links csrc/ck_overlay.cpp alone and runs hostile display lists through ck_overlay_plan -- fields at and past
their limits, text ranges out of range, frame_start going backwards, cap of 0 and of one short, random lists planned into
buffers of exactly the size asked for.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_overlay_plan_is_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "overlay_fuzz")
    csrc = os.path.join(ROOT, "camkifu_amd", "csrc")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize", "overlay_fuzz.cpp"),
                          os.path.join(csrc, "ck_overlay.cpp"), "-o", exe], capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "overlay plan:" in run.stdout and "clean" in run.stdout

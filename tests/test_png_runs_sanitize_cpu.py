"""AddressSanitizer + UBSan over the staged PNG encoder in its runs mode: tools/sanitize/png_runs_fuzz.cpp, a stand-alone
program that links csrc/ck_png.cpp (with csrc/ck_png_stage.h) alone, encodes frames at sizes around the seams and rows with
a run of every length around a match's limits, inflates every file with the library's own inflate and compares the pixels.
Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_runs_mode_is_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "png_runs_fuzz")
    csrc = os.path.join(ROOT, "camkifu_amd", "csrc")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize", "png_runs_fuzz.cpp"),
                          os.path.join(csrc, "ck_png.cpp"), "-o", exe], capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "files round trip, clean" in run.stdout

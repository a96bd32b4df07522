"""AddressSanitizer + UBSan over the stages of the GPU's JPEG entropy coder as the host runs them:
tools/sanitize/jpeg_enc_stage_fuzz.cpp, a stand-alone program that links csrc/ck_jpeg_enc.cpp and csrc/ck_jpeg.cpp alone, fed
with committed goldens extracted into tmp_path.  It codes their coefficients, the synthetic extremes of jpeg_enc_stage_cases
and seeded random coefficients (uncodable ones included) in buffers of exactly their size, and holds every status, frame,
message, length and byte to the plain host coder.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from . import jpeg_enc_cases as cases
from .test_jpeg_enc_sanitize_cpu import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staged_jpeg_coder_is_clean_under_asan_ubsan_and_equals_the_plain_coder(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    files = []
    for case in CASES:
        files.append(str(tmp_path / (cases.name_of(case) + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(cases.golden(case))
    exe = str(tmp_path / "jpeg_enc_stage_fuzz")
    csrc = os.path.join(ROOT, "camkifu_amd", "csrc")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize", "jpeg_enc_stage_fuzz.cpp"),
                          os.path.join(csrc, "ck_jpeg_enc.cpp"), os.path.join(csrc, "ck_jpeg.cpp"), "-o", exe],
                         capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "jpeg staged encoder: %d cases" % len(files) in run.stdout and "equal to the plain coder" in run.stdout

"""AddressSanitizer + UBSan over the host half of the JPEG encoder: tools/sanitize/jpeg_enc_fuzz.cpp, a stand-alone program
that links csrc/ck_jpeg_enc.cpp and csrc/ck_jpeg.cpp alone, fed with committed goldens extracted into tmp_path: each is
decoded, encoded again (the file's bytes must come back), then hostile coefficients over its geometry and output buffers
below the bound.  Every stream the encoder writes goes back through the decoder.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from . import jpeg_enc_cases as cases
from . import jpeg_enc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("ramp", 17, 33, ref.S420, 90, 3), ("noise", 17, 33, ref.GREY, 90, 1), ("noise", 48, 64, ref.S422, 50, 7),
         ("fine", 16, 32, ref.S444, 100, 0), ("checker", 32, 32, ref.S420, 100, 0), cases.forward_case(1, 1, ref.S420, 90),
         ("noise", 80, 24, ref.S444, 90, 3), cases.forward_case(8, 8, ref.S422, 1)]


def test_host_jpeg_encoder_is_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    files = []
    for case in CASES:
        files.append(str(tmp_path / (cases.name_of(case) + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(cases.golden(case))
    exe = str(tmp_path / "jpeg_enc_fuzz")
    csrc = os.path.join(ROOT, "camkifu_amd", "csrc")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize", "jpeg_enc_fuzz.cpp"),
                          os.path.join(csrc, "ck_jpeg_enc.cpp"), os.path.join(csrc, "ck_jpeg.cpp"), "-o", exe],
                         capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "jpeg host encoder: %d cases" % len(files) in run.stdout and "encodes clean" in run.stdout

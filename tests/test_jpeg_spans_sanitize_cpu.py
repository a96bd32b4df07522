"""AddressSanitizer + UBSan over the steps of the span decoder the GPU kernels run: tools/sanitize/jpeg_span_fuzz.cpp, a
stand-alone program that links csrc/ck_jpeg.cpp, csrc/ck_jpeg_plan.cpp and csrc/ck_jpeg_span.cpp (csrc/ck_jpeg_span.h) alone, fed
with the committed cases of test_jpeg_sanitize_cpu extracted into tmp_path (whole, truncated at every offset, mutated at
every offset of the scan), at span sizes of 8 and 64 bytes.  The program also holds every decode against the host decoder:
decision, message, coefficients.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from . import jpeg_cases
from .test_jpeg_sanitize_cpu import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_span_decoder_is_clean_under_asan_ubsan_and_equals_the_host_decoder(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    files = []
    for name in CASES + ["bare"]:
        data = jpeg_cases.file_cases()[name][0] if name != "bare" else jpeg_cases.strip_dht(jpeg_cases.file_cases()[CASES[0]][0])
        files.append(str(tmp_path / (name + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(data)
    exe = str(tmp_path / "jpeg_span_fuzz")
    csrc = os.path.join(ROOT, "camkifu_amd", "csrc")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize", "jpeg_span_fuzz.cpp"),
                          os.path.join(csrc, "ck_jpeg.cpp"), os.path.join(csrc, "ck_jpeg_plan.cpp"), os.path.join(csrc, "ck_jpeg_span.cpp"),
                          "-o", exe], capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "jpeg span decoder: %d cases" % len(files) in run.stdout and "equal to the host decoder" in run.stdout

"""AddressSanitizer + UBSan over the host half of the JPEG decoder: tools/sanitize/jpeg_fuzz.cpp, a stand-alone program
that links csrc/ck_jpeg.cpp alone, fed with committed cases extracted into tmp_path (whole, truncated at every offset,
mutated).  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from . import jpeg_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["noise_17x33_420_q90_r3", "noise_17x33_422_q100_r0", "ramp_17x33_444_q5_r3", "noise_8x8_grey_q90_r0",
         "noise_1x1_420_q90_r0", "ramp_48x64_420_q90_r3", "noise_50x35_422_q5_r0", "ramp_47x61_grey_q100_r3"]


def test_host_jpeg_decoder_is_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    files = []
    for name in CASES + ["bare"]:
        data = jpeg_cases.file_cases()[name][0] if name != "bare" else jpeg_cases.strip_dht(jpeg_cases.file_cases()[CASES[0]][0])
        files.append(str(tmp_path / (name + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(data)
    exe = str(tmp_path / "jpeg_fuzz")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize", "jpeg_fuzz.cpp"),
                          os.path.join(ROOT, "camkifu_amd", "csrc", "ck_jpeg.cpp"), "-o", exe], capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "jpeg host decoder: %d cases" % len(files) in run.stdout and "decodes clean" in run.stdout

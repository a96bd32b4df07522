"""AddressSanitizer + UBSan over optimised Huffman tables as the host runs them: tools/sanitize/jpeg_enc_opt_fuzz.cpp, a
stand-alone program that links csrc/ck_jpeg_enc.cpp and csrc/ck_jpeg.cpp alone.  It drives the histo and tables steps, the
two-pass coder and the staged coder over random and adversarial counters and coefficients in buffers of exactly their size,
holds the two coders to one another and to the standard coder's refusals, and decodes every accepted stream back.
Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_optimised_tables_are_clean_under_asan_ubsan_and_both_coders_agree(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "jpeg_enc_opt_fuzz")
    csrc = os.path.join(ROOT, "camkifu_amd", "csrc")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize", "jpeg_enc_opt_fuzz.cpp"),
                          os.path.join(csrc, "ck_jpeg_enc.cpp"), os.path.join(csrc, "ck_jpeg.cpp"), "-o", exe],
                         capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "tables valid" in run.stdout and "equal in both coders" in run.stdout and " 0 batches" not in run.stdout

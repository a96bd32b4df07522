"""The staged inflate, the text the GPU's inflate kernel runs, before a GPU runs it: tools/sanitize/png_inflate_fuzz.cpp, a
stand-alone program that links csrc/ck_png.cpp (with csrc/ck_png_inflate_stage.h) alone and compares ck_png_unzip_staged with
ck_png_unzip -- status, bytes, message -- on the staged encoder's streams at sizes around the ring's seams, on their
truncations and byte changes and on seeded random strings.  Two builds of the one file: under AddressSanitizer + UBSan every
position of the small streams and every 8th of the 18 large ones (all of them would take most of an hour there); plain -O2
every position of every stream, so that no truncation and no byte change is left out.  Nothing is loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / name)
    csrc = os.path.join(ROOT, "camkifu_amd", "csrc")
    res = subprocess.run([cxx, "-std=c++17", "-pthread"] + flags + ["-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "tools", "sanitize", "png_inflate_fuzz.cpp"), os.path.join(csrc, "ck_png.cpp"), "-o", exe],
                         capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def _run(exe, stride, env=None):
    run = subprocess.run([exe, str(stride)], capture_output=True, text=True, env=env, timeout=1200)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    m = re.search(r"png inflate: (\d+) streams \((\d+) refused\) agree, 18 large streams at stride (\d+), clean", run.stdout)
    assert m and int(m.group(3)) == stride, run.stdout[-2000:]
    return int(m.group(1)), int(m.group(2))


def test_staged_inflate_is_clean_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "png_inflate_fuzz", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    streams, refused = _run(exe, 8, dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert streams > 100000 and refused > streams // 2


def test_every_truncation_and_byte_change_of_the_seam_streams(tmp_path):
    """the same program without the sanitizers, stride 1: four damaged streams for every byte of all 24 streams"""
    exe = _build(tmp_path, "png_inflate_sweep", ["-O2"])
    streams, refused = _run(exe, 1)
    assert streams > 900000 and refused > streams // 2

"""AddressSanitizer + UBSan over the host half of the PNG reader and writer: tools/sanitize/png_fuzz.cpp, a stand-alone program
that links csrc/ck_png.cpp (with csrc/ck_png_stage.h) alone, fed with the zlib streams of test_png_cpu and a few PNG files
written into tmp_path -- whole, cut at every length, changed at every offset -- and then run through the staged encoder at
sizes around its seams.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

from . import png_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_host_code_is_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    files = []

    def put(name, data):
        files.append(str(tmp_path / name))
        with open(files[-1], "wb") as f:
            f.write(data)

    for i, (name, z) in enumerate(sorted(png_cases.small_streams().items())):
        put("small%d.z" % i, z)
    for i, (name, (z, _)) in enumerate(sorted(png_cases.inflate_streams().items())):
        put("inflate%d.z" % i, z)
    put("rgb.png", png_cases.image(7, 9, 2, 8, flavour="fixed")[0])
    put("palette.png", png_cases.image(5, 6, 3, 2, flavour="huffman", idat_split=7)[0])
    put("grey16.png", png_cases.image(3, 4, 0, 16, flavour="stored")[0])
    put("pillow.png", png_cases.golden()["rgb alpha 8 bit"][0])
    exe = str(tmp_path / "png_fuzz")
    csrc = os.path.join(ROOT, "camkifu_amd", "csrc")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sanitize", "png_fuzz.cpp"),
                          os.path.join(csrc, "ck_png.cpp"), "-o", exe], capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "png reader: %d cases" % len(files) in run.stdout and "clean" in run.stdout
    assert "files round trip" in run.stdout

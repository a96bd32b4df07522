"""The staging layouts and the pass rules of the codec entry points (csrc/ck_stage_layout.h over csrc/ck_carve.h), on the CPU:
tools/stage_layouts.cpp, a stand-alone program that includes the two headers alone, is built with the host compiler under
AddressSanitizer + UBSan and prints every offset and total for a fixed list of small inputs.  They are held to
tests/golden/stage_layouts.json -- recorded from the formulas as the entry points had them before there was a carver; the
four rows of the span work block were recorded again when the carver put each of its arrays on 16 bytes (docs/lab_notes.md,
note 20) -- and to what the kernels need of any layout: every part on 16 bytes, none overlapping, the total behind the last.
Nothing is loaded into python."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def up16(v):
    return (v + 15) // 16 * 16


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("stage_layouts") / "stage_layouts")
    res = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                          "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "tools", "stage_layouts.cpp"), "-o", exe], capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -lasan" in res.stderr or "cannot find -lubsan" in res.stderr
                                or ("libasan" in res.stderr and "No such file" in res.stderr)):
        pytest.skip("sanitizer runtime not installed")
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return [json.loads(line) for line in run.stdout.splitlines()]


def layouts(rows, name=None):
    return [r for r in rows if "layout" in r and name in (None, r["layout"])]


def rule(rows, name):
    return [r for r in rows if r.get("rule") == name]


def test_every_offset_and_total_is_the_recorded_one(rows):
    with open(os.path.join(ROOT, "tests", "golden", "stage_layouts.json")) as f:
        want = json.load(f)
    assert len(rows) == len(want)
    for got, w in zip(rows, want):
        assert got == w, (w.get("layout") or w.get("rule"), w.get("in"))


def test_the_inputs_are_the_small_ones_a_layout_can_go_wrong_at(rows):
    huff = layouts(rows, "huff")
    assert {len(r["in"]["seg_len"]) for r in huff} == {1, 3}
    assert {n for r in huff for n in r["in"]["seg_len"]} >= {0, 1, 15, 16, 17}
    assert {r["in"]["spans"] for r in huff} == {0, 1}
    # a row count whose bytes are and are not a multiple of 16: table sets of 8520 bytes, span words of 4, records of 40
    assert {r["in"]["n_sets"] * 8520 % 16 == 0 for r in huff} == {True, False}
    assert {(r["in"]["ns"] + 1) * 4 % 16 == 0 for r in huff if r["in"]["spans"]} == {True, False}
    assert {len(r["in"]["zlen"]) * 40 % 16 == 0 for r in layouts(rows, "png_inf")} == {True, False}
    assert {r["in"]["optimise"] for r in layouts(rows, "jenc_work")} == {0, 1} and {r["in"]["m"] for r in layouts(rows, "jenc_work")} == {1, 3}
    assert {r["in"]["runs"] for r in layouts(rows, "png_work")} == {0, 1} and {r["in"]["m"] for r in layouts(rows, "png_work")} == {1, 3}
    assert any(0 in r["in"]["zlen"] for r in layouts(rows, "png_inf")) and any(0 in r["in"]["zlen"] for r in layouts(rows, "png_decode_device"))
    assert any("palette" in r["in"]["what"] for r in layouts(rows, "png_decode_host"))
    assert any("palette" in r["in"]["what"] for r in layouts(rows, "png_decode_device"))
    assert {r["layout"] for r in layouts(rows)} == {"huff", "jspan", "jenc_work", "png_inf", "png_decode_host", "png_decode_device",
                                                  "png_work", "harvest"}


def test_parts_lie_on_16_bytes_in_order_without_overlap_inside_the_total(rows):
    for r in layouts(rows):
        what = (r["layout"], r["in"])
        end = 0
        for name, off, nbytes, elem in r["parts"]:
            assert off % 16 == 0, (what, name)
            assert off >= end, (what, name)                              # behind everything before it: no overlap
            end = off + nbytes
        assert r["total"] >= end, what
        assert r["total"] < end + 16, what                               # and no more than the rounding behind the last part
        for key in ("n_bytes", "upload", "dstride", "pin_words"):
            assert r.get(key, 0) % 16 == 0, (what, key)


def test_the_8_byte_arrays_come_first_where_the_comments_promise_that(rows):
    seen = 0
    for r in layouts(rows):
        if "first8" not in r:
            continue
        names = [p[0] for p in r["parts"]]
        promised = r["parts"][:names.index(r["first8"]) + 1]
        last8 = max(off for _, off, _, elem in promised if elem == 8)
        first4 = min(off for _, off, _, elem in promised if elem == 4)
        assert last8 < first4, (r["layout"], r["in"])
        seen += 1
    assert seen == len(layouts(rows, "jspan")) + len(layouts(rows, "jenc_work")) > 0


def test_uploaded_blocks_end_where_their_counters_say(rows):
    for r in layouts(rows, "huff"):                                      # ck_jpeg_uploaded_bytes: ends with the last word, not on 16
        name, off, nbytes, _ = r["parts"][-1]
        assert r["total"] == off + nbytes and name == ("span0" if r["in"]["spans"] else "quant")
        assert r["n_bytes"] == dict((p[0], p[1]) for p in r["parts"])["slack"] + 16
    for r in layouts(rows, "png_decode_host"):                           # ck_png_uploaded_bytes: the whole block
        assert r["upload"] == r["total"]
    for r in layouts(rows, "png_decode_device"):                         # as far as the records: they and the rows stay on the device
        assert r["upload"] == dict((p[0], p[1]) for p in r["parts"])["rec"]
    for r in layouts(rows, "png_inf"):
        assert r["dstride"] == up16(r["in"]["most"])


def test_pass_fit_is_the_clamp(rows):
    fits = rule(rows, "fit")
    for r in fits:
        fit = r["budget"] // max(r["frame_bytes"], 1)
        assert r["pass"] == min(max(fit, 1), r["n"]), r
    by = {(r["n"], r["frame_bytes"], r["budget"]): r["pass"] for r in fits}
    assert by[(5, 100, 99)] == 1                                         # fit < 1: one frame all the same
    assert by[(5, 100, 500)] == 5 and by[(5, 100, 499)] == 4             # fit == n, and one byte short of it
    assert by[(5, 100, 100000)] == 5                                     # fit > n
    assert by[(1, 7, 0)] == 1 and by[(5, 0, 3)] == 3
    for r in rule(rows, "fit_hbm"):
        first = min(max(r["budget"] // max(r["frame_bytes"], 1), 1), r["n"])
        assert r["pass"] == min(max(r["hbm"] // max(r["cframe"], 1), 1), first), r
    assert [r["pass"] for r in rule(rows, "fit_hbm")] == [3, 5, 1, 4]
    for r in rule(rows, "fit_streams"):
        frame = sum(r["len"]) // len(r["len"]) + 384 + 16
        first = min(max(r["budget"] // frame, 1), len(r["len"]))
        assert r["pass"] == min(max(r["hbm"] // r["cframe"], 1), first), r
    assert [r["pass"] for r in rule(rows, "fit_streams")] == [2, 1, 2]


def test_png_passes_take_every_frame_once_in_order_within_the_budget(rows):
    takes = rule(rows, "take")
    assert any(len(r["inflated"]) == 20 for r in takes)
    for r in takes:
        inflated, zlen, budget = r["inflated"], r["zlen"], r["budget"]
        at = 0
        for f0, m, rows_bytes, z_bytes in r["passes"]:
            assert f0 == at and m >= 1, r                                # no frame skipped or repeated
            assert rows_bytes == sum(up16(v) for v in inflated[f0:f0 + m])
            assert z_bytes == sum(up16(v) for v in zlen[f0:f0 + m])
            assert rows_bytes <= budget or m == 1, r                     # within the budget, or the one frame that is above it
            if f0 + m < len(inflated):                                   # greedy: the next frame would not have fitted
                assert rows_bytes + up16(inflated[f0 + m]) > budget, r
            at += m
        assert at == len(inflated), r
    by = {(tuple(r["inflated"]), r["budget"]): [(p[0], p[1]) for p in r["passes"]] for r in takes}
    assert by[((100, 10, 10), 64)] == [(0, 1), (1, 2)]                   # a first frame above the budget still takes one frame
    assert by[((16, 16, 32, 64), 64)] == [(0, 3), (3, 1)]                # frames that fill the budget exactly
    assert by[((16, 16, 33, 64), 64)] == [(0, 2), (2, 1), (3, 1)]        # one byte over: 33 rounds up to 48
    twenty = [r for r in takes if len(r["inflated"]) == 20]
    assert [len(r["passes"]) for r in twenty if r["budget"] == 1] == [20] and [len(r["passes"]) for r in twenty if r["budget"] == 100000] == [1]
    assert 1 < len([r for r in twenty if r["budget"] == 96][0]["passes"]) < 20

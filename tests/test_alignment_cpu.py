"""The parts of the alignment tests (tests/align_cases.py, tests/test_gpu_alignment.py) that need no GPU: the placement helper
on CPU tensors, the tables against capi.py, the header and the sources, and the expected values of the rows on shapes of their
own."""
import glob
import inspect
import os
import re

import numpy as np
import pytest

from tests import align_cases as ac
from tests import handover_cases as hc
from tests import test_gpu_alignment as ga

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {1: np.uint8, 2: np.uint16, 4: np.float32}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


@pytest.mark.parametrize("size", sorted(ac.OFFSETS))
def test_place_gives_the_residue_and_the_bands(size):
    assert ac.OFFSETS == {1: (0, 1, 2, 3, 4, 8), 2: (0, 2, 4, 8), 4: (0, 4, 8)}
    for dtype in {1: (np.uint8,), 2: (np.int16, np.uint16), 4: (np.int32, np.float32)}[size]:
        a = (np.arange(3 * 5 * 7) * 37 % 251).astype(dtype).reshape(3, 5, 7)
        for offset in ac.OFFSETS[size]:
            t = ac.place(a, offset, device="cpu")
            assert t.data_ptr() % 16 == offset and t.is_contiguous() and tuple(t.shape) == a.shape
            assert t.numpy().tobytes() == a.tobytes()
            front, behind = ac.bands(t)
            assert len(front) >= ac.PAD and len(behind) >= ac.PAD and (front == ac.GUARD).all() and (behind == ac.GUARD).all()
            ac.untouched(t)
            ac.unchanged(t, a)
    with pytest.raises(AssertionError):
        ac.place(np.zeros(4, np.int32), 2, device="cpu")               # no residue of the element type


@pytest.mark.parametrize("where", ["last byte in front", "first byte behind", "last byte of the allocation", "first byte of the allocation"])
def test_untouched_sees_one_changed_band_byte(where):
    t = ac.place(np.arange(40, dtype=np.uint8), 3, device="cpu")
    flat, start, nbytes = t._placed
    at = {"last byte in front": start - 1, "first byte behind": start + nbytes, "last byte of the allocation": flat.numel() - 1,
          "first byte of the allocation": 0}[where]
    flat[at] = 0x5B
    with pytest.raises(AssertionError, match="guard band"):
        ac.untouched(t)
    flat[at] = ac.GUARD
    ac.untouched(t)
    t[7] = 0                                                            # the tensor itself is not a band ...
    ac.untouched(t)
    with pytest.raises(AssertionError, match="changed its input"):      # ... but it is what unchanged looks at
        ac.unchanged(t, np.arange(40, dtype=np.uint8))


def test_the_tables_cover_every_turn_and_every_out():
    from camkifu_amd import capi
    assert sorted(ac.ARGS) == sorted(ac.METHODS) == sorted(ac.ROWS_OF) and set(hc.METHODS) < set(ac.METHODS)
    for m in hc.METHODS:
        assert len(ac.ARGS[m]) == hc.N_ARGS.get(m, 1), m
    # every method of capi.Context that hands a caller's array to Context._in is in the table
    takes_arrays = {name for name, fn in inspect.getmembers(capi.Context, inspect.isfunction) if not name.startswith("_")
                    and re.search(r"self\._(in|rec|goban|weight_ptrs|train_batch)\(", inspect.getsource(fn))}
    assert takes_arrays - {"i420_to_bgr"} <= set(ac.METHODS) and "i420_to_bgr_levels" in ac.METHODS, takes_arrays - set(ac.METHODS)
    for m, k in list(hc.TURNS) + [("png_encode", 0)]:
        assert (m, k) in ga.INPUT_TURNS and ac.offsets_of(m, k) == ac.OFFSETS[np.dtype(ac.ARGS[m][k]).itemsize]
    assert {m for m, k in ga.INPUT_TURNS if k == "all"} == {m for m in hc.METHODS if hc.N_ARGS.get(m, 1) > 1}
    assert set(ac.ROWS_OF["png_encode"]) <= set(__import__("tests.scratch_cases", fromlist=["NAMES"]).NAMES)
    # every method of capi.Context with an `out=` parameter, found by looking
    with_out = sorted(name for name, fn in inspect.getmembers(capi.Context, inspect.isfunction)
                      if not name.startswith("_") and "out" in inspect.signature(fn).parameters)
    assert with_out == sorted(ac.OUT) == sorted(ac.OUT_ROWS)
    assert sorted({m for m, _ in ga.OUT_CASES}) == with_out
    from tests.test_gpu_handover import OUT_METHODS
    assert set(OUT_METHODS) <= {name for names in ac.OUT_ROWS.values() for name in names}
    for m, names in ac.OUT_ROWS.items():
        for name in names:
            assert name in ac.ROWS_OF.get(m, ()) or name in __import__("tests.scratch_cases", fromlist=["NAMES"]).NAMES, name
    for m, k in ac.IN_PLACE:
        assert k < len(ac.ARGS[m])
    assert set(ac.ONE_SPACE) <= set(hc.METHODS) and set(ac.OWN) <= set(hc.METHODS)


def test_allowed_is_the_refusals_offset_by_offset():
    assert ga.ALLOWED is ac.ALLOWED
    want = {}
    for m, a, _, _, align, msg in ac.REFUSALS:
        if a is None:
            continue
        size = np.dtype(ac.OUT[m] if a == "out" else ac.ARGS[m][a]).itemsize
        for off in ac.OFFSETS[size]:
            if off % align:
                want[(m, a, off)] = msg
    assert ac.ALLOWED == want and len(want) == 6 + 3 + 3 + 3 + 6 + 8
    # the record rows: written at 0 and 8, refused at 4
    for m in ("board_detect_records", "cnn_regions_records"):
        assert sorted(off for (mm, a, off) in ac.ALLOWED if mm == m) == [1, 2, 3, 4]
    # a refusal capi cannot reach is one of an output capi allocates itself
    assert {(m, c) for m, a, _, c, _, _ in ac.REFUSALS if a is None} == {
        ("jpeg_coefficients_device", "coef"), ("jpeg_coefficients_device", "quant"), ("harvest_patches", "x"), ("harvest_patches", "src")}


def test_allowed_equals_the_headers_list_and_the_sources_say_so():
    header = _read("include", "camkifu_amd.h")
    section = header[header.index("Alignment of device memory"):]
    section = section[:section.index("*/")]
    listed = re.findall(r'^ \*\s+(ck_\w+)\s+(\w+)\s+(\d+)\s+CK_ERR_ARG "([^"]+)"$', section, re.M)
    assert [(c, arg, int(n), msg) for c, arg, n, msg in listed] == [(c, arg, n, msg) for _, _, c, arg, n, msg in ac.REFUSALS]
    assert "Alignment of device memory" in _read("INTEGRATION.md")
    entry_points = sorted(glob.glob(os.path.join(ROOT, "camkifu_amd", "csrc", "ck_api*.hip")))   # (a later split cannot hide a refusal)
    assert {os.path.basename(p) for p in entry_points} >= {"ck_api.hip", "ck_api_jpeg.hip", "ck_api_png.hip"}
    sources = "".join(_read(p) for p in entry_points) + _read("camkifu_amd", "csrc", "k_records.hip")
    for msg in set(ac.ALLOWED.values()) | {r[5] for r in ac.REFUSALS}:
        assert '"%s"' % msg in sources, msg
    # and every alignment refusal of these sources is in the table
    in_sources = set(re.findall(r'ck_fail\(ctx, CK_ERR_ARG, "([^"]*(?:must lie on|aligned)[^"]*)"', sources))
    assert in_sources == {r[5] for r in ac.REFUSALS}
    # each has its case in the argument contract
    contract = _read("tests", "test_gpu_arg_contract.py")
    for msg in in_sources:
        assert '"%s"' % msg in contract, msg
    for _, _, c_name, _, _, _ in ac.REFUSALS:
        assert "e.L.%s(" % c_name in contract or "L.%s(" % c_name in contract, c_name


def test_the_rows_on_their_own_shapes_reach_their_paths_and_have_expected_values(ora):
    own = ac.own_rows(ora)
    assert {m: tuple(r.name for r in rows) for m, rows in own.items()} == ac.OWN
    for m, rows in own.items():
        for r in rows:
            assert len(r.args) == len(ac.ARGS[m])
            for k, a in enumerate(r.args):
                assert a.dtype == np.dtype(ac.ARGS[m][k]) and a.flags.c_contiguous, (r.name, k)
            r.reaches()
            want = r.expect()
            assert want is r.expect()                                   # computed once
            assert len(want) == len(r.args[0]), r.name                  # one answer per frame
    # the shapes the kernels' conditions give
    assert ac.median_interior_tiles(108, 108, 15) == [(1, 1)] and not ac.median_interior_tiles(104, 108, 15) and not ac.median_interior_tiles(108, 106, 15)
    assert ac.median_interior_tiles(110, 112, 5) == [(1, 1)] and not ac.median_interior_tiles(109, 112, 5) and not ac.median_interior_tiles(110, 111, 5)
    assert not ac.median_interior_tiles(96, 128, 15)                    # the handover input has none
    for f in hc._scenes()[0]:
        assert f.shape == (96, 128, 3)

"""The host decisions of k_board_lines (csrc/ck_host_geom.cpp: ck_hough_slab, ck_board_round_want, ck_board_rank,
ck_peaks_to_lines) through ctypes, no GPU, against tests/board_ref.py.  The component tables are built from the
reference's contours with the table slots shuffled, as the kernels hand them out in no particular order; exact areas
are the reference's float64 ones (exact on the axis-aligned shapes used here)."""
import ctypes as C

import numpy as np
import pytest

from tests import board_ref as R
from tests.test_gpu_board_lines import SLAB_SHAPES, _nest_and_frame_maps, _zero_area_maps


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_contours", C.c_int32), ("n_lines", C.c_int32), ("reserved", C.c_int32),
                ("biggest_area", C.c_double)]


@pytest.fixture(scope="module")
def lib():
    from camkifu_amd import capi
    capi.build()
    L = C.CDLL(capi.SO_PATH)
    L.ck_hough_slab.argtypes = [C.c_int] * 5 + [C.c_void_p] * 3
    L.ck_board_round_want.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
    L.ck_board_rank.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.ck_peaks_to_lines.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ck_peaks_to_lines.restype = None
    return L


# ---------------------------------------------------------------- Hough slab geometry
@pytest.mark.parametrize("n, h, w", SLAB_SHAPES + [(n, 1080, 1920) for n in (1, 32, 33, 128)])
def test_hough_slab(lib, n, h, w):
    row_bytes, rb, threads = C.c_size_t(0), C.c_int(0), C.c_int(0)
    assert lib.ck_hough_slab(n, h, w, 32, 1024, C.byref(row_bytes), C.byref(rb), C.byref(threads)) == 0
    assert (rb.value, threads.value) == R.hough_slab(n, h, w)
    assert row_bytes.value == 4 * (w + h + 2)
    assert (rb.value + 2) * row_bytes.value <= (144 if threads.value == 1024 else 72) * 1024


def test_hough_slab_too_large(lib):
    out = C.c_size_t(7), C.c_int(7), C.c_int(7)
    h = w = 36864 // 3 // 2                               # S = w + h + 2 > 36864 / 3: not even one inner row
    assert 36864 // (w + h + 2) - 2 < 1
    assert lib.ck_hough_slab(1, h, w, 32, 1024, *[C.byref(o) for o in out]) == -1
    assert lib.ck_hough_slab(1, h, w - 2, 32, 1024, *[C.byref(o) for o in out]) == 0 and out[1].value == 1


# ---------------------------------------------------------------- rounds, ranking and gate
def _select(lib, e, seed=0):
    """the exact-area rounds and the ranking over the reference's contours of edge map e -> (sel as discovery keys,
    Result, {key: round it was measured in})"""
    cs = R.external_contours(e)
    nc = len(cs)
    slot_of = np.random.default_rng(seed).permutation(nc)              # contour (discovery order) -> table slot
    root, ub, exact = np.zeros(nc, np.int32), np.zeros(nc), np.zeros(nc)
    for c, s in zip(cs, slot_of):
        root[s] = c["key"]
        ub[s] = float(c["xs"].max() - c["xs"].min()) * float(c["ys"].max() - c["ys"].min())
        exact[s] = R.min_area(c["xs"], c["ys"])
    area, known = np.zeros(nc), (ub == 0.0).astype(np.uint8)
    measured = {}
    for rnd in range(3):
        want = np.zeros(max(nc, 1), np.uint8)
        must, may, count = R.round_wants(rnd, ub, area, known)
        got = lib.ck_board_round_want(rnd, nc, ub.ctypes.data, area.ctypes.data, known.ctypes.data, want.ctypes.data)
        took = set(np.nonzero(want)[0].tolist())
        assert got == count == len(took) and must <= took <= must | may, "round %d" % rnd
        if not got:
            break
        assert rnd < 2, "contour selection did not converge"
        for s in took:
            area[s], known[s] = exact[s], 1
            measured[int(root[s])] = rnd
    sel, res = np.full(4, 99, np.int32), Result(status=R.NO_CONTOUR if nc == 0 else R.LINES)
    go = lib.ck_board_rank(nc, root.ctypes.data, area.ctypes.data, known.ctypes.data, e.shape[0], e.shape[1],
                           sel.ctypes.data, C.byref(res))
    assert go == sel[3] and go == (res.status == R.LINES and nc > 0)
    return [int(root[s]) if s >= 0 else -1 for s in sel[:3]], res, measured


def _check_select(lib, e, thr):
    ref = R.board_lines(e, thr)
    keys_cv = [c["key"] for c in R.external_contours(e)[::-1]]
    for seed in range(3):
        sel, res, measured = _select(lib, e, seed)
        assert res.status == ref["status"]
        if ref["status"] == R.NO_CONTOUR:
            assert sel == [-1, -1, -1]
            continue
        assert res.biggest_area == ref["biggest_area"]
        if ref["status"] == R.TOO_SMALL:
            assert sel == [-1, -1, -1]
            continue
        pos, _, _ = R.select(ref["areas"])
        want = [keys_cv[p] for p in pos[::-1]]                           # biggest first
        assert sel == want + [-1] * (3 - len(want))
    return measured


def test_rank_equal_areas(lib):
    e = R.equal_combs()
    for m in (e, e[:, ::-1], e[::-1]):
        _check_select(lib, m, 40)


def test_rank_gate(lib):
    assert R.board_lines(R.gate_map(False), 8)["status"] == R.TOO_SMALL
    assert R.board_lines(R.gate_map(True), 8)["status"] == R.LINES
    _check_select(lib, R.gate_map(False), 8)
    _check_select(lib, R.gate_map(True), 8)


def test_rank_zero_area_and_nesting(lib):
    for e in _zero_area_maps() + _nest_and_frame_maps() + [np.zeros((20, 30), np.uint8)]:
        _check_select(lib, e, 10)


@pytest.mark.parametrize("k", [17, 18])
def test_rounds_diagonal_decoys(lib, k):
    """the 16 largest bounding boxes are strokes of area 0: the outline is measured in the second round, and nothing is
    left for a third"""
    for e in (R.decoy_map(k), R.decoy_map(k)[:, ::-1]):
        cs = R.external_contours(e)
        winner = max(cs, key=lambda c: R.min_area(c["xs"], c["ys"]))["key"]
        measured = _check_select(lib, e, 20)
        assert measured[winner] == 1 and sorted(set(measured.values())) == [0, 1]
        assert sum(1 for r in measured.values() if r == 0) == 16 and len(measured) == k + 1


# ---------------------------------------------------------------- peaks to lines
@pytest.mark.parametrize("h, w, seed", [(64, 300, 1), (64, 300, 2), (90, 130, 3)])
def test_peaks_to_lines(lib, h, w, seed):
    rng = np.random.default_rng(seed)
    ref = None
    while ref is None or ref["status"] != R.LINES or len(ref["lines"]) < 8:
        ref = R.board_lines(R.slab_map(rng, h, w), 12)
    pk = R.peaks(ref["ghost"], 12)
    assert len(pk) == len(ref["lines"]) and len(np.unique(pk[:, 1])) < len(pk)         # ties in count
    pk = np.ascontiguousarray(pk[rng.permutation(len(pk))])                         # the kernel's order is arbitrary
    numrho = 2 * (w + h) + 1
    for cap in (len(pk) + 5, len(pk), 3, 0):
        lines = np.full((len(pk) + 5, 2), -7.0, np.float32)
        lib.ck_peaks_to_lines(pk.ctypes.data, len(pk), numrho, cap, lines.ctypes.data)
        k = min(cap, len(pk))
        assert np.array_equal(lines[:k], ref["lines"][:k]) and (lines[k:] == -7.0).all()

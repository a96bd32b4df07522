"""The plain K3..K6 references of tests/board_ref.py on hand-worked edge maps, and against the oracle's contours,
minAreaRect, selection and HoughLines on random maps up to 1080p (the oracle's Hough was otherwise checked against a
naive loop on one 60x80 image)."""
import numpy as np
import pytest

from tests import board_ref as R


def _tops(e):
    return [(c["key"], sorted(zip(c["ys"].tolist(), c["xs"].tolist()))) for c in R.external_contours(e)]


# ---------------------------------------------------------------- hand-worked maps
def test_contours_outline_nested_and_frame_split():
    e = np.zeros((20, 30), np.uint8)
    R.outline(e, 2, 3, 15, 25)
    e[8, 8:12] = 255                                          # inside the closed outline: not top-level
    e[5:19, 28] = 255                                         # reaches the frame row 19: cleared there
    e[19, :] = 255
    e[0, 0:10] = 255                                          # on the frame: gone
    t = _tops(e)
    assert [k for k, _ in t] == [2 * 30 + 3, 5 * 30 + 28]
    box = [(y, x) for y in range(2, 16) for x in range(3, 26) if y in (2, 15) or x in (3, 25)]
    assert t[0][1] == sorted(box)
    assert t[1][1] == [(y, 28) for y in range(5, 19)]
    # a U standing on the frame row splits into its two arms when the frame is cleared
    u = np.zeros((12, 12), np.uint8)
    u[3:12, 3] = u[3:12, 8] = 255
    u[11, 3:9] = 255
    assert [k for k, _ in _tops(u)] == [3 * 12 + 3, 3 * 12 + 8]


def test_outer_border_is_4_adjacent_to_s0():
    """a thick L: the pixel in its inner corner meets S0 only diagonally, so it is not outer border; the pixels of a
    closed outline's inside face meet only the hole"""
    e = np.zeros((20, 24), np.uint8)
    e[5:15, 5:7] = 255
    e[13:15, 5:18] = 255
    (key, pix), = _tops(e)
    assert key == 5 * 24 + 5
    assert (13, 6) not in pix and (12, 6) in pix and (13, 7) in pix
    assert len(pix) == e.astype(bool).sum() - 1
    f = np.zeros((12, 12), np.uint8)
    f[2:10, 2:10] = 255
    f[4:8, 4:8] = 0                                           # a 2-px thick frame around a hole
    (_, pix), = _tops(f)
    assert len(pix) == 28 and (3, 3) not in pix and (2, 2) in pix


def test_contours_8_connected_edges_4_connected_background():
    e = np.zeros((10, 10), np.uint8)
    for i in range(6):
        e[2 + i, 2 + i] = 255                                 # one diagonal stroke: one component
    e[2, 6] = e[3, 7] = 255                                   # touches nothing 8-wise... except (3,7)-(2,6)
    t = _tops(e)
    assert len(t) == 2 and t[0][0] == 2 * 10 + 2
    # a diamond of diagonal steps closes its inside for 4-connected background
    d = np.zeros((11, 11), np.uint8)
    for k in range(4):
        d[1 + k, 5 + k] = d[1 + k, 5 - k] = d[9 - k, 5 + k] = d[9 - k, 5 - k] = 255
    d[5, 1] = d[5, 9] = 255
    d[5, 5] = 255                                             # inside the diamond: not top-level
    t = _tops(d)
    assert len(t) == 1 and len(t[0][1]) == 16


def test_min_area_hand_and_brute():
    assert R.min_area([0, 10, 10, 0, 5], [0, 0, 4, 4, 2]) == 40.0
    assert R.min_area([3], [3]) == 0.0 and R.min_area([0, 3], [0, 4]) == 0.0
    assert R.min_area([0, 1, 2, 4], [0, 1, 2, 4]) == 0.0                      # collinear
    assert R.min_area([0, 2, 0, 2, 0], [0, 0, 2, 2, 0]) == 4.0                 # duplicates
    assert abs(R.min_area([0, 4, 0], [0, 0, 4]) - 16.0) < 1e-9                  # right triangle: legs or hypotenuse
    rng = np.random.default_rng(7)
    for _ in range(60):
        p = rng.integers(0, 300, (int(rng.integers(3, 80)), 2))
        assert abs(R.min_area(p[:, 0], p[:, 1]) - R._min_area_brute(p)) <= 1e-9 * max(1.0, R._min_area_brute(p))


def test_select_is_insort():
    pos, big, s = R.select([5.0, 5.0, 1.0, 5.0, 0.0])
    assert pos == [0, 1, 3] and big == 5.0 and s == [0.0, 1.0, 5.0, 5.0, 5.0]
    pos, big, _ = R.select([0.0, 7.0])
    assert pos == [0, 1] and big == 7.0


def test_selection_maps():
    r = R.board_lines(R.equal_combs(), 40)
    assert r["status"] == R.LINES and r["n_contours"] == 4 and r["areas"] == [7744.0] * 4
    # cv2 order is reverse discovery; equal areas keep insort order, so the three raster-first combs win
    keys = [c["key"] for c in R.external_contours(R.equal_combs())]
    assert keys == sorted(keys)
    g = R.external_contours(R.equal_combs())
    assert not r["ghost"][g[3]["ys"], g[3]["xs"]].any() and all(r["ghost"][c["ys"], c["xs"]].all() for c in g[:3])
    h, w = R.GATE_HW
    lo, hi = R.board_lines(R.gate_map(False)), R.board_lines(R.gate_map(True))
    assert lo["biggest_area"] == h * w / 3 and lo["status"] == R.TOO_SMALL and not lo["ghost"].any()
    assert hi["biggest_area"] == h * w / 3 + 1 and hi["status"] == R.LINES
    d = R.board_lines(R.decoy_map(), 20)
    assert d["status"] == R.LINES and d["n_contours"] == 18 and d["biggest_area"] == 85.0 * 95.0
    assert sorted(d["areas"])[-2] == 0.0
    strokes = np.zeros((30, 40), np.uint8)
    strokes[5, 5:30] = 255
    R.draw_line(strokes, 3, 10, 18, 25)                         # 45 degrees: collinear pixels
    strokes[20, 5] = 255
    z = R.board_lines(strokes)
    assert z["status"] == R.TOO_SMALL and z["n_contours"] == 3 and z["biggest_area"] == 0.0
    assert R.board_lines(np.zeros((9, 9), np.uint8))["status"] == R.NO_CONTOUR


def test_hough_vectorised_equals_naive():
    rng = np.random.default_rng(11)
    for h, w in [(60, 80), (33, 47), (64, 300)]:
        img = (rng.random((h, w)) < 0.03).astype(np.uint8) * 255
        R.draw_line(img, 1, 1, w - 2, h - 2)
        img[:, w // 3] = 255
        for thr in (3, 10):
            l1, a1 = R.hough_lines(img, thr, want_accum=True)
            l2, a2 = R._hough_naive(img, thr)
            assert np.array_equal(a1, a2) and np.array_equal(l1, l2)


def test_hough_slab_formula():
    """(rb, threads) as k_board_lines computes them (`ck_hough_slab`, csrc/ck_host_geom.cpp; tests/test_board_select_cpu.py holds that function to this one)"""
    assert R.hough_slab(1, 720, 1280) == (7, 512) and R.hough_slab(32, 720, 1280) == (7, 512)
    assert R.hough_slab(33, 720, 1280) == (10, 1024) and R.hough_slab(1, 768, 1024) == (8, 512)
    assert R.hough_slab(33, 1440, 2560) == (7, 1024) and R.hough_slab(1, 1080, 1920) == (4, 512)
    assert R.hough_slab(1, 64, 6078) == (1, 512) and R.hough_slab(1, 64, 6200) == (3, 1024)


# ---------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("h, w, density", [(60, 90, 0.05), (60, 90, 0.4), (121, 203, 0.1), (480, 640, 0.003),
                                           (720, 1280, 0.003), (1080, 1920, 0.002)])
def test_reference_vs_oracle_random_maps(ora, h, w, density):
    rng = np.random.default_rng(h * 7 + w)
    e = (rng.random((h, w)) < density).astype(np.uint8) * 255
    for _ in range(6):
        R.draw_line(e, *rng.uniform(0, w, 1), *rng.uniform(0, h, 1), *rng.uniform(0, w, 1), *rng.uniform(0, h, 1))
    R.outline(e, h // 8, w // 8, h - h // 8, w - w // 8)
    cs = R.external_contours(e)
    n, lab, starts = ora.find_external_sets(e)
    assert n == len(cs) and [c["key"] for c in cs] == [int(y) * w + int(x) for x, y in starts]
    lab2 = np.full((h, w), -1, np.int32)
    for k, c in enumerate(cs):
        lab2[c["ys"], c["xs"]] = k
    assert np.array_equal(lab, lab2)
    thr = max(8, min(h, w) // 5)
    ref = R.board_lines(e, thr)
    o = ora.board_lines(e, thr, cap=1 << 20)
    assert ref["n_contours"] == o["n_contours"]
    assert abs(ref["biggest_area"] - o["biggest_area"]) <= 1e-5 * ref["biggest_area"]
    assert not ref["close"] and ref["status"] == R.LINES and o["status"] == len(ref["lines"])
    assert np.array_equal(ref["ghost"], o["ghost"]) and np.array_equal(ref["lines"], o["lines"])
    # the Hough alone, on the edge map itself (more points than any ghost of these maps)
    l1, a1 = R.hough_lines(e, thr, want_accum=True)
    l2, a2 = ora.hough_lines(e, thr, cap=1 << 20, want_accum=True)
    assert np.array_equal(a1, a2) and np.array_equal(l1, l2)


def test_reference_vs_oracle_selection_maps(ora):
    for e, thr in [(R.equal_combs(), 40), (R.gate_map(False), 8), (R.gate_map(True), 8), (R.decoy_map(), 20)]:
        ref, o = R.board_lines(e, thr), ora.board_lines(e, thr, cap=1 << 16)
        assert ref["biggest_area"] == o["biggest_area"] and ref["n_contours"] == o["n_contours"]
        assert np.array_equal(ref["ghost"], o["ghost"]) and np.array_equal(ref["lines"], o["lines"])


def test_random_maps_rarely_close(ora):
    """noise, an outline and four random lines: 3rd and 4th float64 areas within 1e-5 of each other are rare (at 10 %
    noise they are not: L-shaped triples of area 1 abound, and exact ties count as close)"""
    rng = np.random.default_rng(5)
    close = 0
    for k in range(40):
        e = (rng.random((60, 90)) < 0.03).astype(np.uint8) * 255
        R.outline(e, 5, 8, 54, 80)
        for _ in range(4):
            R.draw_line(e, *rng.uniform(0, 90, 1), *rng.uniform(0, 60, 1), *rng.uniform(0, 90, 1), *rng.uniform(0, 60, 1))
        r = R.board_lines(e, 20)
        o = ora.board_lines(e, 20)
        close += r["close"]
        if not r["close"]:
            assert np.array_equal(r["ghost"], o["ghost"]) and np.array_equal(r["lines"], o["lines"])
    assert close <= 4

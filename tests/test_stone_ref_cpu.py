"""tests/stone_ref.py checked without a GPU: its new pieces on hand-worked inputs whose answers are written out here, then
against oracle/ora_grid.py, oracle/ora_stones.py and the oracle's border follower on EVERY case of tests/stone_cases.py and
on the scenes tests/test_gpu_gridlines.py and tests/test_gpu_stonefind.py use (Canny map, lines of every zone in order,
grid; start, vertex count and pixel set of every contour; stones, zones and hull mask), and the host half of the library
(ck_update_grid) against stone_ref.update_grid on the lines of the Hough cases.  Every case must take the paths it is named
for (stone_cases.GRID_PATHS and STONE_PATHS, from the path records; the follower choice from the shape), and no decision of
the contour filters that float32 and float64 could take differently lies within 1e-3 of its threshold.

Capacity: over all grid cases the largest number of lines one zone gives is 13 (negative_counters_hatch, a 40 x 40 zone
of parallel bars) against CK_ZONE_LINES = 32, and the counters stay within -37 .. +37 against the signed 8-bit cells of
hough_zones_kernel; both are asserted below (`< 32`, and the exact range), so the CK_ERR_CAPACITY branch needs no GPU
case: no input found so far reaches it."""
import numpy as np
import pytest

from . import stone_cases as K, stone_ref as R


@pytest.fixture(scope="module")
def grid_cases():
    return K.grid_cases()


@pytest.fixture(scope="module")
def grid_refs(grid_cases):
    return {name: R.find_intersections(c["img"], c["mtx"], c["rects"]) for name, c in grid_cases.items()}


@pytest.fixture(scope="module")
def contour_cases():
    return K.contour_cases()


GRID_NAMES = sorted(K.GRID_PATHS)


# ------------------------------------------------------------------------------------------------ hand-worked
def test_rng_is_multiply_with_carry():
    """(2^32 - 1) K + (2^32 - 1) = K 2^32 + (2^32 - K - 1) with K = 4164903690 = 0xF83F630A"""
    r = R.Rng()
    assert r.below(1 << 32) == 0x07C09CF5 and r.state == 0xF83F630A07C09CF5
    r = R.Rng()
    assert [r.below(n) for n in (4, 3, 2, 1)] == [0x07C09CF5 % 4, 3133359004 % 3, 2578348940 % 2, 0] == [1, 1, 0, 0]


def test_trig_table_is_float32_of_the_double_cosine():
    assert R.COS[0] == 1 and R.SIN[0] == 0
    assert float(R.COS[45]) == float(np.float32(0.70710678)) and R.COS[45] == R.SIN[45] == R.SIN[135] == -R.COS[135]
    assert 0 < float(R.COS[90]) < 1e-7 and R.SIN[90] == 1          # 90 * (float)(pi / 180) falls just short of pi / 2


def test_hough_upright_stroke_by_hand():
    """column 1 of a 4 x 4 zone, threshold 3, minLineLength 2.  The draws are 1, 1, 0, 0: (1, 1), then (1, 3) (moved into
    slot 1), then (1, 0): the third vote makes 3 at angle 0 -- and at every angle that rounds the stroke into one column,
    1 .. 9 and 171 .. 179, angle 0 first.  Downwards from (1, 0) the walk runs to the border, upwards it stops at once:
    the line is (1, 3) - (1, 0); (1, 2) never voted and loses a vote all the same (-1); the last draw is dead."""
    z = np.zeros((4, 4), np.uint8)
    z[:, 1] = 255
    lines, rec = R.hough_lines_p(z, 3, 2)
    assert lines == [(1, 3, 1, 0)]
    assert (rec["drawn"], rec["dead"], rec["weak"], rec["kept"], rec["short"]) == (3, 1, 2, 1, 0)
    assert (rec["cmin"], rec["cmax"]) == (-1, 3)
    ln = rec["lines"][0]
    assert ln["angle"] == 0 and ln["tied"] == list(range(1, 10)) + list(range(171, 180))
    assert (ln["xflag"], ln["unit"], ln["frac"], ln["ends"], ln["steps"]) == (False, 1, 0, ("border", "border"), (3, 0))


def test_hough_level_stroke_short_and_kept():
    """row 2 of a 6 x 6 zone (threshold 4, minLineLength 4): columns 0 .. 3 give a line of extent 3, found and too short:
    its pixels go, no vote is taken back; columns 0 .. 4 give extent 4: kept, walked x-major with the first step to -x"""
    z = np.zeros((6, 6), np.uint8)
    z[2, 0:4] = 255
    lines, rec = R.hough_lines_p(z, 4, 4)
    assert lines == [] and rec["short"] == 1 and rec["cmin"] == 0 and rec["shorts"][0]["extent"] == 3
    assert rec["shorts"][0]["ends"].count("gap") == 1
    z[2, 4] = 255
    lines, rec = R.hough_lines_p(z, 4, 4)
    assert len(lines) == 1 and sorted([lines[0][:2], lines[0][2:]]) == [(0, 2), (4, 2)]
    assert rec["lines"][0]["xflag"] and rec["lines"][0]["unit"] == -1 and lines[0][:2] == (0, 2)
    # the first angle that rounds all five points into one column: 2 sin + 4 cos < 2.5 from 83 degrees on (2.473; at 82
    # degrees 2.537)
    assert rec["lines"][0]["angle"] == 83 and rec["lines"][0]["tied"] == list(range(84, 97))


def test_walk_choice_at_45_and_135_degrees_is_immaterial(grid_cases, grid_refs):
    """|a| = |b| exactly at 45 and 135 degrees (the float32 sine and cosine are equal there): the y-major walk steps by
    (-65536, +-1), the x-major one by (-1, +-65536) from a half-pixel offset on the other axis -- the same pixels in the
    same order.  So `>=` for `>` in the xflag test is an equivalent mutant: no input can tell the two apart."""
    assert R.COS[45] == R.SIN[45] and -R.COS[135] == R.SIN[135]
    assert not any(abs(R.COS[n]) == abs(R.SIN[n]) for n in range(180) if n not in (45, 135))
    c, ref = grid_cases["angles_axes"], grid_refs["angles_axes"]
    edges, seen = ref["edges"], 0
    for (r, col), rec in ref["records"].items():
        if not any(ln["angle"] in (45, 135) for ln in rec["lines"] + rec["shorts"]):
            continue
        x0, y0, x1, y1 = (int(v) for v in c["rects"][r][col])
        lines, rec2 = R.hough_lines_p(edges[x0:x1, y0:y1], rec["threshold"], rec["min_len"], xflag_on_equal=True)
        assert lines == ref["found"].get((r, col), []) and rec2["cmin"] == rec["cmin"] and rec2["dead"] == rec["dead"]
        assert any(ln["xflag"] for ln in rec2["lines"] + rec2["shorts"] if ln["angle"] in (45, 135))
        seen += 1
    assert seen >= 10


def test_update_grid_by_hand():
    """zone (100, 100) .. (120, 120), margin 20 / 7.  Lines in zone coordinates (x = column, y = row)."""
    box, slot = (100, 100, 120, 120), (110, 110)
    level, upright = (0, 8, 16, 8), (4, 0, 4, 16)
    assert R.update_grid([], box, slot) == (110, 110)
    assert R.update_grid([(0, 0, 10, 10)], box, slot) == (110, 110)              # 45 degrees: not a grid line
    # a level line is probed at (mid of the zone, mean of its x + y0): (110, 108), inside
    assert R.update_grid([level], box, slot) == (-110, -110)
    # the same probe for a short stroke at the left: (110, 102), under 100 + 2.857: ignored
    assert R.update_grid([(0, 8, 4, 8)], box, slot) == (110, 110)
    # a level line anywhere down the zone passes: its row is never looked at
    assert R.update_grid([(0, 19, 16, 19)], box, slot) == (-110, -110)
    # the cross meets at column 4, row 8 -> (row + x0, column + y0) = (108, 104), both orders
    assert R.update_grid([level, upright], box, slot) == (-108, -104)
    # two crossings outside the shrunk zone do not count: upright at column 1 -> (108, 101), outside
    assert R.update_grid([level, (1, 0, 1, 16)], box, slot) == (-110, -110)
    # parallels never cross; five good lines only negate
    assert R.update_grid([level, (0, 9, 16, 9)], box, slot) == (-110, -110)
    assert R.update_grid([level, upright] + [(0, 9 + k, 16, 9 + k) for k in range(3)], box, slot) == (-110, -110)
    # the mean of crossings truncates toward zero: (108, 104) twice and (108, 105) twice -> 104.5 -> -104
    assert R.update_grid([level, upright, (5, 0, 5, 16)], box, slot) == (-108, -104)


def test_follower_by_hand():
    e = np.zeros((9, 12), np.uint8)
    e[2, 2] = 255                                    # an isolated pixel: one vertex
    e[2, 5] = e[3, 6] = 255                          # two pixels on a diagonal: there and back, two vertices
    e[5, 1:5] = 255                                  # a level stroke of four: two vertices, its ends
    e[5:8, 7:10] = 255                               # a 3 x 3 blob: four corners, the middle is not border
    got = R.follow_contours(e)
    assert [(c["start"], c["nvert"], len(c["pix"])) for c in got] == [((7, 5), 4, 8), ((1, 5), 2, 4), ((5, 2), 2, 2), ((2, 2), 1, 1)]
    assert (8, 6) not in got[0]["pix"]
    # a figure eight of two rings sharing a corner pixel: the follower cuts both corners at the shared pixel diagonally
    # ((4, 5) -> (5, 6) and (6, 5) -> (5, 4)) and never stands on it -- no background touches it.  Vertices: (1, 1) S,
    # (1, 5) E, (4, 5) SE, (5, 6) S, (5, 9) E, (9, 9) N, (9, 5) W, (6, 5) NW, (5, 4) N, (5, 1) W
    f = np.zeros((12, 12), np.uint8)
    K.ring(f, 1, 1, 5, 5)
    K.ring(f, 5, 5, 9, 9)
    (c,) = R.follow_contours(f)
    assert c["start"] == (1, 1) and c["nvert"] == 10 and len(c["pix"]) == 30 and (5, 5) not in c["pix"]
    # a caret: the start pixel (5, 1) is the tip, passed again between the two arms.  The first neighbour clockwise from
    # west is the SE arm, so the follower takes the SW arm first, comes back through the tip -- the start, but not from
    # the first neighbour: no stop --, takes the SE arm and stops on its way back: vertices (5, 1), (3, 3), (5, 1), (7, 3)
    v = np.zeros((6, 11), np.uint8)
    v[1, 5] = v[2, 4] = v[3, 3] = v[2, 6] = v[3, 7] = 255
    (c,) = R.follow_contours(v)
    assert c["start"] == (5, 1) and c["nvert"] == 4 and len(c["pix"]) == 5


def test_follower_search_may_skip_the_neighbour_after_the_one_it_came_from(contour_cases):
    """after a step the counter-clockwise search starts one past the pixel it came from; starting two past it is an
    equivalent mutant: that neighbour touches the pixel before, whose own search has just passed it over or come from
    it.  Held here on random maps and on the small cases, so the GPU file need not tell the two apart."""
    rng = np.random.default_rng(0)
    maps = [((rng.random((7, 7)) < 0.45) * 255).astype(np.uint8) for _ in range(400)]
    maps += [e for name, batch in contour_cases.items() if batch.shape[1] < 100 for e in batch]
    key = lambda cs: [(c["start"], c["nvert"], c["pix"]) for c in cs]
    assert all(key(R.follow_contours(e)) == key(R.follow_contours(e, resume=5)) for e in maps)


def test_follower_choice_from_the_shape():
    assert R.follower_in_lds(511, 1024) and not R.follower_in_lds(512, 1024)
    assert 511 * 32 * 4 + 4 == 65412                 # the largest request: 64 KB less 124 bytes
    assert R.follower_in_lds(379, 379)


# ------------------------------------------------------------------------------------------------ grid lines
@pytest.mark.parametrize("name", GRID_NAMES)
def test_grid_case_takes_its_paths(grid_cases, grid_refs, name):
    took, max_lines, cmin, cmax = R.grid_paths(grid_refs[name], grid_cases[name]["rects"])
    print(name, "lines per zone <=", max_lines, "counters", cmin, "..", cmax)
    missing = [p for p in K.GRID_PATHS[name] if p not in took]
    assert not missing, (name, missing)
    assert max_lines < R.ZONE_LINES


def test_grid_cases_capacity_and_counter_range(grid_cases, grid_refs):
    stats = [R.grid_paths(grid_refs[n], grid_cases[n]["rects"])[1:] for n in GRID_NAMES]
    assert max(s[0] for s in stats) == 13 < R.ZONE_LINES
    assert (min(s[1] for s in stats), max(s[2] for s in stats)) == (-37, 37)


def test_grid_case_names_are_all_listed(grid_cases):
    assert sorted(grid_cases) == GRID_NAMES


def test_zone_tables(grid_cases, ora):
    assert np.array_equal(K.posgrid(), ora.posgrid(380))
    assert np.array_equal(K.zones_of(K.posgrid()), np.array([[ora.sf_getrect(r, c) for c in range(19)] for r in range(19)]))
    sizes = {(int(q[2] - q[0]), int(q[3] - q[1])) for q in K.mixed_table(0).reshape(-1, 4)}
    assert sizes == set(K.SIZES) and {(4, 4), (4, 40), (40, 4), (40, 40), (19, 20), (7, 33), (8, 8), (5, 13)} <= sizes
    for c in grid_cases.values():
        q = np.asarray(c["rects"]).reshape(-1, 4)
        side = c["img"].shape[0]
        assert (q[:, :2] >= 0).all() and (q[:, 2:] <= side).all() and ((q[:, 2:] - q[:, :2]) >= 4).all()
        assert ((q[:, 2:] - q[:, :2]) <= 40).all()
    bad = K.refused_table()[9, 9]
    assert (bad[2] - bad[0], bad[3] - bad[1]) == (41, 20)
    assert grid_cases["side_127"]["img"].shape[0] % 4 == 3
    assert (grid_cases["goban_learnt"]["mtx"] != grid_cases["goban_default"]["mtx"]).any()


def _same_as_oracle(img, mtx, rects, ref=None):
    from oracle import ora_grid as G
    ref = ref or R.find_intersections(img, mtx, rects)
    g, f, e = G.find_intersections(img, mtx, rects, want_lines=True)
    assert np.array_equal(ref["edges"], e)
    assert ref["found"] == f
    assert np.array_equal(ref["grid"], g)
    return ref


@pytest.mark.parametrize("name", GRID_NAMES)
def test_grid_reference_equals_oracle_on_case(grid_cases, grid_refs, ora, name):
    c = grid_cases[name]
    _same_as_oracle(c["img"], c["mtx"], c["rects"], grid_refs[name])


def test_grid_reference_equals_oracle_on_scenes(ora):
    """the inputs of tests/test_gpu_gridlines.py and of test_find_intersections_on_hostile_images"""
    from camkifu_amd import synth
    dst = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)
    mtx, rects = K.posgrid(), K.zones_of(K.posgrid())
    lines = 0
    for seed, density in ((1, 0.0), (2, 0.2), (3, 0.5)):
        rng = np.random.default_rng(seed)
        corners = synth.random_corners(480, 640, rng)
        frame = synth.render(480, 640, synth.random_stones(rng, density=density), corners, seed=seed).numpy()
        gob = ora.warp_perspective(frame, ora.get_perspective_transform(corners, dst))
        lines += len(_same_as_oracle(gob, mtx, rects)["found"])
    assert lines > 300
    rng = np.random.default_rng(12)
    noise = rng.integers(0, 256, (380, 380, 3), dtype=np.uint8)
    mosaic = np.kron(rng.integers(0, 256, (38, 38, 3), dtype=np.uint8), np.ones((10, 10, 1), np.uint8))
    stripes = np.zeros((380, 380, 3), np.uint8)
    stripes[:, ::7] = 255
    stripes[::5, :] = 128
    for img in (noise, mosaic, stripes):
        _same_as_oracle(img, mtx, rects)


def test_ck_update_grid_equals_reference_on_the_hough_lines(grid_cases, grid_refs):
    """the host half of ck_find_intersections on its own (no GPU): every zone of every case that gave a line"""
    from camkifu_amd import capi
    zones = moved = 0
    for name in GRID_NAMES:
        c, ref = grid_cases[name], grid_refs[name]
        for (r, col), lines in ref["found"].items():
            slot = np.array(c["mtx"][r, col], np.int16)
            capi.update_grid(np.array(lines, np.int32), c["rects"][r][col], slot)
            want = R.update_grid(lines, c["rects"][r][col], c["mtx"][r, col])
            assert tuple(int(v) for v in slot) == want == tuple(int(v) for v in ref["grid"][r, col]), (name, r, col)
            zones += 1
            moved += tuple(abs(v) for v in want) != tuple(int(v) for v in c["mtx"][r, col])
    assert zones > 2000 and moved > 100


# ------------------------------------------------------------------------------------------------ contours
def test_contour_case_shapes(contour_cases):
    """the cases are what their names say: widths on every residue the bit words care about, pixels on the word seams,
    rings on the first and last row and column that can hold an edge, both sides of the follower switch"""
    assert {contour_cases["seams_w%d" % w].shape[2] % 32 for w in (64, 65, 66, 63)} == {0, 1, 2, 31}
    assert {w % 4 == 0 for w in (64, 65, 66, 63, 96, 100)} == {True, False}
    for w in (64, 65, 66, 63, 96, 100):
        e = contour_cases["seams_w%d" % w][0]
        h = e.shape[0]
        assert e[1, 1:w - 1].all() and e[h - 2, 1:w - 1].all() and e[1:h - 1, 1].all() and e[1:h - 1, w - 2].all()
        xs = np.nonzero(e[2:h - 2, 2:w - 2])[1] + 2
        assert {int(v) for v in (xs - 1) & 31} >= {29, 30, 31, 0}
    assert R.follower_in_lds(*contour_cases["follower_lds_511x1024"].shape[1:])
    assert not R.follower_in_lds(*contour_cases["follower_global_512x1024"].shape[1:])
    assert not contour_cases["all_maps_empty"].any() and not contour_cases["one_map_empty"][1].any()
    sp = R.follow_contours(contour_cases["spiral_dominates"][0])
    assert len(sp) == 1 and len(sp[0]["pix"]) > 0.2 * 61 * 83
    big = R.follow_contours(contour_cases["follower_lds_511x1024"][0])
    assert max(len(c["pix"]) for c in big) > 15000 and min(c["nvert"] for c in big) == 1


@pytest.mark.parametrize("name", sorted(K.contour_cases()))
def test_contour_reference_equals_oracle_and_the_set_definition(contour_cases, ora, name):
    for e in contour_cases[name]:
        got = R.follow_contours(e)
        want = list(reversed(ora.find_external_suzuki(e)))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g["start"] == tuple(int(v) for v in w["start"])
            assert g["nvert"] == len(w["vert"])
            assert g["pix"] == set(map(tuple, w["pix"].tolist())) == g["set_def"]


def test_contour_reference_equals_oracle_on_scenes(ora):
    """the random maps of tests/test_gpu_stonefind.py, the small ones"""
    for shape, density, seed in (((40, 56), 0.15, 1), ((97, 131), 0.3, 2), ((120, 64), 0.55, 3)):
        rng = np.random.default_rng(seed)
        edges = ((rng.random((3,) + shape) < density) * 255).astype(np.uint8)
        for e in edges:
            got = R.follow_contours(e)
            want = list(reversed(ora.find_external_suzuki(e)))
            assert [(g["start"], g["nvert"], g["pix"]) for g in got] == \
                   [(tuple(int(v) for v in w["start"]), len(w["vert"]), set(map(tuple, w["pix"].tolist()))) for w in want]


# ------------------------------------------------------------------------------------------------ contour stones
@pytest.fixture(scope="module")
def stone_cases():
    return K.stone_cases()


@pytest.fixture(scope="module")
def stone_refs(stone_cases):
    rects = K.zones_of(K.posgrid())
    return {name: R.find_stones(c["img"], c["fg"], rects, *c["region"]) for name, c in stone_cases.items()}


STONE_NAMES = sorted(K.STONE_PATHS)


def test_opening_by_hand():
    """one column, top to bottom: set runs of 2 (rows 0 - 1), 3 (3 - 5), 4 (7 - 10) and 6 (13 - 18).  Both passes look at rows
    y - 3 .. y, so a run of at least four comes back three rows LOWER (7 - 10 -> 10 - 13, 13 - 18 -> 16 - 21, cut at the
    last row) and the run of three goes.  Rows above the view are ignored by both passes: the erosion keeps the run that
    starts in row 0 although it is only two long, and the dilation stretches it to rows 0 - 4."""
    col = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 0], np.uint8)[:, None] * 255
    want = np.array([1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1], np.uint8)[:, None] * 255
    assert np.array_equal(R.open_rows(col), want)
    below = col[2:]                                       # the same column seen from row 2 on: nothing set touches the top now
    assert (R.open_rows(below)[:, 0] // 255).tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1]
    assert not np.array_equal(R.open_rows(col, back=4), want)


def test_hull_rectangle_and_line_by_hand():
    pts = [(0, 0), (4, 0), (4, 3), (0, 3), (2, 1), (2, 0), (4, 2), (1, 3)]
    assert set(R.hull(pts)) == {(0, 0), (4, 0), (4, 3), (0, 3)} and len(R.hull(pts)) == 4
    assert R.min_rect(R.hull(pts))[:2] == (3.0, 4.0)
    lo, hi, angle = R.min_rect(R.hull([(0, 0), (10, 10), (5, 15), (-5, 5)]))
    assert abs(lo - 50 ** 0.5) < 1e-12 and abs(hi - 200 ** 0.5) < 1e-12 and abs(angle % 90 - 45) < 1e-12
    assert R.line_walk((0, 0), (5, 2)) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]
    assert R.line_walk((5, 2), (0, 0)) == R.line_walk((0, 0), (5, 2))
    assert R.line_walk((1, 4), (2, 0)) == [(1, 4), (1, 3), (1, 2), (2, 1), (2, 0)]


def test_filled_hull_by_hand():
    """the triangle (0, 0), (6, 0), (3, 4).  Outline: the top side; (0, 0) - (3, 4) walks (0, 0), (1, 1), (1, 2), (2, 3), (3, 4)
    -- the error term 4 - 6 = -2 is negative at once (the column moves), then 0, -6, -4; (3, 4) - (6, 0) starts from its
    left end (3, 4): (4, 3), (4, 2), (5, 1), (6, 0).  Fill, rows 0 .. 3, edges at 0.75 y and 6 - 0.75 y in 16.16: row 1
    ceil(0.75) = 1 .. floor(5.25) = 5, row 2 ceil(1.5) = 2 .. 4 (and the outline's (1, 2)), row 3 ceil(2.25) = 3 ..
    floor(3.75) = 3 (and (2, 3), (4, 3)).  The last row is the outline's."""
    img = np.zeros((5, 7), np.uint8)
    R.fill_hull(img, [(0, 0), (6, 0), (3, 4)])
    assert img.tolist() == [[1, 1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 0], [0, 1, 1, 1, 1, 0, 0], [0, 0, 1, 1, 1, 0, 0], [0, 0, 0, 1, 0, 0, 0]]
    one = np.zeros((3, 3), np.uint8)
    R.fill_hull(one, [(1, 1)])
    assert one.sum() == 1 and one[1, 1] == 1


def test_chamfer_by_hand():
    """one source in the corner of a 4 x 6 box: a knight's move costs 143976, two of them 287952 -- less than a diagonal
    and two straight steps (222822 is for (1, 3); (2, 4) is 2 x 143976)"""
    img = np.full((4, 6), 255, np.uint8)
    img[0, 0] = 0
    d = R.chamfer(img)
    assert d[0, 0] == 0 and d[0, 3] == 3 * 65536 and d[2, 2] == 2 * 91750 and d[1, 2] == 143976 and d[2, 4] == 2 * 143976
    assert d[1, 3] == 143976 + 65536 and d[3, 5] == 143976 + 2 * 91750 - 0 * 65536 or d[3, 5] == min(3 * 91750 + 2 * 65536, 2 * 143976 + 91750)


def test_find_centers_by_hand():
    """a 40 x 40 box at radius 10: 2 x 2 cells of 20, reach 20 / 3.  A peak at (9, 10) is 1 from the first cell's centre:
    found.  Peaks in the four corners are 14.1 from theirs: none.  A box of ten rows has no row of cells: division by zero."""
    d = np.zeros((40, 40), np.int64)
    d[10, 9] = 5
    centres, margin = R.find_centers(d, 10.0)
    assert centres[0] == (9, 10) and len(centres) == 1            # the other cells' first maximum is their corner (0, 0)
    e = np.zeros((40, 40), np.int64)
    e[0, 0] = e[0, 39] = e[39, 0] = e[39, 39] = 5
    assert R.find_centers(e, 10.0)[0] == []
    with pytest.raises(ZeroDivisionError):
        R.find_centers(np.zeros((10, 40), np.int64), 10.0)
    assert R.find_centers(np.zeros((11, 40), np.int64), 10.0)[0] == []


def test_no_candidate_can_divide_by_zero():
    """the bound of tests/stone_cases.py's docstring, checked numerically: a rectangle lo <= hi with lo >= 1.5 r cannot
    enclose, with area <= (r - 1) W, a shape that spans W along a strip of r - 1 pixels"""
    for r in (4.0, 10.0, 25.0):
        for lo in np.linspace(1.5 * r, 40 * r, 400):
            hi_max = (1.0 / (1.0 / (r - 1) ** 2 - 1.0 / lo ** 2)) ** 0.5
            assert hi_max < 1.35 * r < lo


def test_find_color_by_hand():
    z = np.zeros((3, 3, 4), np.int16)
    z[:, :, 1:] = 100
    z[1, 1] = (1, 20, 20, 20)
    for level, want, branch in ((20, R.B, "bare_darker"), (240, R.W, "bare_brighter"), (110, R.E, "bare_alike")):
        z[1, 1, 1:] = level
        st, took = np.zeros((3, 3), np.uint8), set()
        R.find_color(1, 1, z, st, took)
        assert st[1, 1] == want and branch in took and "agreed" in took
    z[1, 1, 1:] = 70                                      # 90 from every neighbour: between 70 and 100, nobody votes
    st, took = np.zeros((3, 3), np.uint8), set()
    R.find_color(1, 1, z, st, took)
    assert st[1, 1] == R.E and took == {"bare_between", "too_few_votes"}
    z[0, :, 0] = z[1, 0, 0] = 1                           # the row above and the west neighbour lie under hulls
    z[0, :, 1:] = 21
    z[1, 0, 1:] = 200
    z[1, 1, 1:] = 20
    st, took = np.zeros((3, 3), np.uint8), set()
    st[0, :] = R.B
    st[1, 0] = R.W
    R.find_color(1, 1, z, st, took)                       # NW and N are allies within 10 % (3 < 6), NE is not looked at (only
    assert st[1, 1] == R.B                                # the decided ones, NW, N and W, are), W is an enemy: 540 > 60 -> black
    assert took == {"ally", "hull_later", "enemy", "agreed"}
    st[0, 0] = R.E
    st[0, 1] = R.W                                        # NW undecided, N an "ally" that is white, W says black, and so does
    took = set()                                          # the bare east neighbour, 240 brighter: the third vote, two colours
    st[1, 1] = 0
    R.find_color(1, 1, z, st, took)
    assert st[1, 1] == R.E and took == {"hull_undecided", "ally", "hull_later", "enemy", "bare_darker", "disagreed"}


@pytest.mark.parametrize("name", STONE_NAMES)
def test_stone_case_takes_its_paths(stone_refs, name):
    out = stone_refs[name]
    took = R.stone_paths(out)
    missing = [p for p in K.STONE_PATHS[name] if p not in took]
    assert not missing, (name, missing)
    margin = R.stone_margins(out)
    print(name, "smallest margin of an inexact decision", margin)
    assert margin >= 1e-3                                 # float32 against float64 minAreaRect cannot decide a case


def test_stone_case_names_and_regions(stone_cases, stone_refs):
    assert sorted(stone_cases) == STONE_NAMES
    regions = {c["region"] for c in stone_cases.values()}
    assert regions >= set(K.REGIONS) and len(K.REGIONS) == 10
    views = {stone_refs[n]["record"]["view"] for n in STONE_NAMES}
    assert views == {(139, 139), (139, 140), (140, 139), (140, 140), (379, 379)}
    assert all(v[1] % 64 for v in views) and {v[0] % 4 for v in views} == {0, 3}
    for names in K.STONE_BATCHES.values():
        assert len({stone_cases[n]["region"] for n in names}) == 1
    names = K.STONE_BATCHES["batch_1_and_3_without_hull"]
    assert [not stone_refs[n]["mask"].any() for n in names] == [False, True, False, True]
    assert all(not stone_refs[n]["mask"].any() for n in K.STONE_BATCHES["batch_without_any_span"])


def test_rows_above_the_view_would_change_the_answer_if_read(stone_cases, stone_refs):
    """both cases give the answer of the cropped mask -- the same one --, and an opening that looked at the rows above the
    view would give another: with 0 there the blobs lose their first rows, with 255 they grow upwards"""
    rects = K.zones_of(K.posgrid())
    x0, y0 = int(rects[6, 6, 0]), int(rects[6, 6, 1])
    a, b = stone_cases["above_view_0"], stone_cases["above_view_255"]
    assert x0 >= 4 and not a["fg"][x0 - 4:x0].any() and b["fg"][x0 - 4:x0].all()
    assert np.array_equal(a["fg"][x0:], b["fg"][x0:]) and a["fg"][x0:x0 + 6].any(axis=1).all()
    for key in ("stones", "zones", "mask"):
        assert np.array_equal(stone_refs["above_view_0"][key], stone_refs["above_view_255"][key])
    h, w = stone_refs["above_view_0"]["record"]["view"]
    cropped = R.open_rows(a["fg"][x0:x0 + h, y0:y0 + w])
    for c in (a, b):
        read_above = R.open_rows(c["fg"])[x0:x0 + h, y0:y0 + w]
        assert not np.array_equal(read_above, cropped)
        zero_above = R.open_rows(np.vstack([np.zeros((4, w), np.uint8), c["fg"][x0:x0 + h, y0:y0 + w]]))[4:]
        assert not np.array_equal(zero_above, cropped)


def test_stone_reference_mutants_are_told_apart_by_the_cases(stone_cases, stone_refs):
    """the four one-line changes the library was also built with (see tests/test_gpu_stone_paths.py), made to the
    reference: each changes the answer of the case built for it, so the cases can tell the library's mutant too"""
    rects = K.zones_of(K.posgrid())
    for kw, name in ((dict(back=4), "above_view_0"), (dict(min_vert=11), "filters"), (dict(masked_on_equal=True), "filters"),
                     (dict(round_mean=True), "two_fifths")):
        c, ref = stone_cases[name], stone_refs[name]
        out = R.find_stones(c["img"], c["fg"], rects, *c["region"], **kw)
        assert not np.array_equal(out["zones"], ref["zones"]), kw


@pytest.mark.parametrize("name", STONE_NAMES)
def test_stone_reference_equals_oracle_on_case(stone_cases, stone_refs, ora, name):
    from oracle import ora_stones as S
    c, ref = stone_cases[name], stone_refs[name]
    stones, zones, mask, info = S.find_stones(c["img"], c["fg"], *c["region"], want_all=True)
    assert np.array_equal(ref["mask"], mask) and np.array_equal(ref["zones"], zones) and np.array_equal(ref["stones"], stones)
    assert ref["record"]["fg_kept"] == len(info["fg"])


def test_stone_reference_pieces_equal_oracle(ora):
    """opening, filled hull and the centre decision on random inputs: the chamfer distance here is a shortest-path search,
    the oracle's the library's two raster passes -- never below it, and the decision the same"""
    from oracle import ora_stones as S
    rng = np.random.default_rng(5)
    fg = (rng.random((40, 33)) < 0.8).astype(np.uint8) * 255
    assert np.array_equal(R.open_rows(fg), S.morph_open_rows(fg))
    for _ in range(30):
        pts = rng.integers(1, 50, (int(rng.integers(3, 20)), 2))
        hl = R.hull(map(tuple, pts))
        assert set(hl) == set(map(tuple, S.convex_hull(pts).tolist()))
        a, b = np.zeros((52, 52), np.uint8), np.zeros((52, 52), np.uint8)
        R.fill_hull(a, hl)
        S.fill_polygon(b, S.convex_hull(pts), 1)
        assert np.array_equal(a, b)
        lo, hi, _, rivals = R.min_rect(hl, want_rival=True)
        w, h, _ = S.min_area_rect_box(pts)
        assert abs(lo * hi - w * h) <= 1e-4 * lo * hi      # (every side of a triangle gives a rectangle of the same area)
        assert any(abs(r[0] - min(w, h)) <= 1e-4 * max(1, r[0]) and abs(r[1] - max(w, h)) <= 1e-4 * r[1] for r in rivals)
    for _ in range(10):
        box = np.full((int(rng.integers(12, 45)), int(rng.integers(12, 45))), 255, np.uint8)
        for y, x in zip(rng.integers(0, box.shape[0], 6), rng.integers(0, box.shape[1], 6)):
            box[y, x] = 0
        exact = R.chamfer(box)
        passes = np.round(S.distance_transform_5x5(box).astype(np.float64) * 65536).astype(np.int64)
        assert (passes >= exact).all()
        assert bool(R.find_centers(exact, 10.0)[0]) == bool(S.find_centers(passes, 10.0))


def test_stone_reference_equals_oracle_on_scenes(ora):
    """frames of the filmed game tests/test_gpu_stonefind.py uses (a hand over the board, fresh stones in the mask)"""
    from camkifu_amd import synth
    from oracle import ora_stones as S
    dst = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)
    film, corners, truth, moves, hands = synth.film(70, 480, 640, seed=synth.SEED, quiet=40, move_every=10, hand_frames=5)
    frames = film.numpy()
    M = ora.get_perspective_transform(corners, dst)
    model = ora.MOG2(380, 380, 3)
    rects = K.zones_of(K.posgrid())
    kept = 0
    for f in range(63):
        gob = ora.warp_perspective(frames[f], M)
        fg = model.apply(gob, 0.01 if f < 50 else 0.005)
        if f in (45, 52, 62):
            ref = R.find_stones(gob, fg, rects)
            stones, zones, mask, info = S.find_stones(gob, fg, want_all=True)
            assert np.array_equal(ref["mask"], mask) and np.array_equal(ref["zones"], zones) and np.array_equal(ref["stones"], stones)
            kept += len(info["fg"])
    assert kept >= 1

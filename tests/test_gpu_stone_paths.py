"""ck_find_intersections (k_gridlines.hip: gray_planes_hist_kernel, K2's Canny with per-image thresholds,
hough_zones_kernel, update_grid on the host), ck_contours_external (k_contours.hip: prep_rows_kernel / prep_rows4_kernel,
link / flatten / roots / border list kernels, trace_count_lds_kernel / trace_count_kernel) and ck_contour_stones
(k_stonefind.hip: fg_open_kernel, crop_bgr_kernel, paint_spans_kernel, zone_sums_kernel, the two Canny chains on the cropped
view; the host geometry of ck_stonegeom.cpp) held bit for bit to the plain references of tests/stone_ref.py on every case of
tests/stone_cases.py -- inputs built per path, each asserted to take its path in tests/test_stone_ref_cpu.py:

  find_intersections: the Canny map, the lines of every zone in the order found, the grid;
  contours_external:  start, vertex count and pixel set of every contour, in cv2's order;
  contour_stones:     stones, zones and the hull mask.

Every case runs from host memory and from device memory, the second run after a call of another size on the same context
(scratch that grew earlier is reused).  Refusals are checked by code and message, and the context must work afterwards.
The CK_ERR_STATE answer of ck_contour_stones has no case: no input reaches it (tests/stone_cases.py says why).

Mutants of the library this file was run against on an MI355X (one-line changes, each built as a library of its own, not
committed), one per row, with what caught it:

  wave_max_first keeps the LARGER angle among equals          test_find_intersections_case (12 of 13), _batches, _refuses
  votes taken back for a line found too short as well         test_find_intersections_case (9 cases), _batches[names0], _refuses
  first border neighbour searched counter-clockwise, both     test_contours_external_case (12 of 14, follower_lds_511x1024 and
  followers                                                   follower_global_512x1024 among them), _unaligned_device_pointer
  the opening's erosion reads row y - 4 instead of y - 3      test_contour_stones_case (15 of 17: all with a blob), _batches, _refusals
  `0.4 * area <= visible` in the zone decision                test_contour_stones_case (filters, two_fifths, whole_board, 3 regions)
  `nvert < 11` in the foreground filter                       test_contour_stones_case[filters], _batches[batch_1_and_3_without_hull]
  the zone mean rounded instead of truncated                  test_contour_stones_case (16 of 17: all but flat), _batches, _refusals
  `>=` for `>` in the xflag test                              equivalent: |a| = |b| only at 45 and 135 degrees, where both
                                                              walk forms visit the same pixels in the same order (asserted
                                                              in tests/test_stone_ref_cpu.py)
  the follower resumes one neighbour later (`dir + 5`)        equivalent, in either follower: that neighbour touches the
                                                              pixel before (asserted in tests/test_stone_ref_cpu.py)

A follower that merely starts its first search one direction off (from NW, N or NE instead of W) is equivalent as well:
the three pixels above the first pixel of a component are background.
"""
import numpy as np
import pytest

from . import align_cases as ac, stone_cases as K, stone_ref as R

pytestmark = pytest.mark.gpu
GRID_NAMES = sorted(K.GRID_PATHS)
CONTOUR_NAMES = sorted(K.contour_cases())
STONE_NAMES = sorted(K.STONE_PATHS)


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def grid_cases():
    return K.grid_cases()


@pytest.fixture(scope="module")
def grid_refs(grid_cases):
    return {name: R.find_intersections(c["img"], c["mtx"], c["rects"]) for name, c in grid_cases.items()}


@pytest.fixture(scope="module")
def contour_cases():
    return K.contour_cases()


@pytest.fixture(scope="module")
def contour_refs(contour_cases):
    return {name: [R.follow_contours(e) for e in batch] for name, batch in contour_cases.items()}


def _dev(a, misalign=0):
    """a device copy; with `misalign`, one that starts that many bytes past 16 bytes, between guard bands (tests/align_cases.py)"""
    import torch
    if not misalign:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = ac.place(a, misalign)
    assert out.data_ptr() % 4 == misalign % 4 and out.is_contiguous()
    return out


# ------------------------------------------------------------------------------------------------ grid lines
def _check_grid(got, ref, what):
    grid, found, edges = got
    assert np.array_equal(edges, ref["edges"]), what
    for key in sorted(set(found) | set(ref["found"])):
        assert found.get(key) == ref["found"].get(key), (what, key, ref["records"][key]["lines"])
    assert np.array_equal(grid, ref["grid"]), what


def _other_grid_call(ck, grid_cases, name):
    """a call with another image side (and other zone sizes) than `name`'s"""
    c = grid_cases["side_127" if grid_cases[name]["img"].shape[0] != 127 else "side_76"]
    ck.find_intersections(np.stack([c["img"]] * 2), c["mtx"], c["rects"])


@pytest.mark.parametrize("name", GRID_NAMES)
def test_find_intersections_case(ck, grid_cases, grid_refs, name):
    c, ref = grid_cases[name], grid_refs[name]
    _check_grid(ck.find_intersections(c["img"], c["mtx"], c["rects"], want_lines=True), ref, name + " host")
    _other_grid_call(ck, grid_cases, name)
    _check_grid(ck.find_intersections(_dev(c["img"]), c["mtx"], c["rects"], want_lines=True), ref, name + " device, again")
    assert np.array_equal(ck.find_intersections(c["img"], c["mtx"], c["rects"]), ref["grid"])


@pytest.mark.parametrize("names", [("sizes_fan_a", "negative_counters_hatch"), ("goban_default", "otsu_flat", "otsu_two_level", "otsu_flat")])
def test_find_intersections_batches(ck, grid_cases, grid_refs, names):
    """images of one zone table in one call: per-image thresholds (one of them 0 / 0), per-image line tables"""
    c0 = grid_cases[names[0]]
    assert all(np.array_equal(grid_cases[n]["rects"], c0["rects"]) for n in names)
    batch = np.stack([grid_cases[n]["img"] for n in names])
    for src in (batch, _dev(batch)):
        grid, found, edges = ck.find_intersections(src, c0["mtx"], c0["rects"], want_lines=True)
        for k, n in enumerate(names):
            _check_grid((grid[k], found[k], edges[k]), grid_refs[n], "%s in batch" % n)


def test_find_intersections_refuses_a_41_pixel_zone(ck, grid_cases, grid_refs):
    from camkifu_amd import capi
    c = grid_cases["sizes_fan_a"]
    with pytest.raises(capi.CkError, match="intersection zone of 41 pixels: at most 40") as err:
        ck.find_intersections(c["img"], c["mtx"], K.refused_table())
    assert err.value.code == capi.CK_ERR_ARG
    small = c["rects"].copy()
    small[0, 0] = (10, 10, 13, 30)
    with pytest.raises(capi.CkError, match="3 x 20 pixels, at least 4 x 4") as err:
        ck.find_intersections(c["img"], c["mtx"], small)
    assert err.value.code == capi.CK_ERR_ARG
    _check_grid(ck.find_intersections(c["img"], c["mtx"], c["rects"], want_lines=True), grid_refs["sizes_fan_a"], "after refusals")


# ------------------------------------------------------------------------------------------------ contours
def _check_contours(got, ref, what):
    assert len(got) == len(ref), what
    for f, (g_map, r_map) in enumerate(zip(got, ref)):
        assert [(c["start"], c["nvert"]) for c in g_map] == [(c["start"], c["nvert"]) for c in r_map], (what, f)
        for g, r in zip(g_map, r_map):
            pix = set(map(tuple, g["pix"].tolist()))
            assert len(pix) == len(g["pix"]) and pix == r["pix"], (what, f, r["start"])


@pytest.mark.parametrize("name", CONTOUR_NAMES)
def test_contours_external_case(ck, contour_cases, contour_refs, name):
    batch, ref = contour_cases[name], contour_refs[name]
    _check_contours(ck.contours_external(batch, want_points=True), ref, name + " host")
    other = contour_cases["noise_odd_width" if name != "noise_odd_width" else "shapes"]
    ck.contours_external(other)
    _check_contours(ck.contours_external(_dev(batch), want_points=True), ref, name + " device, again")
    one = ck.contours_external(batch[-1])
    assert [(c["start"], c["nvert"]) for c in one] == [(c["start"], c["nvert"]) for c in ref[-1]]


@pytest.mark.parametrize("name", ["seams_w64", "seams_w96", "shapes"])
def test_contours_external_from_an_unaligned_device_pointer(ck, contour_cases, contour_refs, name):
    """w % 4 == 0 but the map starts 1, 2 or 3 bytes past a dword: prep_rows_kernel instead of prep_rows4_kernel"""
    batch = contour_cases[name]
    assert batch.shape[2] % 4 == 0
    for off in (1, 2, 3):
        maps = _dev(batch, misalign=off)
        _check_contours(ck.contours_external(maps, want_points=True), contour_refs[name], "%s + %d" % (name, off))
        ac.untouched(maps)
        ac.unchanged(maps, batch)


def test_contours_external_refusals(ck, contour_cases, contour_refs):
    from camkifu_amd import capi
    with pytest.raises(capi.CkError, match="edge map smaller than 3x3") as err:
        ck.contours_external(np.full((2, 2, 9), 255, np.uint8))
    assert err.value.code == capi.CK_ERR_ARG
    _check_contours(ck.contours_external(contour_cases["shapes"], want_points=True), contour_refs["shapes"], "after a refusal")


# ------------------------------------------------------------------------------------------------ contour stones
RECTS = K.zones_of(K.posgrid())


@pytest.fixture(scope="module")
def stone_cases():
    return K.stone_cases()


@pytest.fixture(scope="module")
def stone_refs(stone_cases):
    return {name: R.find_stones(c["img"], c["fg"], RECTS, *c["region"]) for name, c in stone_cases.items()}


def _check_stones(got, ref, what):
    stones, zones, mask = got
    assert np.array_equal(mask, ref["mask"]), what
    assert np.array_equal(zones, ref["zones"]), (what, np.argwhere((zones != ref["zones"]).any(-1))[:5].tolist())
    assert np.array_equal(stones, ref["stones"]), what


def _other_stones_call(ck, stone_cases, name):
    """a call on a view of another size than `name`'s, two images"""
    c = stone_cases["region_r6_c12" if stone_cases[name]["region"] == (0, K.GS, 0, K.GS) else "whole_board"]
    ck.contour_stones(np.stack([c["img"]] * 2), np.stack([c["fg"]] * 2), RECTS, *c["region"])


@pytest.mark.parametrize("name", STONE_NAMES)
def test_contour_stones_case(ck, stone_cases, stone_refs, name):
    c, ref = stone_cases[name], stone_refs[name]
    _check_stones(ck.contour_stones(c["img"], c["fg"], RECTS, *c["region"], want_all=True), ref, name + " host")
    _other_stones_call(ck, stone_cases, name)
    _check_stones(ck.contour_stones(_dev(c["img"]), _dev(c["fg"]), RECTS, *c["region"], want_all=True), ref, name + " device, again")
    assert np.array_equal(ck.contour_stones(c["img"], c["fg"], RECTS, *c["region"]), ref["stones"])


@pytest.mark.parametrize("batch", sorted(K.STONE_BATCHES))
def test_contour_stones_batches(ck, stone_cases, stone_refs, batch):
    """images of one region in one call: images without any hull between images with hulls (their spans are skipped, their
    zones all bare), and a call without a single span (nothing to paint)"""
    names = K.STONE_BATCHES[batch]
    region = stone_cases[names[0]]["region"]
    img = np.stack([stone_cases[n]["img"] for n in names])
    fg = np.stack([stone_cases[n]["fg"] for n in names])
    for src in ((img, fg), (_dev(img), _dev(fg))):
        stones, zones, mask = ck.contour_stones(src[0], src[1], RECTS, *region, want_all=True)
        for k, n in enumerate(names):
            _check_stones((stones[k], zones[k], mask[k]), stone_refs[n], "%s in %s" % (n, batch))


def test_contour_stones_refusals(ck, stone_cases, stone_refs):
    from camkifu_amd import capi
    c = stone_cases["region_r0_c0"]
    far = RECTS.copy()
    far[1, 1] = (300, 300, 320, 320)
    with pytest.raises(capi.CkError, match=r"zone \(1, 1\) does not lie inside the analysed view") as err:
        ck.contour_stones(c["img"], c["fg"], far, *c["region"])
    assert err.value.code == capi.CK_ERR_ARG
    thin = RECTS.copy()
    thin[:, :, 2] = thin[:, :, 0] + 2
    with pytest.raises(capi.CkError, match=r"zone rectangles give a 2 x 20 view at \(0, 0\) of a 380 image") as err:
        ck.contour_stones(c["img"], c["fg"], thin, 0, 1, 0, 1)
    assert err.value.code == capi.CK_ERR_ARG
    _check_stones(ck.contour_stones(c["img"], c["fg"], RECTS, *c["region"], want_all=True), stone_refs["region_r0_c0"], "after refusals")

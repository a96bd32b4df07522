"""The plain references of K1 / K2 (tests/filter_ref.py) pinned from three sides, and the inputs of tests/test_gpu_filters.py
checked for what they were built for, without a GPU:

  * the three forms of the median agree with each other, and the references equal the CPU restatement in C (`ora`) for every
    window 3 .. 17 and for Canny / Otsu / goban_canny / board_edges on every case of tests/filter_cases.py, a 1080p scene included;
  * maps worked by hand: a constant, a vertical and a horizontal step, the tie rules;
  * every case has the property it was built for, asserted with the model of the median kernel's path choice and the model of
    the tiled hysteresis (filter_cases.median_paths, tiled_hysteresis) and the reference alone.  A case that misses its
    property FAILS as a bad input;
  * the mutants of the GPU file's list that can be applied to the reference or a model change the result on these inputs."""
import numpy as np
import pytest
from scipy import ndimage

from tests import filter_cases as fc
from tests import filter_ref as fr

MEDIAN_CASES = fc.median_cases()
CANNY_CASES = fc.canny_cases()
GOBAN_CASES = fc.goban_cases()
BOARD_CASES = fc.board_cases()
_ids = lambda cases: [c[0] for c in cases]


# ------------------------------------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("k", [3, 5, 7, 9, 11, 13, 15, 17])
def test_the_median_forms_agree(ora, k):
    rng = np.random.default_rng(k)
    imgs = [rng.integers(0, 256, (23, 37, 3), dtype=np.uint8), fc.smooth(k, 40, 31), rng.integers(0, 2, (19, 26, 3), dtype=np.uint8) * 255,
            np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3), fc.flat_noise(k, 30, 50, 253, 2)]
    for img in imgs:
        want = fr.median_rank(img, k)
        assert np.array_equal(fr.median_counting(img, k), want)
        assert np.array_equal(fr.median_partition(img, k), want)
        assert np.array_equal(ora.median(img, k), want)
    big = fc.smooth(50 + k, 170, 203)
    assert np.array_equal(fr.median_counting(big, k), fr.median_rank(big, k))
    plane = imgs[0][..., 0]
    assert np.array_equal(fr.median(plane, k), fr.median(imgs[0], k)[..., 0])


def test_median_by_hand():
    img = np.zeros((5, 5, 1), np.uint8)
    img[2, 2] = 9
    assert not fr.median(img, 3).any()                                  # one outlier vanishes
    img[:, :3] = 7
    assert np.array_equal(fr.median(img, 3)[..., 0], np.repeat([[7, 7, 7, 0, 0]], 5, 0))   # a straight edge stays where it is
    corner = np.zeros((6, 6, 1), np.uint8)
    corner[:3, :3] = 5
    # the block's free corner (2, 2) sees 4 of 9 pixels of the block: it goes; (0, 0) sees the replicated corner: it stays
    out = fr.median(corner, 3)[..., 0]
    assert out[2, 2] == 0 and out[0, 0] == 5 and out[2, 1] == 5 and out[1, 2] == 5 and out[3, 1] == 0


def test_canny_by_hand():
    flat = np.full((16, 16, 3), 100, np.uint8)
    res = fr.canny(flat, 25, 75)
    assert not res["edges"].any() and (res["map"] == 1).all() and not res["mag"].any()
    step = np.zeros((16, 16, 3), np.uint8)
    step[:, 8:] = 200
    res = fr.canny(step, 25, 75)
    # columns 7 and 8 both have magnitude 800: `>` towards the left, `>=` towards the right keeps the left one only
    assert (res["mag"][:, 7] == 800).all() and (res["mag"][:, 8] == 800).all() and (res["dx"][:, 7] == 800).all()
    assert (res["map"][:, 7] == 2).all() and (res["map"][:, 8] == 1).all() and res["edges"].sum() == 255 * 16
    res = fr.canny(step, 25, 75, sector0_strict=True)
    assert not res["edges"].any()
    res = fr.canny(np.ascontiguousarray(step.transpose(1, 0, 2)), 25, 75)
    assert (res["map"][7] == 2).all() and (res["map"][8] == 1).all() and (res["dy"][7] == 800).all() and res["edges"].sum() == 255 * 16
    # equal channels: the first one is chosen; a larger one later wins
    assert not fr.canny(step, 25, 75)["channel"].any()
    assert (fr.canny(step, 25, 75, first_channel=False)["channel"][:, 7] == 2).all()
    step[:, 8:, 1] = 201
    assert (fr.canny(step, 25, 75)["channel"][:, 7] == 1).all()
    # weak alone is no edge; low > high swaps; thresholds are exclusive
    assert not fr.canny(step, 804, 900)["edges"].any() and (fr.canny(step, 700, 803)["map"][:, 7] == 2).all()
    assert (fr.canny(step, 700, 804)["map"][:, 7] == 0).all() and not fr.canny(step, 700, 804)["edges"].any()
    assert np.array_equal(fr.canny(step, 803, 700)["map"], fr.canny(step, 700, 803)["map"])


def test_grey_and_otsu(ora):
    assert fr.bgr2gray(np.uint8([[[255, 255, 255]], [[0, 0, 0]], [[255, 0, 0]], [[0, 255, 0]], [[0, 0, 255]]])).ravel().tolist() == [255, 0, 29, 150, 76]
    two = np.repeat(np.uint8([10, 200]), 50)
    assert fr.otsu_level(two) == 10.0                                   # every level 10 .. 199 separates alike: the first wins
    assert fr.otsu_level(np.full(100, 77, np.uint8)) == 0.0             # one class only: nothing is ever a maximum
    rng = np.random.default_rng(3)
    for k in range(6):
        img = fc.smooth(k, 50, 60) if k % 2 else rng.integers(0, 256, (50, 60, 3), dtype=np.uint8) // (k + 1)
        assert np.array_equal(fr.bgr2gray(img), ora.bgr2gray(img))
        assert fr.otsu_level(fr.bgr2gray(img)) == ora.otsu_level(ora.bgr2gray(img))


# ------------------------------------------------------------------------------------------------ K1 cases
@pytest.mark.parametrize("case", MEDIAN_CASES, ids=_ids(MEDIAN_CASES))
def test_median_cases_reference_equals_restatement_and_property_holds(ora, case):
    name, k, frames, wants = case
    n = {}
    for f in frames:
        assert np.array_equal(fr.median(f, k), ora.median(f, k)), name
        for key, v in fc.count_paths(fc.median_paths(f, k)).items():
            n[key] = n.get(key, 0) + v
    print(name, {a: b for a, b in n.items() if b})
    for key, least in wants.items():
        assert n[key] >= least, "bad input: %s has %d of class %s, wants %d" % (name, n[key], key, least)


def test_range_ends_are_reached_by_both_paths():
    """medians 0 and 255 out of the radix descent (a minority of the opposite extreme makes the samples span 255 levels) and out
    of scans (constants, near-constants)"""
    _, k, frames, _ = next(c for c in MEDIAN_CASES if c[0] == "ends")
    seen = set()
    for f in frames:
        med = fr.median(f, k)
        for c, tiles in enumerate(fc.median_paths(f, k)):
            for (by, bx), t in tiles.items():
                part = med[by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48, c]
                for v in (0, 255):
                    if (part == v).any():
                        seen.add((t["path"], v))
    assert {("radix", 0), ("radix", 255), ("scan", 0), ("scan", 255)} <= seen


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11, 13, 15, 17])
def test_window_sizes_sit_at_the_interior_condition(k):
    big, at, less_w, less_h = fc.window_sizes(k)
    inner = lambda shape: [(by, bx) for by in range(-(-shape[0] // 48)) for bx in range(-(-shape[1] // 48)) if fc.is_interior(shape[0], shape[1], k, by, bx)]
    assert inner(at) == [(1, 1)] and inner(less_w) == [] and inner(less_h) == []
    rows, cols = {by for by, _ in inner(big)}, {bx for _, bx in inner(big)}
    assert len(rows) >= 2 and len(cols) >= 2 and big[1] % 4 != 0
    assert {fc.window_sizes(kk)[0][1] % 4 for kk in (3, 5, 7)} == {1, 2, 3}


def test_batches_are_unaligned_and_meet_both_tile_orders():
    h, w = fc.BATCH_SHAPE
    assert (h * w * 3) % 4 != 0 and (h * w) % 2 == 1
    tiles = -(-h // 48) * -(-w // 48)
    sizes = {c[0]: len(c[2]) for c in MEDIAN_CASES if c[0].startswith("batch")}
    assert (tiles * 3 * sizes["batch3"]) % 8 != 0 and (tiles * 3 * sizes["batch4"]) % 8 == 0 and sizes["batch3"] >= 3
    a, b = (next(c for c in MEDIAN_CASES if c[0] == n)[2] for n in ("batch3", "batch4"))
    assert np.array_equal(a, b[:3])                                      # the same content both ways
    nms = lambda shape, n: -(-shape[0] // fc.NTH) * -(-shape[1] // fc.NTW) * n
    odd = {c[0]: c[1] for c in CANNY_CASES if c[0].startswith("odd_batch")}
    assert nms(odd["odd_batch3"].shape[1:3], 3) % 8 != 0 and nms(odd["odd_batch4"].shape[1:3], 4) % 8 == 0
    assert (odd["odd_batch3"].shape[1] * odd["odd_batch3"].shape[2]) % 2 == 1 and odd["odd_batch3"].shape[2] % 4 != 0
    gob = {c[0]: c[1] for c in GOBAN_CASES}
    assert nms(fc.CHAIN_SHAPE, len(gob["chains"])) % 8 != 0 and nms(fc.CHAIN_SHAPE, len(gob["chains_remap"])) % 8 == 0


# ------------------------------------------------------------------------------------------------ K2 cases
def _same_canny(ora, img, low, high, res):
    e, m, mag, dx, dy = ora.canny(img, low, high, want_map=True)
    assert np.array_equal(res["map"], m) and np.array_equal(res["edges"], e)
    assert np.array_equal(res["mag"], mag) and np.array_equal(res["dx"], dx) and np.array_equal(res["dy"], dy)


def _interior_nms_tiles(h, w):
    return [(by, bx) for by in range(-(-h // fc.NTH)) for bx in range(-(-w // fc.NTW))
            if bx * 64 >= 8 and bx * 64 + 72 <= w and by * 28 >= 2 and by * 28 + 30 <= h]


@pytest.mark.parametrize("case", CANNY_CASES, ids=_ids(CANNY_CASES))
def test_canny_cases_reference_equals_restatement(ora, case):
    name, frames, low, high = case
    for f in frames:
        res = fr.canny(f, low, high)
        _same_canny(ora, f, low, high, res)
        assert np.array_equal(fc.tiled_hysteresis(res["map"]), res["edges"])


def test_map_cases_fill_interior_tiles():
    by_name = {c[0]: c for c in CANNY_CASES}
    for name in ("noise", "noise_dense", "texture", "equal_channels", "odd_batch3"):
        _, frames, low, high = by_name[name]
        h, w = frames.shape[1:3]
        inner = _interior_nms_tiles(h, w)
        assert len(inner) >= 2, name
        for f in frames[:1]:
            m = fr.canny(f, low, high)["map"]
            counts = [(m[by * 28:(by + 1) * 28, bx * 64:(bx + 1) * 64] != 1).sum() for by, bx in inner]
            print(name, "candidates per interior tile", min(counts), max(counts))
            assert min(counts) >= (300 if name == "noise_dense" else 20), name
    # ties between the channels inside an interior tile, resolved for the first channel
    _, frames, low, high = by_name["equal_channels"]
    res = fr.canny(frames[0], low, high)
    assert not res["channel"].any() and (res["map"] != 1).sum() > 500
    assert (fr.canny(frames[0], low, high, first_channel=False)["channel"] == 2).all()
    assert _interior_nms_tiles(58, 136) == [(1, 1)] and not _interior_nms_tiles(57, 136) and not _interior_nms_tiles(58, 135)


@pytest.mark.parametrize("chain", fc.CHAINS, ids=[c[0] for c in fc.CHAINS])
def test_chain_cases(chain):
    """one 8-connected component of candidates, at least 5 NMS tiles long, strong pixels in ONE tile: all of it is edge, and
    none of it without them; the links between tiles it was drawn for are there.  The same for the Otsu thresholds, on the map
    the reference computes behind its two medians."""
    name, *_, kinds = chain
    for how in ("fixed", "otsu"):
        maps = []
        for strong in (True, False):
            if how == "fixed":
                res = fr.canny(fc.chain_image(name, strong), 25, 75)
            else:
                res = fr.goban_canny(fc.goban_chain_image(name, strong))
                assert (res["low"], res["high"]) == (50, 100)
            maps.append(res)
            m = res["map"]
            assert ndimage.label(m != 1, structure=np.ones((3, 3)))[1] == 1, (name, how)
            ys, xs = np.nonzero(m != 1)
            assert len({(y // fc.NTH, x // fc.NTW) for y, x in zip(ys, xs)}) >= 5, (name, how)
            ys, xs = np.nonzero(m == 2)
            assert len({(y // fc.NTH, x // fc.NTW) for y, x in zip(ys, xs)}) == (1 if strong else 0), (name, how)
            assert np.array_equal(res["edges"] > 0, (m != 1) if strong else np.zeros_like(m, bool)), (name, how)
            cross = fc.crossings(m)
            assert all(cross.get(kind, 0) >= 1 for kind in kinds), (name, how, cross)


def test_the_chains_cross_every_kind_of_border():
    seen = set()
    for name, *_ in fc.CHAINS:
        seen |= set(fc.crossings(fr.canny(fc.chain_image(name), 25, 75)["map"]))
    assert seen >= {"W_side", "N_top", "NW_corner", "NW_side", "NW_top", "NE_corner", "NE_side", "NE_top"}, seen


# ------------------------------------------------------------------------------------------------ the two chains of calls
@pytest.mark.parametrize("case", GOBAN_CASES, ids=_ids(GOBAN_CASES))
def test_goban_cases_reference_equals_restatement(ora, case):
    name, frames = case
    seen = set()
    for f in frames:
        key = f.tobytes()
        if key in seen:
            continue
        seen.add(key)
        res = fr.goban_canny(f)
        e, otsu = ora.goban_canny(f, want_otsu=True)
        assert res["otsu"] == otsu and np.array_equal(res["edges"], e), name


@pytest.mark.parametrize("case", BOARD_CASES, ids=_ids(BOARD_CASES))
def test_board_cases_reference_equals_restatement(ora, case):
    name, frames = case
    for f in frames:
        res = fr.board_edges(f)
        assert np.array_equal(res["median"], ora.median(f, 15)), name
        assert np.array_equal(res["edges"], ora.canny(res["median"], 25, 75)), name


def _range_spans(paths):
    """-> {tile: hi - lo, the largest over the channels}"""
    return {key: max(p[key]["hi"] - p[key]["lo"] for p in paths) for key in paths[0]}


def test_blob_cases_have_edges_in_tiles_of_span_one():
    _, frames = next(c for c in GOBAN_CASES if c[0] == "blobs")
    for f, level in zip(frames, (4.0, 3.0, 2.0)):
        res = fr.goban_canny(f)
        assert res["otsu"] == level
        spans = _range_spans(fc.median_paths(fr.median(f, 13), 7))
        n = sum(1 for (by, bx), s in spans.items() if s == 1 and res["edges"][by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48].any())
        print("Otsu %r thresholds (%d, %d): %d edge pixels, %d range tiles of span 1 with edges" % (level, res["low"], res["high"], (res["edges"] > 0).sum(), n))
        assert n >= 16, "bad input"


def test_striped_case_gives_up_in_the_second_median():
    _, frames = next(c for c in GOBAN_CASES if c[0] == "striped")
    for f in frames:
        res = fr.goban_canny(f)
        assert (res["otsu"], res["low"], res["high"]) == (140.0, 70, 140)
        n = fc.count_paths(fc.median_paths(fr.median(f, 13), 7))
        print("median 7 behind median 13: gave up going down in", n["gave_up_down"], "of", n["tiles"])
        assert n["gave_up_down"] >= 8 and (res["edges"] > 0).sum() > 1000, "bad input"


def test_bounds_left_by_an_abandoned_scan_would_still_hold():
    """why 'the bounds of an abandoned scan kept on give-up' is no mutant that a result can show: going up, the scan leaves
    hi = 255 and lo = 0 or g0 + 1 (no median was <= g0); going down, lo = 0 (a block was still scanning) and hi = the end of
    the finished upward scan.  Both hold for every median of the tile -- on every tile of these cases that gives up."""
    seen = {"up": 0, "down": 0}
    jobs = [(f, k) for name, k, frames, _ in MEDIAN_CASES if name in ("hidden_up", "hidden_down", "hidden_inside", "cap", "ends") for f in frames]
    jobs += [(fr.median(f, 13), 7) for f in next(c for c in GOBAN_CASES if c[0] == "striped")[1]]
    for f, k in jobs:
        for tiles in fc.median_paths(f, k, keep_bounds_on_give_up=True):
            for t in tiles.values():
                if t["path"] == "gave_up":
                    seen[t["gave_up_dir"]] += 1
                    assert t["lo"] <= t["min"] and t["max"] <= t["hi"], t
    assert seen["up"] >= 100 and seen["down"] >= 100, seen


def test_span5_case_hangs_weak_tiles_on_a_strong_neighbour():
    """board thresholds: NMS tiles all of whose range tiles span exactly 5 levels (30 > 25: not to be skipped; a bound one level
    tighter would skip them) hold edge pixels but no strong one"""
    _, frames = next(c for c in BOARD_CASES if c[0] == "span5")
    for f in frames[:2]:
        res = fr.board_edges(f)
        paths = fc.median_paths(f, 15)
        h, w = f.shape[:2]
        hanging = 0
        tight = fc.flat_nms_tiles(fc.median_paths(f, 15, lo_plus=3), h, w, 25) & ~fc.flat_nms_tiles(paths, h, w, 25)
        for by, bx in zip(*np.nonzero(tight)):
            part = np.s_[by * 28:(by + 1) * 28, bx * 64:(bx + 1) * 64]
            hanging += bool(res["edges"][part].any() and not (res["map"][part] == 2).any())
        print("NMS tiles of span 5 with edge pixels and no strong one:", hanging)
        assert hanging >= 8, "bad input"
    assert max(t["hit254"] for p in fc.median_paths(frames[1], 15) for t in p.values())


# ------------------------------------------------------------------------------------------------ mutants
def test_the_cases_tell_the_mutants_apart():
    """the mutants of tests/test_gpu_filters.py's list that have a counterpart in the reference or the models: each changes the
    result on the inputs the GPU file runs"""
    caught = {}

    def count(name, differs):
        caught[name] = caught.get(name, 0) + int(bool(differs))

    # tie rules and channel order in the reference (K2: key_of tags reversed; m2 = m in sector 0)
    for name, frames, low, high in CANNY_CASES:
        if name in ("equal_channels", "texture", "noise"):
            plain = fr.canny(frames[0], low, high)
            count("last_channel", not np.array_equal(fr.canny(frames[0], low, high, first_channel=False)["map"], plain["map"]))
            count("sector0_strict", not np.array_equal(fr.canny(frames[0], low, high, sector0_strict=True)["map"], plain["map"]))
    # the link kernel's skip rule and the tile-local NE link, in the model of the tiled hysteresis
    for name, *_ in fc.CHAINS:
        res = fr.canny(fc.chain_image(name), 25, 75)
        for mutant, how in (("skip_last_column", dict(skip_last_column=True)), ("skip_top_row", dict(skip_top_row=True)), ("no_local_ne", dict(local_ne=False))):
            count(mutant, not np.array_equal(fc.tiled_hysteresis(res["map"], **how), res["edges"]))
    # the bounds of K1 and the flat test of K2, in the model of the path choice
    jobs = [(f, fr.board_edges(f), None) for f in next(c for c in BOARD_CASES if c[0] == "span5")[1][:2]]
    for f in next(c for c in GOBAN_CASES if c[0] == "blobs")[1][:1]:
        jobs.append((fr.median(f, 13), fr.goban_canny(f), 7))
    for f, res, k in jobs:
        src, kk = (f, 15) if k is None else (f, k)
        h, w = src.shape[:2]
        plain = fc.median_paths(src, kk)
        same = fc.canny_with_skips(res["median"], res["low"], res["high"], fc.flat_nms_tiles(plain, h, w, res["low"]))
        assert np.array_equal(same["edges"], res["edges"]) and np.array_equal(same["map"], res["map"])      # right bounds skip nothing that matters
        for mutant, how in (("lo_plus_3", dict(lo_plus=3)), ("hi_minus_1", dict(hi_minus=1)), ("top_at_254", dict(top_at_254=True))):
            flat = fc.flat_nms_tiles(fc.median_paths(src, kk, **how), h, w, res["low"])
            count(mutant, not np.array_equal(fc.canny_with_skips(res["median"], res["low"], res["high"], flat)["edges"], res["edges"]))
        for mutant, how in (("flat_slack_6", dict(slack=6)), ("flat_first_tile_only", dict(first_only=True))):
            flat = fc.flat_nms_tiles(plain, h, w, res["low"], **how)
            count(mutant, not np.array_equal(fc.canny_with_skips(res["median"], res["low"], res["high"], flat)["edges"], res["edges"]))
    print(caught)
    assert len(caught) == 10 and all(n > 0 for n in caught.values()), caught

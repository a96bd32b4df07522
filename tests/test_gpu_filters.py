"""K1 (k_median.hip: ck.median / median15) and K2 (k_canny.hip: ck.canny edges AND map), and the two chains of calls built from
them (ck.goban_canny edges and Otsu level, ck.board_edges), against the plain references of tests/filter_ref.py, BIT FOR BIT, on
the inputs of tests/filter_cases.py -- each built for one of the kernels' own branches, and each checked for that property
without a GPU in tests/test_filter_ref_cpu.py:

  K1  hidden content (the sampled pixels say 'flat', the medians are elsewhere: the scan gives up, upwards and downwards);
      scans of exactly 12 thresholds that finish and scans that need a 13th, both ways; scans that run into 254 and into 0 in
      interior and rim tiles, medians 0 and 255 out of the radix descent; every window 3 .. 17 on noise, smooth and flat content
      at a size with interior tiles both ways, at the smallest size with an interior tile and one pixel below it in w and in
      h, widths of every residue mod 4; batches whose frames start off a dword, with and without the remapped tile order;
  K2  noise, dense candidates, hard 0 / 255 texture and equal channels in interior NMS tiles; sizes at the interior
      condition's edge; batches of odd h w; weak chains several NMS tiles long that reach their strong pixels, all in ONE
      tile, through every kind of border between tiles (W, N, NW and NE through a side, the top and a corner), and the same
      chains without strong pixels; fixed thresholds (a frame >= 1 of a batch) and per-frame Otsu thresholds;
  bounds  what K1 hands to K2 to skip flat tiles: blob outlines of one level under Otsu thresholds of 1 .. 4, and for the
      board thresholds a weak diagonal chain in tiles of span exactly 5 that hangs on strong pixels tiles away, at mid-grey
      and at the top of the range; stripes that make the SECOND median of goban_canny give up.
Every call is made with host and with device-resident input, and once more on the same context after a call of another
size (the scratch buffers -- bounds, candidate lists, counters -- are reused across calls).

Mutants of the kernels that must each fail this file.  Each was built as a library of its own and run once against this
file on an MI355X; what failed (of 73, 74 from the kept-bounds row on; names in brackets are cases; `chain` = test_the_median_cases_through_the_board_chain):
  K1  no reset of med[][][] when a scan gives up          6: median [hidden_down, ends, batch3, batch4], board [ends], chain.
                                                             (Going UP the leftovers are below every median and the descent
                                                             repairs them: hidden_up passes; going down they are not.)
      lo_bound = thr + 3                                   2: goban [blobs], board [span5]
      hi_bound = top - 1                                   2: goban [blobs], board [span5]
      top = thr - 1 also when the scan ran into 254        1: board [span5] (its frame at the top of the range)
      a wrong v_perm selector in the interior loads, K = 3 2: median [k3_166x202, k3_111x113]
      the same, K = 5                                      3: median [k5_163x201, k5_110x112, batch3_k5]
      the rim path's replicate clamp one pixel short      47: every median case, goban [chains, chains_remap, mix], board
                                                             [chains, ends], chain
      the remap's channel term (t % 3) dropped from bzi    5: median [batch4, batch4_k7], goban [blobs, chains_remap], board
                                                             [scene_1080p] -- the grids that are multiples of 8
      the bounds of an abandoned scan kept on give-up      0: EQUIVALENT.  What the kernel's expressions hold at that point
                                                             are still bounds: going up hi = 255 and lo = 0 or g0 + 1 (no
                                                             median was <= g0); going down lo = 0 and hi = the end of the
                                                             finished upward scan.  (0, 255) is only looser.  tests/
                                                             test_filter_ref_cpu.py::test_bounds_left_by_an_abandoned_scan_
                                                             would_still_hold asserts it on every tile here that gives up.
  K2  the flat test as 6 (hi - lo) <= low + 6              2: goban [blobs], board [span5]
      the flat test reading only the first range tile      6: goban [blobs, chains, chains_remap], board [span5, chains,
                                                             scene_1080p]
      the link kernel also skipping column NTW - 1         9: canny [equal_channels, edge_58x136, chain_up_right_strong,
                                                             chain_steep_up_right_strong], goban [chains, chains_remap],
                                                             board [chains, ends], chain
      the link kernel also skipping y % NTH == 0          20: canny [texture, equal_channels, the four edge_ sizes, odd_batch3,
                                                             odd_batch4, every _strong chain but the horizontal one], goban
                                                             [chains, chains_remap, striped], board [span5, chains, ends], chain
      the NE link dropped in the tile-local pass          17: canny [texture, equal_channels, edge_ sizes, odd batches,
                                                             chain_up_right_strong, chain_steep_up_right_strong], goban
                                                             [blobs, chains, chains_remap, mix], board [chains, ends], chain
      key_of tags reversed (the last channel wins a tie)  25: canny [all but equal_channels -- where every channel gives the
                                                             same dx, dy -- i.e. noise, textures, edge_ sizes, odd batches,
                                                             all twelve chains through their noise frame], goban [mix],
                                                             board [ends], chain
      m2 = m in sector 0 (`>` on both sides)              33: every canny case, goban [all], board [all], chain
      thr[2 f] read with the unpermuted blockIdx.z         2: goban [chains_remap, mix] -- the grids that are multiples of 8
Ten of these have a counterpart in the reference or in a model, which tests/test_filter_ref_cpu.py::
test_the_cases_tell_the_mutants_apart applies to these inputs.  Mutants that would read or write outside a buffer or could
hang (a wider interior condition, a longer list) were not built: the sizes at the conditions' edges stand for them.

The model of K1's path choice was confirmed once by a build with -DMED_DBG=1: see the table in tests/filter_cases.py."""
import numpy as np
import pytest

from tests import filter_cases as fc
from tests import filter_ref as fr

pytestmark = pytest.mark.gpu
MEDIAN_CASES = fc.median_cases()
CANNY_CASES = fc.canny_cases()
GOBAN_CASES = fc.goban_cases()
BOARD_CASES = fc.board_cases()
_ids = lambda cases: [c[0] for c in cases]


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _both_ways(call, frames, other):
    """-> the results of call(frames) with host input, with device input, and again with host input after `other()` has used
    the context at another size"""
    import torch
    yield "host", call(frames)
    yield "device", call(torch.from_numpy(frames).cuda())
    other()
    yield "again", call(frames)


def _other_size(ck, k=0):
    """a call of another size through the same scratch buffers: a larger frame of noise (bounds, lists and counters all in use)"""
    img = fc.noise(77 + k, 90, 410)
    return lambda: (ck.board_edges(np.stack([img, img[::-1].copy()])), ck.goban_canny(img))


@pytest.mark.parametrize("case", MEDIAN_CASES, ids=_ids(MEDIAN_CASES))
def test_median_equals_the_plain_reference(ck, case):
    name, k, frames, _ = case
    want = np.stack([fr.median(f, k) for f in frames])
    for how, got in _both_ways(lambda a: ck.median(a, k), frames, _other_size(ck, k)):
        got = _np(got)
        for j in range(len(frames)):
            assert np.array_equal(got[j], want[j]), (name, how, "frame %d: %d bytes differ" % (j, (got[j] != want[j]).sum()))
    if k == 15:
        assert np.array_equal(ck.median15(frames), want), name
        assert np.array_equal(ck.median15(frames[-1]), want[-1]), name          # a frame on its own: another grid


@pytest.mark.parametrize("case", CANNY_CASES, ids=_ids(CANNY_CASES))
def test_canny_edges_and_map_equal_the_plain_reference(ck, case):
    name, frames, low, high = case
    want = [fr.canny(f, low, high) for f in frames]
    for how, (edges, m) in _both_ways(lambda a: ck.canny(a, low, high, want_map=True), frames, _other_size(ck)):
        edges, m = _np(edges), _np(m)
        for j, w in enumerate(want):
            assert np.array_equal(m[j], w["map"]), (name, how, "frame %d: %d map bytes differ" % (j, (m[j] != w["map"]).sum()))
            assert np.array_equal(edges[j], w["edges"]), (name, how, "frame %d: %d edge bytes differ" % (j, (edges[j] != w["edges"]).sum()))
    if name.startswith("chain_"):
        chain = want[1]["map"] != 1
        assert np.array_equal(_np(ck.canny(frames, low, high))[1] > 0, chain if name.endswith("_strong") else np.zeros_like(chain))


@pytest.mark.parametrize("case", GOBAN_CASES, ids=_ids(GOBAN_CASES))
def test_goban_canny_equals_the_plain_reference(ck, case):
    name, frames = case
    cache = {}
    want = [cache.setdefault(f.tobytes(), fr.goban_canny(f)) for f in frames]
    for how, (edges, otsu) in _both_ways(lambda a: ck.goban_canny(a, want_otsu=True), frames, _other_size(ck)):
        edges = _np(edges)
        for j, w in enumerate(want):
            assert otsu[j] == w["otsu"], (name, how, j, otsu[j], w["otsu"])
            assert np.array_equal(edges[j], w["edges"]), (name, how, "frame %d: %d edge bytes differ" % (j, (edges[j] != w["edges"]).sum()))
    # the chain of calls in parts gives the same: median 13, median 7 (bytes) and Canny with the reference's thresholds (map)
    if name == "blobs":
        for f, w in zip(frames, want):
            m = ck.median(ck.median(f, 13), 7)
            assert np.array_equal(m, w["median"])
            e, mp = ck.canny(m, w["low"], w["high"], want_map=True)
            assert np.array_equal(mp, w["map"]) and np.array_equal(e, w["edges"])


@pytest.mark.parametrize("case", BOARD_CASES, ids=_ids(BOARD_CASES))
def test_board_edges_equal_the_plain_reference(ck, case):
    name, frames = case
    want = [fr.board_edges(f) for f in frames]
    for how, edges in _both_ways(ck.board_edges, frames, _other_size(ck)):
        edges = _np(edges)
        for j, w in enumerate(want):
            assert np.array_equal(edges[j], w["edges"]), (name, how, "frame %d: %d edge bytes differ" % (j, (edges[j] != w["edges"]).sum()))
    if name != "scene_1080p":
        assert np.array_equal(ck.median15(frames), np.stack([w["median"] for w in want]))


def test_the_median_cases_through_the_board_chain(ck):
    """the K1 cases once more with K2 behind them: whatever bounds a tile leaves -- a finished scan's, (0, 255) of a scan given
    up or of the radix descent -- no edge may be lost"""
    for name in ("hidden_up", "hidden_down", "hidden_inside", "cap", "ends", "batch3", "batch4"):
        _, k, frames, _ = next(c for c in MEDIAN_CASES if c[0] == name)
        got = ck.board_edges(frames)
        for j, f in enumerate(frames):
            assert np.array_equal(got[j], fr.board_edges(f)["edges"]), (name, j)

"""K3..K6 (k_contours.hip, k_board_lines) on the GPU against the plain references of tests/board_ref.py, which share no
code with the oracle: the ghost, status and n_contours bit for bit, the line list bit for bit and in order, biggest_area
exact on axis-aligned outlines (float32 calipers are exact there) and within 1e-5 relative elsewhere.

* Slab geometry: every small-path slab height rb from 1 to 10 on thin maps, 1280x720 (rb 7) and 1024x768 (rb 8), and
  33-frame calls with rb 7 and 8 on the 1024-thread path.  The maps are searched so that the reference accumulator
  has a peak on a slab's first and last row, equal counts across a slab boundary, a peak at theta 0 or 179, a peak at
  negative rho, and a peak in the partial last slab where rb does not divide 180.  (rho indices 0 and numrho - 1 are
  out of reach: |rho| is at most the image diagonal, below w + h.)
* Selection on edge maps: equal areas, the gate at exactly h*w/3 and one above, zero-area strokes and single pixels,
  nesting, strokes split by the cleared frame, 17 and 18 diagonal decoys whose bounding boxes beat the winner.
* Every labelling form, each on a map that yields lines.
* The single-counter gather: 128 frames of 2^24 pixels in all, one of them a zigzag component with more hull candidates
  than its segment of the gather buffer holds, in both labelling forms.
* Capacity: ghosts with more points than the first point list holds (combs, a striped frame through K1+K2), alone and
  in batches; the top-level contour cap min(h*w/4 + 1, 131072) still raises CkError."""
import numpy as np
import pytest

from tests import board_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _check(out, ghost, ref, what="", exact_area=False):
    """one frame of Context.board_lines against board_ref.board_lines (ghost None: not compared)"""
    assert out["n_contours"] == ref["n_contours"], what
    assert out["status"] == ref["status"], what
    if ref["status"] == R.NO_CONTOUR:
        return
    if exact_area:
        assert out["biggest_area"] == ref["biggest_area"], what
    else:
        assert abs(out["biggest_area"] - ref["biggest_area"]) <= 1e-5 * max(1.0, ref["biggest_area"]), what
    if ghost is not None:
        assert np.array_equal(_host(ghost), ref["ghost"]), "%s: ghost differs at %d pixels" % (
            what, int((_host(ghost) != ref["ghost"]).sum()))
    assert out["n_lines"] == len(ref["lines"]), what
    assert np.array_equal(out["lines"], ref["lines"][:len(out["lines"])]), what


def _run(ck, maps, refs, thr, what, cap=4096, exact_area=False):
    out, ghost = ck.board_lines(np.stack(maps), hough_thresh=thr, cap=cap, want_ghost=True)
    for k, ref in enumerate(refs):
        _check(out[k], ghost[k], ref, "%s frame %d" % (what, k), exact_area)
    return out


# ---------------------------------------------------------------- slab geometry
THIN = [(1, 64, 18432 // (k + 2) - 66) for k in range(1, 11)]          # small-path rb = k (board_ref.hough_slab)
SLAB_SHAPES = THIN + [(1, 720, 1280), (1, 768, 1024), (33, 64, 3934), (33, 64, 3434)]


def _searched_maps(h, w, rb, thr, tries=80):
    """slab maps kept while each adds a situation the others lack; -> (maps, refs, classes hit)"""
    need = ["first_row", "last_row", "tie_across", "theta_0_179", "rho_negative"]
    if R.NUMANGLE % rb:
        need.append("partial_slab")
    rng = np.random.default_rng(h * 100003 + w)
    maps, refs, got = [], [], set()
    for _ in range(tries):
        e = R.slab_map(rng, h, w)
        ref = R.board_lines(e, thr)
        if ref["status"] != R.LINES or ref["close"]:
            continue
        hit = R.slab_classes(R.hough_accum(ref["ghost"]), thr, rb)
        new = {k for k in need if hit[k]} - got
        if new:
            got |= new
            maps.append(e)
            refs.append(ref)
        if got >= set(need):
            break
    return maps, refs, got, need


@pytest.mark.parametrize("n, h, w", SLAB_SHAPES)
def test_slab_geometry(ck, n, h, w):
    thr = 12 if h < 100 else 30
    rb0, _ = R.hough_slab(n, h, w)
    maps, refs, got, need = _searched_maps(h, w, rb0, thr)
    assert set(need) <= got, "(%d x %d) classes never hit: %s" % (h, w, sorted(set(need) - got))
    reps = max(1, -(-n // len(maps)))
    maps, refs = (maps * reps)[:max(n, len(maps))], (refs * reps)[:max(n, len(maps))]
    rb, threads = R.hough_slab(len(maps), h, w)
    assert rb == rb0
    print("%d x %d, %d frames: rb %d, %d threads, %d workgroups per frame, last slab %d rows"
          % (h, w, len(maps), rb, threads, -(-R.NUMANGLE // rb), R.NUMANGLE - (-(-R.NUMANGLE // rb) - 1) * rb))
    _run(ck, maps, refs, thr, "%dx%d" % (h, w))


# ---------------------------------------------------------------- selection
def test_equal_areas(ck):
    """four combs of area 7744 exactly: cv2 keeps the three raster-first ones"""
    e = R.equal_combs()
    ref = R.board_lines(e, 40)
    assert ref["areas"] == [7744.0] * 4
    _run(ck, [e, e[:, ::-1].copy(), e[::-1].copy()], [ref, R.board_lines(e[:, ::-1], 40), R.board_lines(e[::-1], 40)],
         40, "equal combs", exact_area=True)


def test_gate(ck):
    h, w = R.GATE_HW
    lo, hi = R.gate_map(False), R.gate_map(True)
    rlo, rhi = R.board_lines(lo, 8), R.board_lines(hi, 8)
    assert rlo["status"] == R.TOO_SMALL and rlo["biggest_area"] == h * w / 3
    assert rhi["status"] == R.LINES and rhi["biggest_area"] == h * w / 3 + 1
    out = _run(ck, [lo, hi, lo], [rlo, rhi, rlo], 8, "gate", exact_area=True)
    assert out[0]["biggest_area"] == 560.0 and out[0]["n_lines"] == 0


def _zero_area_maps():
    """strokes (horizontal, vertical, 45 degrees) and single pixels only: TOO_SMALL with biggest_area 0; then the
    same beside an outline: the top three take the two raster-first zero-area contours"""
    e = np.zeros((60, 90), np.uint8)
    e[5, 5:60] = 255
    e[10:50, 70] = 255
    R.draw_line(e, 10, 15, 40, 45)
    e[30, 60] = e[55, 8] = e[2, 80] = 255
    f = e.copy()
    R.outline(f, 12, 45, 56, 86)
    f[30, 60] = 0
    return [e, f]


def _nest_and_frame_maps():
    e = np.zeros((60, 90), np.uint8)
    R.outline(e, 4, 4, 55, 85)
    R.outline(e, 10, 10, 40, 60)                              # nested: not top-level, nor what it holds
    e[20, 20:40] = 255
    s = np.zeros((60, 90), np.uint8)
    s[0:60, 30] = s[59, 10:80] = s[0, 50:89] = 255             # strokes through the frame rows and columns
    s[30, 0:89] = 255
    s[40:60, 70] = s[40, 60:80] = 255
    R.outline(s, 45, 5, 55, 25)
    t = np.zeros((60, 90), np.uint8)                          # thick strokes: pixels that meet S0 only diagonally
    t[5:50, 5:9] = 255
    t[45:50, 5:80] = 255
    t[10:20, 30:60] = 255
    t[12:18, 35:55] = 0
    return [e, s, t]


def test_zero_area_nesting_frame_split(ck):
    for maps in (_zero_area_maps(), _nest_and_frame_maps()):
        refs = [R.board_lines(e, 10) for e in maps]
        _run(ck, maps, refs, 10, "selection maps")
    refs = [R.board_lines(e, 10) for e in _zero_area_maps()]
    assert refs[0]["status"] == R.TOO_SMALL and refs[0]["biggest_area"] == 0.0 and refs[0]["n_contours"] == 6
    assert refs[1]["status"] == R.LINES and sorted(refs[1]["areas"])[-3:-1] == [0.0, 0.0]


@pytest.mark.parametrize("k", [17, 18])
def test_diagonal_decoys(ck, k):
    """the 16 largest bounding boxes are all strokes of area 0: the second round of exact areas must find the outline"""
    e = R.decoy_map(k)
    ref = R.board_lines(e, 20)
    assert ref["status"] == R.LINES and ref["n_contours"] == k + 1 and ref["biggest_area"] == 8075.0
    _run(ck, [e, e[:, ::-1].copy()], [ref, R.board_lines(e[:, ::-1], 20)], 20, "decoys", exact_area=True)


# ---------------------------------------------------------------- labelling forms
@pytest.mark.parametrize("w, form", [(1000, "runs, w <= 1024"), (2000, "runs, w <= 2048"), (4000, "runs, w <= 4096"),
                                     (1002, "dense, w % 4 != 0"), (4200, "dense, w > 4096")])
def test_ccl_forms(ck, w, form):
    rng = np.random.default_rng(w)
    maps = [R.slab_map(rng, 64, w) for _ in range(3)]
    refs = [R.board_lines(e, 12) for e in maps]
    assert all(r["status"] == R.LINES and len(r["lines"]) for r in refs)
    _run(ck, maps, refs, 12, form)


def test_ccl_unaligned_device_pointer(ck):
    import torch
    rng = np.random.default_rng(77)
    maps = np.stack([R.slab_map(rng, 64, 1000) for _ in range(2)])
    buf = torch.zeros(maps.size + 1, dtype=torch.uint8, device="cuda:0")
    buf[1:] = torch.from_numpy(maps.ravel()).to("cuda:0")
    dev = buf[1:].view(maps.shape)
    assert dev.data_ptr() % 4 == 1
    out, ghost = ck.board_lines(dev, hough_thresh=12, want_ghost=True)
    for k in range(len(maps)):
        ref = R.board_lines(maps[k], 12)
        assert ref["status"] == R.LINES and len(ref["lines"])
        _check(out[k], ghost[k], ref, "unaligned frame %d" % k)


def test_ccl_denser_than_the_run_nodes(ck):
    rng = np.random.default_rng(4711)
    dense = (rng.random((280, 400)) < 0.7).astype(np.uint8) * 255
    sparse = R.slab_map(rng, 280, 400)
    refs = [R.board_lines(e, 30) for e in (sparse, dense)]
    assert refs[0]["status"] == R.LINES and len(refs[0]["lines"])
    ck.timing_enable(True)
    try:
        ck.timing_reset()
        _run(ck, [sparse, dense], refs, 30, "dense fallback")
        assert ck.timing_get("ccl")[1] == 2
    finally:
        ck.timing_enable(False)


@pytest.mark.parametrize("w, form", [(512, "runs"), (510, "dense")])
def test_gather_segment_overflow(ck, w, form):
    """n * h * w >= 2^22 gives every frame a segment of 2^22 // n hull candidates; the zigzag frame has more, so the round
    is gathered again through one counter for all frames: contour_gather runs twice for the one round there is"""
    n, h, thr = 128, 256, 100
    z, sq = R.zigzag(h, w), R.outline(np.zeros((h, w), np.uint8), 10, 10, 30, 40)
    cz, cs = int(R.hull_candidates(z).sum()), int(R.hull_candidates(sq).sum())
    print("%s: %d candidates in the zigzag frame, segment %d, %d edge pixels" % (form, cz, 2 ** 22 // n, int((z > 0).sum())))
    assert n * h * w >= 2 ** 22 and cz > 2 ** 22 // n
    if form == "runs":
        assert int((z > 0).sum()) <= 65536                    # the run nodes fit: the call stays in the run-table form
    assert cz + (n - 1) * cs < 2 ** 22
    rz, rs = R.board_lines(z, thr), R.board_lines(sq, thr)
    assert rz["status"] == R.LINES and rz["n_contours"] == 1 and rs["n_contours"] == 1
    assert int((rz["ghost"] > 0).sum()) < max(h * w // 8, 1 << 16)
    maps, refs = [sq] * 5 + [z] + [sq] * (n - 6), [rs] * 5 + [rz] + [rs] * (n - 6)
    ck.timing_enable(True)
    try:
        ck.timing_reset()
        _run(ck, maps, refs, thr, "zigzag, " + form, cap=16384)
        assert ck.timing_get("contour_gather")[1] == 2
        assert ck.timing_get("ccl")[1] == 1                   # the form the width selects, no dense redo
    finally:
        ck.timing_enable(False)


# ---------------------------------------------------------------- capacity
_COMBS = {(480, 640): (2, 96), (1080, 1920): (4, 400)}       # tooth step, Hough threshold (peaks under PEAK_CAP)


@pytest.mark.parametrize("h, w", list(_COMBS))
def test_comb_ghost_beyond_the_point_list(ck, h, w):
    """the whole comb is outer border: more ghost points than max(h*w/8, 65536); the call sizes the list again and
    equals the reference, alone and in a batch of 8 with ordinary maps"""
    step, thr = _COMBS[(h, w)]
    e = R.comb(h, w, step)
    ref = R.board_lines(e, thr)
    pcap = max(h * w // 8, 1 << 16)
    assert int((ref["ghost"] > 0).sum()) > pcap and ref["status"] == R.LINES
    ck.timing_enable(True)
    try:
        ck.timing_reset()
        _run(ck, [e], [ref], thr, "comb", cap=16384)
        assert ck.timing_get("ghost")[1] == 2 and ck.timing_get("hough_vote")[1] == 2
        rng = np.random.default_rng(h)
        others = [R.slab_map(rng, h, w) for _ in range(7)]
        orefs = [R.board_lines(m, thr) for m in others]
        maps, refs = others[:3] + [e] + others[3:], orefs[:3] + [ref] + orefs[3:]
        ck.timing_reset()
        _run(ck, maps, refs, thr, "comb in a batch", cap=16384)
        assert ck.timing_get("ghost")[1] == 2
        ck.timing_reset()
        _run(ck, others, orefs, thr, "ordinary batch", cap=16384)
        assert ck.timing_get("ghost")[1] == 1                 # no overflow: one pass
    finally:
        ck.timing_enable(False)


def test_striped_frame_through_board_detect(ck, ora):
    """7-px vertical stripes joined by one band survive K1+K2 as a comb of edges: at 1080p the ghost holds more points
    than h*w/8"""
    h, w = 1080, 1920
    fr = np.full((h, w, 3), 200, np.uint8)
    for x0 in range(8, w - 8, 14):
        fr[8:h - 8, x0:x0 + 7] = 40
    fr[h // 2:h // 2 + 20, 8:w - 8] = 40
    e = ora.canny(ora.median(fr, 15), 25, 75)
    assert np.array_equal(_host(ck.board_edges(fr)), e)
    ref = R.board_lines(e)
    assert int((ref["ghost"] > 0).sum()) > h * w // 8 and ref["status"] == R.LINES
    out = ck.board_detect(np.stack([fr, fr[:, ::-1].copy()]), cap=16384)
    _check(out[0], None, ref, "striped frame")
    assert out[1]["n_lines"] > 0


def test_top_level_contour_cap(ck):
    """isolated dots on a 2-px lattice at 1080p: 518 400 top-level contours, more than min(h*w/4 + 1, 131072)"""
    from camkifu_amd import capi
    e = R.dot_lattice(1080, 1920)
    with pytest.raises(capi.CkError, match=r"error 3: .*more than 131072 external contours"):
        ck.board_lines(e)
    ok = R.slab_map(np.random.default_rng(3), 64, 1000)           # the context stays usable
    _run(ck, [ok], [R.board_lines(ok, 12)], 12, "after the cap")

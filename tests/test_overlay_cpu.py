"""Overlays without a GPU: display lists and their packing, the limits ck_overlay_plan enforces, the plan's coverage
against the reference painter, the font, and the lists the reference's drawing names build (against a stub context)."""
import json
import os

import numpy as np
import pytest

from . import overlay_cases as cases
from . import overlay_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (17, 33), (35, 69)]


@pytest.fixture(scope="module")
def capi():
    from camkifu_amd import capi
    capi.build()
    return capi


@pytest.fixture(scope="module")
def glyphs(capi):
    return np.stack([capi.overlay_glyph(ch) for ch in range(32, 127)])


# ---- DisplayList ------------------------------------------------------------------------------------------------------
def test_pack_round_trips():
    from camkifu_amd.core import overlay
    a = overlay.DisplayList().segment(1, 2, -3, 4, (1, 2, 3), thickness=3).text(5, 6, "Frame 1/2", 255, scale=2)
    a.circle(7, 8, 5, (255, 255, 0)).disc(9, 10, 6, 0, alpha=96).rect(4, 3, 2, 1, (0, 0, 255), thickness=0).text(0, 0, b"\x1f\xc8")
    b = overlay.DisplayList()
    c = overlay.DisplayList().extend(a).text(1, 1, "second")
    prims, start, text = overlay.pack([a, b, c])
    assert prims.dtype == np.int32 and prims.shape == (13, 8) and start.tolist() == [0, 6, 6, 13]
    assert text == b"Frame 1/2\x1f\xc8Frame 1/2\x1f\xc8second"
    assert prims[0].tolist() == [overlay.SEGMENT, 1, 2, -3, 4, 3, cases.col(1, 2, 3), 0]
    assert prims[1].tolist() == [overlay.TEXT, 5, 6, 9, 0, 2, cases.col(255, 255, 255), 0]
    assert prims[2].tolist() == [overlay.CIRCLE, 7, 8, 1, 0, 5, cases.col(255, 255, 0), 0]
    assert prims[3].tolist() == [overlay.DISC, 9, 10, 0, 0, 6, cases.col(0, 0, 0, 96), 0]
    assert prims[4].tolist() == [overlay.RECT, 4, 3, 2, 1, 0, cases.col(0, 0, 255), 0]
    assert prims[5].tolist() == [overlay.TEXT, 0, 0, 2, 0, 1, cases.col(255, 255, 255), 9] and prims[12, 7] == 22
    back = overlay.unpack(prims, start, text)
    assert [d.prims for d in back] == [a.prims, b.prims, c.prims]
    assert overlay.colour_code((300.7, -2, 127.9)) == cases.col(255, 0, 127) & 0xffffffff      # truncated, clamped
    assert (overlay.SEGMENT, overlay.CIRCLE, overlay.DISC, overlay.RECT, overlay.TEXT) == (
        ref.SEGMENT, ref.CIRCLE, ref.DISC, ref.RECT, ref.TEXT)


# ---- limits -----------------------------------------------------------------------------------------------------------
OPAQUE = cases.col(1, 2, 3)
REFUSED = {
    "unknown kind 0": [(0, 0, 0, 0, 0, 1, OPAQUE, 0)],
    "unknown kind 6": [(6, 0, 0, 0, 0, 1, OPAQUE, 0)],
    "x0 too far": [cases.seg(32768, 0, 0, 0)],
    "y0 too far": [cases.disc(0, -32768, 1)],
    "x1 too far": [cases.seg(0, 0, -32768, 0)],
    "y1 too far": [cases.rect(0, 0, 0, 32768)],
    "even thickness": [cases.seg(0, 0, 5, 5, 2)],
    "thickness 17": [cases.seg(0, 0, 5, 5, 17)],
    "thickness 0": [cases.seg(0, 0, 5, 5, 0)],
    "ring thickness 4": [cases.circle(3, 3, 5, 4)],
    "ring thickness 17": [cases.circle(3, 3, 5, 17)],
    "radius -1": [cases.disc(3, 3, -1)],
    "radius 4096": [cases.circle(3, 3, 4096)],
    "scale 0": [(ref.TEXT, 0, 0, 0, 0, 0, OPAQUE, 0)],
    "scale 9": [(ref.TEXT, 0, 0, 0, 0, 9, OPAQUE, 0)],
    "text past the end": [(ref.TEXT, 0, 0, 3, 0, 1, OPAQUE, 2)],
    "text offset negative": [(ref.TEXT, 0, 0, 1, 0, 1, OPAQUE, -1)],
    "text length negative": [(ref.TEXT, 0, 0, -1, 0, 1, OPAQUE, 0)],
    "text offset huge": [(ref.TEXT, 0, 0, 2, 0, 1, OPAQUE, 2 ** 31 - 1)],
    "alpha 0": [cases.seg(0, 0, 5, 5, 1, cases.col(9, 9, 9, 0))],
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_plan_refuses(capi, why):
    prims = np.array([cases.seg(0, 0, 3, 3)] + REFUSED[why], np.int32)
    with pytest.raises(capi.CkError) as e:
        capi.overlay_plan(1, 20, 20, prims, [0, 2], text_len=4)
    assert e.value.code == capi.CK_ERR_ARG
    capi.overlay_plan(1, 20, 20, prims[:1], [0, 1], text_len=4)                      # the rest of the list is fine
    capi.overlay_plan(2, 20, 20, prims, [0, 1, 1], text_len=4)                       # and so is a list nobody owns


def test_plan_refuses_frame_starts_and_accepts_the_limits(capi):
    ok = np.array([cases.seg(-32767, 32767, 32767, -32767, 15), cases.circle(0, 0, 4095, 15), cases.disc(0, 0, 0),
                   (ref.TEXT, 0, 0, 4, 0, 8, OPAQUE, 0), (ref.TEXT, 0, 0, 0, 0, 1, OPAQUE, 4), cases.rect(5, 5, 1, 1, 0)], np.int32)
    capi.overlay_plan(1, 20, 20, ok, [0, 6], text_len=4)
    for start in ([0, 2, 1], [1, 2, 3], [0, -1, 2], [-1, 0, 1]):
        with pytest.raises(capi.CkError) as e:
            capi.overlay_plan(2, 20, 20, ok, start, text_len=4)
        assert e.value.code == capi.CK_ERR_ARG, start
    bin_size, bin_start, bin_prims = capi.overlay_plan(0, 0, 0, np.zeros((0, 8), np.int32), [0])
    assert bin_size > 0 and bin_start.tolist() == [0] and len(bin_prims) == 0
    bin_size, bin_start, bin_prims = capi.overlay_plan(2, 20, 20, np.zeros((0, 8), np.int32), [0, 0, 0])
    assert len(bin_start) == 2 * (-(-20 // bin_size)) ** 2 + 1 and not bin_start.any() and len(bin_prims) == 0


def test_cap_too_small_reports_the_size_needed(capi):
    import ctypes as C
    name, prims, text = [c for c in cases.cases(35, 69) if c[0] == "thick"][0]
    start = cases.as_batch(prims)
    bin_size, bin_start, bin_prims = capi.overlay_plan(1, 35, 69, prims, start, len(text))
    need = len(bin_prims)
    assert need > len(prims)
    L = capi.lib()
    for cap in (0, need - 1):
        bs, refs = C.c_int32(0), C.c_int32(0)
        starts, out = np.full(len(bin_start), -7, np.int32), np.full(need, -7, np.int32)
        rc = L.ck_overlay_plan(1, 35, 69, prims.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p), len(text), C.byref(bs),
                               starts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cap, C.byref(refs))
        assert rc == capi.CK_ERR_CAPACITY and refs.value == need and bs.value == bin_size
        assert (out == -7).all() and np.array_equal(starts, bin_start)


# ---- the plan never loses coverage --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_plan_covers_every_pixel_the_reference_paints(capi, glyphs, shape):
    h, w = shape
    for name, prims, text in cases.cases(h, w):
        bin_size, bin_start, bin_prims = capi.overlay_plan(1, h, w, prims, cases.as_batch(prims), len(text))
        nbx = -(-w // bin_size)
        assert len(bin_start) == nbx * -(-h // bin_size) + 1 and bin_start[0] == 0 and bin_start[-1] == len(bin_prims)
        lists = [bin_prims[bin_start[b]:bin_start[b + 1]].tolist() for b in range(len(bin_start) - 1)]
        for got in lists:
            assert got == sorted(set(got)), name                                 # list order, nothing twice
        for i, prim in enumerate(prims):
            for x, y in ref.pixels_of(prim, h, w, text, glyphs):
                assert i in lists[(y // bin_size) * nbx + x // bin_size], (name, i, x, y)


def test_plan_of_a_batch_keeps_the_frames_apart(capi):
    prims, start, text = cases.batch(35, 69)
    bin_size, bin_start, bin_prims = capi.overlay_plan(3, 35, 69, prims, start, len(text))
    per = (len(bin_start) - 1) // 3
    for f in range(3):
        mine = bin_prims[bin_start[f * per]:bin_start[(f + 1) * per]]
        assert ((mine >= start[f]) & (mine < start[f + 1])).all()
    assert bin_start[per] == bin_start[2 * per] and bin_start[per] > 0 and bin_start[-1] > bin_start[2 * per]


# ---- the font -----------------------------------------------------------------------------------------------------------
def test_font(capi, glyphs):
    assert glyphs.shape == (95, 7) and not glyphs[0].any()
    assert (glyphs < 32).all()                                                       # five columns
    seen = {}
    for ch in range(33, 127):
        rows = glyphs[ch - 32]
        assert rows.any(), chr(ch)
        assert seen.setdefault(rows.tobytes(), ch) == ch, "%r looks like %r" % (chr(ch), chr(seen[rows.tobytes()]))
    for ch in (0, 31, 127, 200, 255, -1, 1000):
        assert np.array_equal(capi.overlay_glyph(ch), glyphs[ord("?") - 32])
    with open(os.path.join(ROOT, "tests", "golden", "font5x7.json")) as f:
        golden = json.load(f)
    assert golden["first"] == 32 and np.array_equal(np.array(golden["rows"], np.uint8), glyphs)
    header = open(os.path.join(ROOT, "camkifu_amd", "csrc", "ck_font5x7.h")).read()
    assert header.count("{0x") == 95


# ---- the reference's drawing names against a stub context ----------------------------------------------------------------
class StubCtx:
    """records what overlay_draw is asked to draw, and draws nothing"""

    def __init__(self):
        self.calls = []

    def overlay_draw(self, images, lists):
        self.calls.append((images, lists))
        return images


@pytest.fixture()
def stub(monkeypatch):
    from camkifu_amd import capi
    ctx = StubCtx()
    monkeypatch.setattr(capi, "get_context", lambda device=0: ctx)
    return ctx


def _only(stub):
    assert len(stub.calls) == 1                                                     # ONE library call, never one per stone
    return stub.calls[0]


def test_draw_lines_builds_one_list(stub):
    from camkifu_amd.core import imgutil, overlay
    img = np.zeros((48, 64, 3), np.uint8)
    imgutil.draw_lines(img, [(1, 2, 3, 4), ((5, 6), (7, 8))], color=(0, 0, 255))
    got_img, dl = _only(stub)
    assert got_img is img
    assert dl.prims == overlay.DisplayList().segment(1, 2, 3, 4, (0, 0, 255)).segment(5, 6, 7, 8, (0, 0, 255)).prims
    with pytest.raises(ValueError):
        imgutil.draw_lines(img, [(1, 2, 3)])
    # an image larger than the screen is shown pyrDown-ed f times: the lines are drawn 1 + 2 f thick
    stub.calls.clear()
    big = np.zeros((3000, 4000), np.uint8)
    imgutil.draw_lines(big, [(0, 0, 9, 9)])
    assert _only(stub)[1].prims[0][5] == 1 + 2 * imgutil._factor(big) and imgutil._factor(big) >= 1 and imgutil._factor(img) == 0


def test_draw_str_builds_shadow_then_text(stub):
    from camkifu_amd.core import imgutil, overlay
    img = np.zeros((48, 64, 3), np.uint8)
    imgutil.draw_str(img, "abc", 10, 20, color=(1, 2, 3))
    want = overlay.DisplayList().text(11, 14, "abc", (0, 0, 0)).text(10, 13, "abc", (1, 2, 3))       # top = baseline - 7
    assert _only(stub)[1].prims == want.prims
    stub.calls.clear()
    imgutil.draw_str(img, "hello!")                                                   # the reference's centring defaults
    x, y = int(64 / 2 - 6 * 3.5), int(48 / 2 - 3)
    assert _only(stub)[1].prims == overlay.DisplayList().text(x + 1, y - 6, "hello!", (0, 0, 0)).text(x, y - 7, "hello!", (255, 255, 255)).prims


def test_goban_corners_paint(stub):
    from camkifu_amd.board.boardfinder import GobanCorners
    from camkifu_amd.core import overlay
    img = np.zeros((480, 640, 3), np.uint8)
    few = GobanCorners([(10, 20), (300, 30)])
    few.paint(img)
    assert _only(stub)[1].prims == overlay.DisplayList().circle(10, 20, 5, (255, 255, 0)).circle(300, 30, 5, (255, 255, 0)).prims
    stub.calls.clear()
    quad = GobanCorners([(100, 100), (400, 110), (420, 380), (90, 400)])
    assert quad.hull is not None
    quad.paint(img)
    prims = _only(stub)[1].prims
    assert [p[0] for p in prims] == [overlay.CIRCLE] * 4 + [overlay.SEGMENT] * 4
    hull = [tuple(p) for p in quad.hull]
    # reference board/boardfinder.py:128-134: edges hull[i] -> hull[i + 1] for i = -1 .. 2, red first, then the ramp
    ramp = [(0, 0, 255), (255, 0, 0), (255 * 2 / 3, 0, 255 * 1 / 3), (255 * 1 / 3, 0, 255 * 2 / 3)]
    for k, i in enumerate(range(-1, 3)):
        assert prims[4 + k] == overlay.DisplayList().segment(*hull[i], *hull[i + 1], ramp[k]).prims[0]
    assert prims[6][6] == overlay.colour_code((170, 0, 85)) and prims[7][6] == overlay.colour_code((85, 0, 170))


class _Capt:
    def __init__(self, pos, total):
        self.pos, self.total = pos, total

    def get(self, prop):
        from camkifu_amd.core import capture
        return {capture.CAP_PROP_POS_FRAMES: self.pos, capture.CAP_PROP_FRAME_COUNT: self.total}[prop]


class _Manager:
    def __init__(self, queue=None):
        self.imqueue, self.capt, self.controller = queue, _Capt(12, 345), None
        self.device = 0


def test_draw_metadata_and_show(stub, monkeypatch):
    import queue
    from camkifu_amd import cvconf
    from camkifu_amd.core import overlay, video
    q = queue.Queue()
    vp = video.VidProcessor(_Manager(q))
    img = np.zeros((100, 200, 3), np.uint8)
    # the default: the image object goes to the queue untouched, the metadata is thrown away, nothing is drawn
    assert cvconf.annotate is False
    vp.metadata["a: {}"].append(3)
    vp._show(img, name="win")
    name, shown, who, loc = q.get_nowait()
    assert shown is img and name == "win" and who is vp and not stub.calls and not vp.metadata and not img.any()
    # reference core/video.py:243-265: x offset 40, 20 pixels per line, defaults from the top, custom lines from the bottom
    vp.metadata["stones: {}"].append(7)
    vp.metadata["k = {}"] = "v"
    vp._draw_metadata(img, "win", frame=True, latency=False, thread=True)
    import threading
    lines = [("Frame 12/345 (0 not shown)", 20), ("thread: " + threading.current_thread().name, 40),
             ("stones: [7]", 100 - 20), ("k = v", 100 - 40)]
    want = overlay.DisplayList()
    for s, y in lines:
        want.text(41, y - 6, s, (0, 0, 0)).text(40, y - 7, s, (255, 255, 255))
    assert _only(stub)[1].prims == want.prims and not vp.metadata
    stub.calls.clear()
    monkeypatch.setattr(cvconf, "annotate", True)
    vp._shown_at.clear()
    vp.metadata["m {}"] = 1
    vp._show(img, name="win")
    assert q.get_nowait()[1] is img
    texts = [p[7] for p in _only(stub)[1].prims]
    assert texts[0] == b"Frame 12/345 (0 not shown)" and texts[2].startswith(b"latency: ") and texts[-1] == b"m 1" and len(texts) == 6


def test_draw_stones_and_grid(stub):
    from camkifu_amd.core import overlay
    from camkifu_amd.golib_shim import B, E, W, gsize
    from camkifu_amd.stone.stonesfinder import PosGrid, StonesFinder
    sf = StonesFinder.__new__(StonesFinder)
    sf._posgrid = PosGrid(380)
    stones = np.full((gsize, gsize), E, dtype=object)
    stones[3, 15], stones[0, 0] = B, W
    canvas = sf.draw_stones(stones)
    assert canvas.shape == (380, 380, 3) and (canvas == (65, 100, 128)).all()         # the brown canvas, nothing drawn by the stub
    got_img, dl = _only(stub)
    assert got_img is canvas and len(dl) == 2 + 361
    mtx = sf._posgrid.mtx
    # reference stone/stonesfinder.py:826-836: discs of radius 10 at (p[1], p[0]), row-major, then the grid's circles
    assert dl.prims[0] == overlay.DisplayList().disc(int(mtx[0, 0, 1]), int(mtx[0, 0, 0]), 10, (255, 255, 255)).prims[0]
    assert dl.prims[1] == overlay.DisplayList().disc(int(mtx[3, 15, 1]), int(mtx[3, 15, 0]), 10, (0, 0, 0)).prims[0]
    grid = overlay.DisplayList()
    for i in range(19):
        for j in range(19):
            grid.circle(int(mtx[i, j, 1]), int(mtx[i, j, 0]), 5, (255, 255, 0))
    assert dl.prims[2:] == grid.prims
    stub.calls.clear()
    mine = np.zeros((380, 380, 3), np.uint8)
    assert sf.draw_stones(stones, mine) is mine and _only(stub)[0] is mine
    stub.calls.clear()
    sf._drawgrid(mine)
    assert _only(stub)[1].prims == grid.prims
    assert StonesFinder.get_display_color(0, 0) == (40, 10, 200) and StonesFinder.get_display_color(1, 1) == (80, 115, 5)


def test_drawvalues_and_intersections(stub):
    from camkifu_amd.core import overlay
    from camkifu_amd.stone.stonesfinder import PosGrid, StonesFinder
    sf = StonesFinder.__new__(StonesFinder)
    sf._posgrid = PosGrid(380)
    mtx = sf._posgrid.mtx
    values = np.full((19, 19), None, dtype=object)
    values[2, 5], values[18, 18] = 7, "ab"
    img = np.zeros((380, 380, 3), np.uint8)
    sf._drawvalues(img, values)
    want = overlay.DisplayList()
    for (r, c), s in (((2, 5), "7"), ((18, 18), "ab")):
        x, y = int(mtx[r, c, 0]) - 10, int(mtx[r, c, 1]) + 2                           # reference :803-806, as written there
        want.text(x + 1, y - 6, s, (0, 0, 0)).text(x, y - 7, s, (255, 255, 255))
    assert _only(stub)[1].prims == want.prims
    stub.calls.clear()
    shown = []
    sf._show = lambda im, name=None, **kw: shown.append((im, name))
    sf._window_name = lambda: "T"
    grid = -mtx.astype(np.int32)
    grid[4, 4] += (1, 0)                                                               # one intersection was updated
    sf.display_intersections(grid, img)
    prims = _only(stub)[1].prims
    assert len(prims) == 361 + 1 and shown == [(img, "T - Intersections")]
    k = 4 * 19 + 4
    # reference :856-859: thickness 6 is even; the odd 7 keeps radius 5 in the middle of the band
    assert prims[k] == overlay.DisplayList().circle(int(-grid[4, 4, 1]), int(-grid[4, 4, 0]), 5, (0, 0, 0), thickness=7).prims[0]
    assert prims[k + 1] == overlay.DisplayList().circle(int(-grid[4, 4, 1]), int(-grid[4, 4, 0]), 5, (40, 10, 200), thickness=3).prims[0]
    assert prims[0] == overlay.DisplayList().circle(int(mtx[0, 0, 1]), int(mtx[0, 0, 0]), 5, (40, 10, 200), thickness=3).prims[0]


def test_sf_neural_target_rectangles():
    from camkifu_amd.core import overlay
    from camkifu_amd.stone import sf_neural
    from camkifu_amd.stone.stonesfinder import PosGrid

    class _Policy:
        def state(self):
            t, hc = np.zeros((19, 19), np.uint8), np.zeros((19, 19), np.uint8)
            t[2, 3], t[2, 4], t[10, 10], t[11, 11] = 5, 40, 16, 200
            hc[2, 4] = 1                                                            # under watch: mark_targets skips it
            return dict(targets=t, heat_color=hc)

    sf = sf_neural.SfNeural.__new__(sf_neural.SfNeural)
    sf.policy, sf._posgrid, sf.manager = _Policy(), PosGrid(380), sf_neural.nm.NNManager()
    counts = np.zeros((19, 19), np.int32)
    counts[10, 11] = 201                                                           # more than half of a 20 x 20 zone
    got = sf.targets_list(counts).prims
    z = sf._posgrid.zones()
    want = overlay.DisplayList()
    for (r, c), red in (((2, 3), 63), ((10, 10), 204), ((11, 11), 255)):            # min(255, t / 5 * 255 // 4)
        x0, y0, x1, y1 = (int(v) for v in z[r, c])
        want.rect(y0, x0, y1, x1, (0, 0, red))
    assert got[:3] == want.prims
    regions = [(i, j) for i in range(sf.manager.split) for j in range(sf.manager.split)
               if (_Policy().state()["targets"][slice(*sf.manager._subregion(i, j)[:2]), slice(*sf.manager._subregion(i, j)[2:])] > 15).any()]
    assert len(got) == 3 + len(regions) and len(regions) >= 2
    for k, (i, j) in enumerate(regions):
        rs, re, cs, ce = sf.manager._subregion(i, j)
        x0, x1, y0, y1 = sf.manager._get_rect_nn(rs, re, cs, ce)
        busy = rs <= 10 < re and cs <= 11 < ce
        assert got[3 + k] == overlay.DisplayList().rect(y0, x0, y1, x1, (255, 0, 0) if busy else (0, 255, 0)).prims[0]
    assert any(p[6] == overlay.colour_code((255, 0, 0)) for p in got[3:]) and any(p[6] == overlay.colour_code((0, 255, 0)) for p in got[3:])


def test_annotation_lists():
    """what tools/transcode.py --annotate draws per frame (core/annotate.py)"""
    from camkifu_amd import capi
    from camkifu_amd.board.boardfinder import GobanCorners
    from camkifu_amd.core import annotate, overlay
    from camkifu_amd.stone.stonesfinder import PosGrid
    grid = PosGrid(380)
    codes = np.zeros((19, 19), np.uint8)
    codes[3, 15], codes[9, 9] = 1, 2
    fg = np.zeros((19, 19), np.int32)
    fg[5, 9], fg[6, 9] = 281, 280                                                   # 0.7 of a 20 x 20 zone is 280: above, and not
    dl = annotate.goban_list(codes, fg, grid, 7, 24, "B[Q16]")
    kinds = [p[0] for p in dl.prims]
    assert kinds == [overlay.CIRCLE] * 361 + [overlay.DISC, overlay.CIRCLE] * 2 + [overlay.RECT] + [overlay.TEXT] * 4
    assert dl.prims[361] == overlay.DisplayList().disc(int(grid.mtx[3, 15, 1]), int(grid.mtx[3, 15, 0]), 6, (0, 0, 0)).prims[0]
    assert dl.prims[362] == overlay.DisplayList().circle(int(grid.mtx[3, 15, 1]), int(grid.mtx[3, 15, 0]), 6, (255, 255, 255)).prims[0]
    assert dl.prims[363][6] == overlay.colour_code((255, 255, 255)) and dl.prims[364][6] == overlay.colour_code((0, 0, 0))
    x0, y0, x1, y1 = (int(v) for v in grid.zones()[5, 9])
    assert dl.prims[365] == overlay.DisplayList().rect(y0, x0, y1 - 1, x1 - 1, (0, 0, 255), thickness=0, alpha=96).prims[0]
    assert [p[7] for p in dl.prims[366:]] == [b"Frame 7/24"] * 2 + [b"B[Q16]"] * 2 and dl.prims[367][1:3] == (4, 4)
    assert dl.prims[369][2] == 380 - 4 - 8
    assert len(annotate.goban_list(codes, None, grid, 7, 24, "")) == 361 + 4 + 2                # no counts, no moves
    assert annotate.moves_text([(1, [("B", 3, 15)]), (2, [("W", 0, 0), ("", 18, 18)])]) == "B[Q16] W[A19] E[T1]"
    # full frames: before the first detection only the text, at scale 2
    early = annotate.frame_list((480, 640), GobanCorners(), None, codes, grid, 1, 24, "")
    assert [p[0] for p in early.prims] == [overlay.TEXT] * 2 and early.prims[1][5] == 2 and early.prims[1][1:3] == (8, 8)
    quad = GobanCorners([(100, 60), (500, 70), (520, 430), (90, 420)])
    mtx = capi.get_perspective_transform(np.asarray(quad.hull, np.float32), np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32))
    dl = annotate.frame_list((480, 640), quad, mtx, codes, grid, 9, 24, "W[K10]")
    kinds = [p[0] for p in dl.prims]
    assert kinds == [overlay.CIRCLE] * 4 + [overlay.SEGMENT] * 4 + [overlay.CIRCLE] * 361 + [overlay.DISC, overlay.CIRCLE] * 2 + [overlay.TEXT] * 4
    assert dl.prims[:8] == quad.display_list().prims
    centre = dl.prims[8 + 9 * 19 + 9]                                               # tengen lands inside the quadrilateral, radius 3
    assert centre[5] == 3 and 250 < centre[1] < 350 and 200 < centre[2] < 290
    corner = dl.prims[8]                                                            # the first intersection: half a cell inside the first corner
    assert abs(corner[1] - 100) < 25 and abs(corner[2] - 60) < 25
    assert dl.prims[8 + 361][1:3] == dl.prims[8 + 3 * 19 + 15][1:3] and dl.prims[8 + 361][5] >= 4

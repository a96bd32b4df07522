"""The overlay rasteriser on the GPU: every byte against the plain painter of tests/overlay_ref.py, over the lists of
tests/overlay_cases.py, on shapes with frames off a dword, partial bins and bin seams; then through the transcoder."""
import importlib.util
import os

import numpy as np
import pytest

from . import overlay_cases as cases
from . import overlay_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def glyphs():
    from camkifu_amd import capi
    return np.stack([capi.overlay_glyph(ch) for ch in range(32, 127)])


def _bin_size():
    from camkifu_amd import capi
    return capi.overlay_plan(0, 0, 0, np.zeros((0, 8), np.int32), [0])[0]


def _shapes():
    b = _bin_size()
    return [(1, 1, 3), (17, 33, 3), (17, 33, 1), (b + 3, 2 * b + 5, 3)]


def _image(n, h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, c)).astype(np.uint8)


def _draw_raw(ck, img, prims, start, text, on_device):
    """ck_overlay_draw on a copy of img (in host memory or HBM) with raw arrays -> the drawn images as numpy"""
    import ctypes as C
    import torch
    from camkifu_amd import capi
    n, h, w, c = img.shape
    prims = np.ascontiguousarray(prims, np.int32)
    start = np.ascontiguousarray(start, np.int32)
    if on_device:
        t = torch.from_numpy(img.copy()).to("cuda:0")
        p, sp, keep = ck._in(t)
    else:
        t = img.copy()
        p, sp = t.ctypes.data_as(C.c_void_p), capi.CK_HOST
    ck._chk(capi.lib().ck_overlay_draw(ck._h, p, n, h, w, c, sp, prims.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p),
                                       C.c_char_p(text), len(text)))
    return t.cpu().numpy() if on_device else t


@pytest.mark.parametrize("k", range(4), ids=["1x1x3", "17x33x3", "17x33x1", "seams"])
def test_every_case_equals_the_reference(ck, glyphs, k):
    """host memory and HBM in turn, one context throughout (so it is reused after calls at other sizes); pixels nothing
    covers keep the random input's bytes"""
    h, w, c = _shapes()[k]
    for j, (name, prims, text) in enumerate(cases.cases(h, w, _bin_size())):
        img = _image(1, h, w, c, seed=j)
        want, covered = ref.paint(img, prims, [0, len(prims)], text, glyphs)
        got = _draw_raw(ck, img, prims, cases.as_batch(prims), text, on_device=bool((j + k) & 1))
        assert np.array_equal(got, want), (name, np.argwhere((got != want).any(-1))[:8].tolist())
        assert np.array_equal(got[~covered], img[~covered]), name
        if k > 0 and name in ("axes", "order", "text", "rings"):                    # (one pixel is easily missed; 17 x 33 is not)
            assert covered.any(), name


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "hbm"])
def test_batch_of_three_lists_one_empty(ck, glyphs, on_device):
    for (h, w, c) in _shapes()[1:]:
        prims, start, text = cases.batch(h, w, _bin_size())
        img = _image(3, h, w, c, seed=11)
        want, covered = ref.paint(img, prims, start, text, glyphs)
        got = _draw_raw(ck, img, prims, start, text, on_device)
        assert np.array_equal(got, want) and np.array_equal(got[1], img[1]) and covered[0].any() and covered[2].any()


def test_context_method_and_empty_calls(ck, glyphs):
    import torch
    from camkifu_amd import capi
    from camkifu_amd.core import overlay
    dl = overlay.DisplayList().rect(2, 2, 12, 9, (10, 200, 30), thickness=2).text(1, 1, "Ab", (255, 255, 255), alpha=128).disc(20, 8, 5, 77)
    prims, start, text = overlay.pack([dl])
    img = _image(1, 17, 33, 3, seed=3)
    want = ref.paint(img, prims, start, text, glyphs)[0]
    one = img[0].copy()
    assert ck.overlay_draw(one, dl) is one and np.array_equal(one, want[0])                   # a single image, in place
    t = torch.from_numpy(img.copy()).to("cuda:0")
    assert ck.overlay_draw(t, [dl]) is t and np.array_equal(t.cpu().numpy(), want)           # a batch in HBM, in place
    grey = np.ascontiguousarray(img[0, :, :, 0])
    want_grey = ref.paint(grey[None], prims, start, text, glyphs)[0][0]
    assert np.array_equal(ck.overlay_draw(grey.copy(), dl), want_grey)                       # (h, w): the colour's b byte
    # nothing to draw launches nothing and touches nothing
    same = img.copy()
    ck.overlay_draw(same, [overlay.DisplayList()])
    ck.overlay_draw(same[:0], [])
    ck.overlay_draw(same, [overlay.DisplayList().disc(-50, -50, 3).text(0, 0, "")])
    assert np.array_equal(same, img)
    for bad, lists in ((np.zeros((4, 4, 2), np.uint8), dl), (np.zeros((1, 4, 4, 4), np.uint8), [dl]), (img.astype(np.int16), [dl]),
                       (img[:, :, ::2], [dl]), (img, [dl, dl])):
        with pytest.raises(capi.CkError):
            ck.overlay_draw(bad, lists)
    with pytest.raises(capi.CkError) as e:                                                   # the limits, through the device entry
        ck.overlay_draw(img.copy(), [overlay.DisplayList().segment(0, 0, 5, 5, thickness=4)])
    assert e.value.code == capi.CK_ERR_ARG
    again = img[0].copy()
    assert np.array_equal(ck.overlay_draw(again, dl), want[0])                                # the context is fine afterwards


def _midgame(seed=4, stones=120):
    rng = np.random.RandomState(seed)
    codes = np.zeros(361, np.uint8)
    codes[rng.choice(361, stones, replace=False)] = rng.randint(1, 3, stones)
    fg = np.zeros((19, 19), np.int32)
    fg[5:7, 9:12] = 400
    return codes.reshape(19, 19), fg


def test_full_size_goban_list(ck, glyphs):
    """the goban annotation of tools/transcode.py --gobans --annotate on one 380 x 380 image"""
    from camkifu_amd.core import annotate, overlay
    from camkifu_amd.stone.stonesfinder import PosGrid
    codes, fg = _midgame()
    dl = annotate.goban_list(codes, fg, PosGrid(380), 57, 128, "B[D4] W[Q16]")
    assert len(dl) == 361 + 2 * 120 + 6 + 4
    prims, start, text = overlay.pack([dl])
    img = _image(1, 380, 380, 3, seed=9)
    want, covered = ref.paint(img, prims, start, text, glyphs)
    got = ck.overlay_draw(img.copy(), [dl])
    assert np.array_equal(got, want) and 0.05 < covered.mean() < 0.6


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _decoded(ck, path):
    from camkifu_amd.core import capture
    cap = capture.AviMjpegCapture(path, decode=ck.jpeg_decode)
    assert cap.isOpened() and cap.damaged == 0
    return np.stack([cap.read()[1] for _ in range(len(cap))])


def test_record_gobans_annotated(ck, glyphs, tmp_path):
    """batches of 4 frames of a synthetic film through record_gobans: with annotate=False the film is byte for byte the
    plain one; with annotate=True it decodes to what overlay_ref draws on the plain run's goban images, within the JPEG's
    own loss: the largest difference of the un-annotated pair, asked of every pixel 8 or more away from every drawn one.
    4:4:4, so that the blocks of every component are 8 x 8.  Measured on an MI355X: the un-annotated pair differs by up to
    41, the 30 297 compared pixels of the annotated film by up to 29."""
    from camkifu_amd import pipeline, synth
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import annotate, overlay
    from camkifu_amd.stone.harvest import replay
    from camkifu_amd.stone.nn_manager import NNManager
    from camkifu_amd.stone.stonesfinder import PosGrid
    tr = _tool("transcode")
    n, batch = 24, 4
    frames = synth.film(n, 480, 640, seed=8, quiet=6, move_every=6, hand_frames=2)[0].numpy()
    ck.cnn_set_weights(NNManager.init_net())
    raw, lists, mirror, grid = [], [], ControllerHeadless(), PosGrid(380)
    with pipeline.FastFilePipeline(480, 640, ControllerHeadless(), ctx=ck, bg_init_frames=3, keep_gobans=True) as pipe:
        for b0 in range(0, n, batch):
            emitted = pipe.process_batch(frames[b0:b0 + batch], batch)
            gobans, fg = pipe.last_gobans, pipe.last_fgcount
            gobans = np.zeros((batch, 380, 380, 3), np.uint8) if gobans is None else (gobans.cpu().numpy() if hasattr(gobans, "cpu") else np.asarray(gobans))
            raw.append(gobans)
            codes = replay(mirror, emitted)
            for f in range(batch):
                lists.append(annotate.goban_list(codes[f], None if fg is None else fg[f], grid, b0 + f + 1, n, annotate.moves_text(emitted[f])))
    raw = np.concatenate(raw)
    paths = [str(tmp_path / name) for name in ("plain.avi", "off.avi", "on.avi")]
    args = dict(quality=90, sampling=1, batch=batch, ctx=ck, bg_init_frames=3)
    tr.record_gobans(frames, paths[0], **args)
    tr.record_gobans(frames, paths[1], annotate=False, **args)
    res = tr.record_gobans(frames, paths[2], annotate=True, **args)
    with open(paths[0], "rb") as a, open(paths[1], "rb") as b:
        assert a.read() == b.read()
    plain, drawn = _decoded(ck, paths[0]), _decoded(ck, paths[2])
    assert plain.shape == drawn.shape == raw.shape and res["frames"] == n
    tolerance = int(np.abs(plain.astype(np.int16) - raw).max())                     # the un-annotated pair's own loss, plus 0
    prims, start, text = overlay.pack(lists)
    want, covered = ref.paint(raw, prims, start, text, glyphs)
    near = covered.copy()                                                           # less than 8 away from a drawn pixel
    for dy in range(-7, 8):
        for dx in range(-7, 8):
            if dx * dx + dy * dy < 64 and (dx or dy):
                ys, yd = slice(max(0, -dy), 380 - max(0, dy)), slice(max(0, dy), 380 - max(0, -dy))
                xs, xd = slice(max(0, -dx), 380 - max(0, dx)), slice(max(0, dx), 380 - max(0, -dx))
                near[:, yd, xd] |= covered[:, ys, xs]
    far = ~near
    apart = np.abs(drawn.astype(np.int16) - want).max(-1)
    # (for the record: the pixels whose own 8 x 8 block holds no drawn pixel see exactly the plain film's blocks)
    clean = ~np.repeat(np.repeat(np.pad(covered, ((0, 0), (0, 4), (0, 4))).reshape(n, 48, 8, 48, 8).any((2, 4)), 8, 1), 8, 2)[:, :380, :380]
    print("annotated film: tolerance %d, %d of %d pixels compared (largest difference %d), %d drawn, frames with a goban image: %d; "
          "in blocks without drawing: %d pixels, largest difference %d" % (
              tolerance, far.sum(), far.size, apart[far].max(), covered.sum(), int((raw.reshape(n, -1).max(1) > 0).sum()),
              clean.sum(), apart[clean].max()))
    # (a frame with a hand over the board is red nearly all over: not every frame has pixels left to compare)
    assert covered.reshape(n, -1).any(1).all() and far.reshape(n, -1).any(1).sum() >= n // 2
    assert apart[far].max() <= tolerance
    # and the drawing is there: where the caption's white text was drawn the film is bright, on every frame
    white = covered & (want == 255).all(-1)
    assert white.reshape(n, -1).any(1).all() and drawn[white].mean() > 170


def test_annotated_full_frames(ck, tmp_path):
    """tools/transcode.py --annotate without --gobans: the analysed frames at full size, captions on every one of them,
    corners, grid and stones once the board is found; the pipeline's own record is what the plain run's is"""
    from camkifu_amd import synth
    from camkifu_amd.stone.nn_manager import NNManager
    tr = _tool("transcode")
    n = 24
    frames = synth.film(n, 480, 640, seed=8, quiet=6, move_every=6, hand_frames=2)[0].numpy()
    ck.cnn_set_weights(NNManager.init_net())
    args = dict(quality=90, sampling=1, batch=4, ctx=ck, bg_init_frames=3)
    plain = tr.record_gobans(frames, str(tmp_path / "gobans.avi"), **args)
    res = tr.record_gobans(frames, str(tmp_path / "seen.avi"), annotate=True, full_frames=True, **args)
    assert res["requests"] == plain["requests"] and res["frames"] == n
    seen = _decoded(ck, str(tmp_path / "seen.avi"))
    assert seen.shape == frames.shape
    changed = (np.abs(seen.astype(np.int16) - frames).max(-1) > 60)                 # (far beyond the loss at quality 90)
    per_frame = changed.reshape(n, -1).sum(1)
    assert (per_frame > 50).all()                                                   # the caption, on every frame
    assert changed[:, 8:24, 8:200].reshape(n, -1).any(1).all()
    # the middle of the frame, where the board lies: the grid from the batch on in which the board is found (here the first:
    # what is drawn is the transform in force AFTER the batch), the stones on top once the fold has reported them
    # (361 rings of radius 3 are 16 pixels each; a few hundred of them must survive the threshold and the JPEG)
    middle = changed[:, 120:360, 200:440].reshape(n, -1).sum(1)
    print("annotated frames: changed pixels per frame", per_frame.tolist(), "in the middle", middle.tolist())
    assert len(res["requests"]) == n and any(res["requests"]) and not res["requests"][0]
    assert middle[0] > 500 and middle[-1] > middle[0]
    with pytest.raises(ValueError):
        tr.record_gobans(frames[:4], str(tmp_path / "no.avi"), full_frames=True, **args)

"""Frame downsampling on the GPU: ck.pyr_down and the fused I420 conversion against the plain reference of
tests/pyr_ref.py, bit for bit -- there is no tolerance anywhere in this file.  The cases (tests/pyr_cases.py) are built
for the branches of camkifu_amd/csrc/k_pyramid.hip: dword and narrow form, interior and rim tiles, every residue of the
width, the smallest sizes, batches whose frames start off a dword, several levels."""
import ctypes as C

import numpy as np
import pytest

from . import pyr_ref
from .pyr_cases import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def synth():
    from camkifu_amd import synth
    return synth


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pyr_down_equals_the_reference(ck, case):
    from camkifu_amd import capi
    img, levels = case["make"](), case["levels"]
    want = pyr_ref.pyr_down_batch(img, levels)
    assert want.shape[-3:-1] == capi.pyr_shape(img.shape[-3], img.shape[-2], levels)
    got = ck.pyr_down(img, levels)
    assert isinstance(got, np.ndarray) and got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), "host input: %d bytes differ" % int((got != want).sum())
    got = ck.pyr_down(_dev(img), levels)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), "device input"
    # a call of another size in between (the scratch buffers and the staging buffers are the context's), then again
    other = np.random.default_rng(99).integers(0, 256, (2, 37, 150, 3), dtype=np.uint8)
    assert np.array_equal(ck.pyr_down(other, 2), pyr_ref.pyr_down_batch(other, 2))
    assert np.array_equal(ck.pyr_down(img, levels), want), "after a call of another size"
    out = np.empty_like(want)
    assert ck.pyr_down(img, levels, out=out) is out and np.array_equal(out, want)
    out = _dev(np.zeros_like(want))
    assert ck.pyr_down(_dev(img), levels, out=out) is out and np.array_equal(out.cpu().numpy(), want)


def test_pyr_down_of_an_offset_device_pointer(ck):
    """a dword width behind a pointer that is not dword aligned takes the narrow form"""
    import torch
    img = np.random.default_rng(5).integers(0, 256, (66, 264, 3), dtype=np.uint8)
    buf = torch.empty(img.size + 8, dtype=torch.uint8, device="cuda")
    for off in (1, 2, 3, 4):
        view = buf[off:off + img.size].view(66, 264, 3)
        view.copy_(torch.from_numpy(img))
        assert view.data_ptr() % 4 == off % 4
        assert np.array_equal(ck.pyr_down(view).cpu().numpy(), pyr_ref.pyr_down(img)), off


I420_SHAPES = [
    # (n, h, w, levels): the dword form needs w % 8 == 0; 66 x 264 has one interior tile
    (1, 66, 264, 1), (3, 66, 264, 1), (2, 130, 520, 2), (1, 64, 256, 1), (1, 1080, 1920, 1), (1, 264, 528, 3),
    # narrow form: even widths that are not multiples of 8; the smallest frame
    (1, 66, 262, 1), (3, 36, 52, 1), (2, 66, 268, 2), (1, 2, 2, 1), (4, 2, 6, 1), (1, 70, 102, 3),
]


@pytest.mark.parametrize("n,h,w,levels", I420_SHAPES, ids=["%dx%dx%d_L%d" % s for s in I420_SHAPES])
def test_fused_conversion_equals_convert_then_pyr_down(ck, ora, n, h, w, levels):
    rng = np.random.default_rng(h * 31 + w + levels)
    raw = rng.integers(0, 256, (n, h * w * 3 // 2), dtype=np.uint8)
    raw[0, :h * w // 2] = rng.integers(0, 2, h * w // 2, dtype=np.uint8) * 255          # luma outside the studio range: saturation
    assert (w % 8 == 0) == (I420_SHAPES.index((n, h, w, levels)) < 6)
    bgr = np.stack([ora.i420_to_bgr(r, h, w) for r in raw])
    want = pyr_ref.pyr_down_batch(bgr, levels)
    got = ck.i420_to_bgr(raw, h, w, levels=levels)
    assert got.shape == want.shape and np.array_equal(got, want), "against the reference of the oracle's conversion"
    full = ck.i420_to_bgr(raw, h, w)
    assert np.array_equal(full, bgr)
    assert np.array_equal(ck.pyr_down(full, levels), got), "against the two-call composition"
    dev = ck.i420_to_bgr(_dev(raw), h, w, levels=levels)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want), "device input"
    import torch
    up = ck.i420_to_bgr(raw, h, w, to_device=torch.device("cuda", 0), levels=levels)
    assert up.is_cuda and np.array_equal(up.cpu().numpy(), want), "host input, device output"
    one = ck.i420_to_bgr(raw[0], h, w, levels=levels)
    assert one.shape == want.shape[1:] and np.array_equal(one, want[0])


def test_argument_errors_leave_the_context_usable(ck):
    from camkifu_amd import capi
    img = np.random.default_rng(1).integers(0, 256, (6, 10, 3), dtype=np.uint8)
    raw = np.zeros(6 * 10 * 3 // 2, np.uint8)
    bad = [
        lambda: ck.pyr_down(img, 0), lambda: ck.pyr_down(img, -1),
        lambda: ck.pyr_down(img, 4),                                       # 6x10 -> 3x5 -> 2x3 -> 1x2 -> a side below 2
        lambda: ck.pyr_down(np.zeros((1, 8, 3), np.uint8)),
        lambda: ck.pyr_down(np.zeros((2, 2, 3), np.uint8), 2),
        lambda: ck.i420_to_bgr(raw, 6, 10, levels=-1),
        lambda: ck.i420_to_bgr(raw, 6, 10, levels=4),
        lambda: ck.i420_to_bgr(np.zeros(3 * 6 * 3 // 2, np.uint8), 3, 6, levels=1),      # odd height
        lambda: ck.i420_to_bgr(np.zeros(4 * 5 * 3 // 2, np.uint8), 4, 5, levels=1),      # odd width
        lambda: capi.pyr_shape(6, 10, 4), lambda: capi.pyr_shape(6, 10, -1),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(capi.CkError):
            call()
        assert np.array_equal(ck.pyr_down(img), pyr_ref.pyr_down(img)), k
    # the same rules at the C-ABI itself: CK_ERR_ARG and a message, before any device work
    L, h = capi.lib(), ck._h
    out = np.zeros(6 * 10 * 3, np.uint8)
    ip, rp, op = (a.ctypes.data_as(C.c_void_p) for a in (img, raw, out))
    for rc in (L.ck_pyr_down(h, ip, 1, 6, 10, 0, capi.CK_HOST, op, capi.CK_HOST),
               L.ck_pyr_down(h, ip, 1, 6, 10, 4, capi.CK_HOST, op, capi.CK_HOST),
               L.ck_pyr_down(h, ip, 1, 1, 60, 1, capi.CK_HOST, op, capi.CK_HOST),
               L.ck_i420_to_bgr_pyr(h, rp, 1, 6, 10, 0, capi.CK_HOST, op, capi.CK_HOST),
               L.ck_i420_to_bgr_pyr(h, rp, 1, 6, 10, 4, capi.CK_HOST, op, capi.CK_HOST),
               L.ck_i420_to_bgr_pyr(h, rp, 1, 3, 20, 1, capi.CK_HOST, op, capi.CK_HOST),
               L.ck_i420_to_bgr_pyr(h, rp, 1, 4, 15, 1, capi.CK_HOST, op, capi.CK_HOST)):
        assert rc == 1 and L.ck_last_error(h)                              # CK_ERR_ARG
        assert not out.any()
    assert capi.pyr_shape(6, 10, 0) == (6, 10) and capi.pyr_shape(6, 10, 3) == (1, 2) and capi.pyr_shape(2160, 3840, 1) == (1080, 1920)
    assert np.array_equal(ck.i420_to_bgr(raw, 6, 10, levels=1), pyr_ref.pyr_down(ck.i420_to_bgr(raw, 6, 10)))


def test_timing_scopes(ck):
    raw = np.zeros((2, 16 * 24 * 3 // 2), np.uint8)
    ck.timing_enable(True)
    try:
        ck.timing_reset()
        ck.i420_to_bgr(raw, 16, 24, levels=2)
        ck.pyr_down(np.zeros((16, 24, 3), np.uint8), 3)
        assert ck.timing_get("i420_pyr_down")[1] == 1 and ck.timing_get("pyr_down")[1] == 1 + 3
        assert ck.timing_get("i420_to_bgr")[1] == 0                        # the full-size conversion never ran
    finally:
        ck.timing_enable(False)


# The clip of tests/test_pyr_ref_cpu.py (moves at frames 12, 24, 36 and 48, no hands).  The pipeline finds the board in its
# first batch of 16 and gives the stones path the frames after it, so with 38 background frames the one-off assessment
# reads frame 54: after the last move, before the clip ends.  (With the finder's default of 50 the 44 frames left would
# end inside the background phase and nothing would be recorded.)
CLIP = dict(nframes=60, every=12, bg=38)


def test_y4m_clip_through_the_pipeline_downsampled(ck, ora, synth, tmp_path):
    """the 1280x960 clip of the CPU suite stored as .y4m and run through process_y4m(downsample=1): the requests equal
    process_batch on the reference-downsampled frames, and the record is the clip's game"""
    from camkifu_amd import pipeline
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture as cap
    from camkifu_amd.stone.nn_manager import NNManager
    nframes = CLIP["nframes"]
    frames, corners, grids, moves = synth.video(nframes, 960, 1280, seed=synth.SEED, new_stone_every=CLIP["every"])
    frames = frames.numpy()
    # a 5 fps file read at file_fps = 5 visits frames 1, 3, 5, ...: every clip frame is written twice
    path = str(tmp_path / "game.y4m")
    i420 = [synth.bgr_to_i420(f) for f in frames]
    cap.write_y4m(path, (i420[k // 2] for k in range(2 * nframes)), 960, 1280, fps=(5, 1))
    c = cap.Y4MCapture(path)
    idx = cap.file_frame_indices(len(c), c.fps)
    assert idx == list(range(1, 2 * nframes, 2))
    ck.cnn_set_weights(NNManager.init_net())
    ctrl = ControllerHeadless()
    pipe = pipeline.FastFilePipeline(480, 640, ctrl, ctx=ck, bg_init_frames=CLIP["bg"])
    emitted = pipe.process_y4m(c, batch=16, downsample=1)
    assert c.get(cap.CAP_PROP_FRAME_WIDTH) == 1280 and c.get(cap.CAP_PROP_FRAME_HEIGHT) == 960
    small = np.stack([pyr_ref.pyr_down(ora.i420_to_bgr(f, 960, 1280)) for f in i420])
    ctrl2 = ControllerHeadless()
    pipe2 = pipeline.FastFilePipeline(480, 640, ctrl2, ctx=ck, bg_init_frames=CLIP["bg"])
    emitted2 = []
    for b0 in range(0, nframes, 16):
        emitted2 += pipe2.process_batch(small[b0:b0 + 16], len(small[b0:b0 + 16]))
    assert emitted == emitted2 and len(emitted) == nframes
    assert pipe.board.mtx is not None and np.array_equal(pipe.board.mtx, pipe2.board.mtx)
    assert ctrl.kifu.to_sgf() == ctrl2.kifu.to_sgf() and pipe.frames_done == nframes
    sym = "EBW"
    recorded = sorted((m.color, m.y, m.x) for m in ctrl.kifu.moves)
    assert recorded == sorted((sym[col], r, c) for col, r, c in moves) and len(moves) >= 1
    want = np.array([[sym[v] for v in row] for row in grids[-1]], dtype=object)
    assert (ctrl.get_stones() == want).all()


def test_4k_scene_board_detect_on_the_downsampled_frame(ck, ora, synth):
    """one 3840x2160 scene, downsampled on the GPU: the board record equals the oracle's on the reference-downsampled frame"""
    sc = synth.scene(2160, 3840, seed=77, density=0.3)
    fr = sc["frame"].numpy()
    want = pyr_ref.pyr_down(fr)
    small = ck.pyr_down(fr)
    assert small.shape == (1080, 1920, 3) and np.array_equal(small, want)
    out = ck.board_detect(small)[0]
    ref = ora.board_lines(ora.canny(ora.median(want, 15), 25, 75))
    print("4K scene, one level down: status %d, %d lines" % (ref["status"], len(ref["lines"])))
    assert out["n_lines"] == max(ref["status"], 0) and out["status"] == {-1: 1, -2: 2}.get(ref["status"], 0)
    assert np.array_equal(out["lines"], ref["lines"]) and out["n_contours"] == ref["n_contours"]
    assert out["biggest_area"] == ref["biggest_area"]
    # and straight from I420 (the frame as a 4K file would hold it)
    raw = synth.bgr_to_i420(fr)
    assert np.array_equal(ck.i420_to_bgr(raw, 2160, 3840, levels=1), pyr_ref.pyr_down(ora.i420_to_bgr(raw, 2160, 3840)))


def test_against_cv2_when_installed(ck):
    cv2 = pytest.importorskip("cv2", reason="cv2 is not installed: ck.pyr_down is not diffed against cv2.pyrDown here")
    for case in CASES:
        img = case["make"]()
        if img.ndim != 3 or case["levels"] != 1 or min(img.shape[:2]) < 3:
            continue
        assert np.array_equal(ck.pyr_down(img), cv2.pyrDown(img)), case["name"]

"""Frame downsampling (cv2.pyrDown behind CaptureReaderBase.downsample), the part that needs no GPU:

  * the two plain references of tests/pyr_ref.py agree on every case of tests/pyr_cases.py and on the sizes below;
  * every case has the property it was built for;
  * every mutant of the reference is told apart on at least one named case;
  * the host plumbing -- the hook, the lock-step reader, the .y4m capture, the sequential manager -- against a stub
    context that answers from the reference (tests/stub_ctx.py's OracleCtx with pyr_down and the fused conversion added).
"""
import threading

import numpy as np
import pytest

from camkifu_amd import cvconf, synth
from camkifu_amd.core import capture as cap

from . import pyr_ref
from .pyr_cases import BY_NAME, CASES
from .stub_ctx import OracleCtx


# ---------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("shape", [(2, 2), (3, 5), (7, 8), (16, 24), (33, 47), (480, 640), (481, 639)])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_two_references_agree(shape, channels):
    rng = np.random.default_rng(shape[0] * 7 + shape[1] + channels)
    img = rng.integers(0, 256, shape + ((channels,) if channels > 1 else ()), dtype=np.uint8)
    a, b = pyr_ref.pyr_down(img), pyr_ref.pyr_down_scipy(img)
    assert a.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2) + img.shape[2:] and a.dtype == np.uint8
    assert np.array_equal(a, b)


def test_reference_by_hand():
    """a 2x2 image by hand: both axes fold -2 -> 0, so taps (1 4 6 4 1) give the two values weights 8 and 8"""
    img = np.array([[10, 50], [90, 250]], np.uint8)
    rows = 8 * img[:, 0].astype(int) + 8 * img[:, 1].astype(int)
    assert pyr_ref.pyr_down(img)[0, 0] == (8 * rows[0] + 8 * rows[1] + 128) >> 8 == 100
    # a 5x5 impulse of 256 would show the kernel; with 8 bits: the centre weight 36 of 255 -> (36 * 255 + 128) >> 8
    imp = np.zeros((9, 9), np.uint8)
    imp[4, 4] = 255
    out = pyr_ref.pyr_down(imp)
    assert out[2, 2] == (36 * 255 + 128) >> 8 and out[1, 2] == (6 * 255 + 128) >> 8 and out[1, 1] == (255 + 128) >> 8


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_property_and_reference_agreement(case):
    img = case["make"]()
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    case["prop"](img)
    frames = img if img.ndim == 4 else img[None]
    for f in frames[:1 if case["big"] else None]:
        for _ in range(case["levels"]):
            a = pyr_ref.pyr_down(f)
            assert np.array_equal(a, pyr_ref.pyr_down_scipy(f))
            f = a
    out = pyr_ref.pyr_down_batch(img, case["levels"])
    assert out.shape[-3:-1] == pyr_ref.pyr_shape(img.shape[-3], img.shape[-2], case["levels"])


MUTANT_CASES = ["noise 66x264", "noise 66x263", "rounding edge 66x264", "rounding edge 40x53", "constant 255", "checkerboard",
                "odd h odd w", "2x2", "3x3"]


def test_every_mutant_is_told_apart():
    """each plausible mistake differs from the reference on at least one named case"""
    imgs = {n: BY_NAME[n]["make"]() for n in MUTANT_CASES}
    refs = {n: pyr_ref.pyr_down(i) for n, i in imgs.items()}
    assert set(pyr_ref.MUTANTS) == {"replicate border", "reflect without the 101", "truncation instead of +128",
                                    "round half to even", "kernel shifted by one pixel", "centre at 2x+1"}
    for name, mutant in pyr_ref.MUTANTS.items():
        caught = [n for n, i in imgs.items() if not np.array_equal(mutant(i), refs[n])]
        print("%-28s caught by %s" % (name, caught))
        assert caught, name
    # the rounding mutants are caught by the rounding cases in particular, and a constant image cannot catch anything
    for name in ("truncation instead of +128", "round half to even"):
        assert not np.array_equal(pyr_ref.MUTANTS[name](imgs["rounding edge 66x264"]), refs["rounding edge 66x264"])
    assert all(np.array_equal(m(imgs["constant 255"]), refs["constant 255"]) for m in pyr_ref.MUTANTS.values())


# ---------------------------------------------------------------------------------------------- host plumbing
class PyrCtx(OracleCtx):
    """the oracle stub plus the two calls of this feature, answered by the reference"""

    def __init__(self):
        super().__init__()
        self.pyr_calls, self.fused_calls = [], []

    def pyr_down(self, frames, levels=1, out=None):
        self.pyr_calls.append((tuple(np.asarray(frames).shape), levels))
        return pyr_ref.pyr_down_batch(np.asarray(frames), levels)

    def i420_to_bgr(self, i420, h, w, to_device=None, out=None, levels=0):
        from oracle import oracle as ora
        raw = np.asarray(i420)
        bgr = ora.i420_to_bgr(raw, h, w) if raw.ndim == 1 else np.stack([ora.i420_to_bgr(r, h, w) for r in raw])
        if levels:
            self.fused_calls.append(levels)
            bgr = pyr_ref.pyr_down_batch(bgr, levels)
        return bgr


class _VM:
    def __init__(self, video):
        self.controller = type("C", (), {"video": video})()
        self.processes = []

    def vid_progress(self, p):
        pass


@pytest.fixture
def levels(monkeypatch):
    def set_levels(n):
        monkeypatch.setattr(cvconf, "downsample", n)
    return set_levels


def _frames(n=40, h=18, w=26):
    fr = np.random.default_rng(12).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    fr[:, 0, 0, 0] = np.arange(n)
    return fr


def test_default_is_off_and_the_hook_is_the_identity():
    assert cvconf.downsample == 0
    ctx = PyrCtx()
    frames = _frames(4)
    rd = cap.CaptureReaderBase(cap.ArrayCapture(frames), _VM(0), ctx=ctx)
    img = frames[1]
    assert rd.downsample(True, img) == (True, img) and rd.downsample(True, img)[1] is img
    ok, got = rd.read(None)
    assert ok and np.array_equal(got, frames[0]) and ctx.pyr_calls == []


@pytest.mark.parametrize("n", [1, 2])
def test_a_consumer_gets_the_reference_result(levels, n):
    levels(n)
    ctx = PyrCtx()
    frames = _frames(3)
    rd = cap.CaptureReaderBase(cap.ArrayCapture(frames), _VM(0), ctx=ctx)
    for f in range(3):
        ok, got = rd.read(None)
        assert ok and isinstance(got, np.ndarray) and np.array_equal(got, pyr_ref.pyr_down_levels(frames[f], n))
    assert ctx.pyr_calls == [((18, 26, 3), n)] * 3
    # the end of the source, and the marker of a released lock-step reader, pass through untouched
    assert rd.read(None) == (False, None) and len(ctx.pyr_calls) == 3
    assert rd.downsample(False, None) == (False, None)
    assert rd.downsample(False, cvconf.unsynced) == (False, cvconf.unsynced)
    assert rd.downsample(True, cvconf.unsynced) == (True, cvconf.unsynced)
    # the capture's own properties keep describing the source
    assert rd.get(cap.CAP_PROP_FRAME_WIDTH) == 26 and rd.get(cap.CAP_PROP_FRAME_HEIGHT) == 18


def test_a_subclass_may_override_the_hook(levels):
    class Halved(cap.CaptureReaderBase):
        def downsample(self, ret, img):
            return ret, (img[::2, ::2] if ret else img)
    frames = _frames(2)
    rd = Halved(cap.ArrayCapture(frames), _VM(0))
    assert np.array_equal(rd.read(None)[1], frames[0, ::2, ::2])


def _y4m(tmp_path, n=60, h=16, w=24):
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, (n, h * w * 3 // 2), dtype=np.uint8)
    raw[:, :h * w] = np.arange(n, dtype=np.uint8)[:, None]              # a flat luma plane carries the frame id
    path = str(tmp_path / "clip.y4m")
    cap.write_y4m(path, raw, h, w)
    return path, raw


def test_y4m_capture_takes_the_fused_path(tmp_path, levels, ora):
    path, raw = _y4m(tmp_path, n=20)
    ctx = PyrCtx()
    rd = cap.CaptureReaderBase(cap.Y4MCapture(path, convert=ctx.i420_to_bgr), _VM(path), ctx=ctx)
    levels(1)
    seen = []
    while True:
        pos = int(rd.get(cap.CAP_PROP_POS_FRAMES))
        ok, img = rd.read(None)
        if not ok:
            break
        f = int(rd.get(cap.CAP_PROP_POS_FRAMES)) - 1
        seen.append(f)
        assert np.array_equal(img, pyr_ref.pyr_down(ora.i420_to_bgr(raw[f], 16, 24))) and img.shape == (8, 12, 3)
        assert pos < f
    # downsampling changes neither the frames visited nor their arithmetic, and the file still reports its own size
    assert seen == cap.file_frame_indices(20, 30.0, cvconf.file_fps) == [6, 13]
    assert ctx.fused_calls == [1, 1] and ctx.pyr_calls == []           # one fused conversion per frame, no second pass
    assert rd.get(cap.CAP_PROP_FRAME_WIDTH) == 24 and rd.get(cap.CAP_PROP_FRAME_HEIGHT) == 16
    levels(0)
    rd.set(cap.CAP_PROP_POS_FRAMES, 0)
    assert rd.read(None)[1].shape == (16, 24, 3) and ctx.fused_calls == [1, 1]


def test_file_frame_indices_do_not_depend_on_downsampling(levels):
    before = cap.file_frame_indices(100, 30.0), cap.file_frame_indices(40, 30.0, 60), cap.file_frame_indices(60, 30.0, 5, start=1)
    levels(2)
    assert (cap.file_frame_indices(100, 30.0), cap.file_frame_indices(40, 30.0, 60), cap.file_frame_indices(60, 30.0, 5, start=1)) == before
    assert before[0] == list(range(6, 100, 7))


class _Proc:
    def __init__(self):
        self.got, self.active = [], True

    def ready_to_read(self):
        return self.active


def test_lock_step_reader_downsamples_once_per_generation(tmp_path, levels, ora):
    """two consumers, one hook call (and one conversion) per frame served"""
    levels(1)
    path, raw = _y4m(tmp_path, n=60)
    calls = []

    class Counting(cap.CaptureReader):
        def downsample(self, ret, img):
            calls.append(ret)
            return super().downsample(ret, img)

    ctx = PyrCtx()
    vm = _VM(path)
    # the file's frames behind a capture without a fused path: the hook does the work
    source = cap.ArrayCapture(np.stack([ora.i420_to_bgr(r, 16, 24) for r in raw]), fps=30.0)
    rd = Counting(source, vm, ctx=ctx)
    rd.sleep_time = 0.001
    procs = [_Proc(), _Proc()]
    vm.processes = [type("VT", (), {"processor": p, "ready_to_read": p.ready_to_read})() for p in procs]

    def consume(p, delay):
        import time
        while True:
            ok, img = rd.read(p)
            if not ok:
                p.active = False
                return
            p.got.append(img.copy())
            img[:] = 255
            time.sleep(delay)
    ts = [threading.Thread(target=consume, args=(p, d)) for p, d in zip(procs, (0.0, 0.003))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in ts)
    expected = [0] + cap.file_frame_indices(60, 30.0, cvconf.file_fps, start=1)
    want = [pyr_ref.pyr_down(ora.i420_to_bgr(raw[f], 16, 24)) for f in expected]
    for p in procs:
        assert len(p.got) == len(want) and all(np.array_equal(a, b) for a, b in zip(p.got, want))
    # one generation per frame served (then failed reads at the end of the file, as many as consumers came back for):
    # the hook ran once for each, the kernel once per frame
    assert calls[:len(expected)] == [True] * len(expected) and not any(calls[len(expected):]) and len(calls) > len(expected)
    assert ctx.pyr_calls == [((16, 24, 3), 1)] * len(expected)
    rd.unsync_threads(True)
    assert rd.read(procs[0]) == (False, cvconf.unsynced)


def test_sequential_manager_on_a_downsampled_clip(monkeypatch, levels):
    """VManagerSeq over a 1280x960 clip with cvconf.downsample = 1: the finders work on 640x480 frames, find the board and
    record the clip's moves.  The clip plays its moves (one every 12 frames, no hands) while the stones finder still learns
    its background; the one-off assessment after those 50 frames reads them all -- moves in the steady state need the
    players' hands (synth.film), which this clip does not have."""
    from camkifu_amd import capi
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core.vmanager import VManagerSeq
    from oracle import oracle as ora
    nframes, every = 60, 12
    frames, corners, grids, moves = synth.video(nframes, 960, 1280, seed=synth.SEED, new_stone_every=every)
    frames = frames.numpy()
    ctx = PyrCtx()
    monkeypatch.setattr(capi, "Context", lambda device=0: ctx)
    monkeypatch.setattr(capi, "get_context", lambda device=0: ctx)
    monkeypatch.setattr(capi, "get_perspective_transform", ora.get_perspective_transform)
    levels(1)
    controller = ControllerHeadless(video=frames)
    vm = VManagerSeq(controller)
    vm.run()
    assert getattr(vm, "error", None) is None
    bf, sf = vm.board_finder, vm.stones_finder
    assert bf.mtx is not None and bf.corners.hull is not None
    assert np.abs(np.array(bf.corners.hull, np.float64) - corners / 2).max() < 12         # the corners of the half-size frame
    assert ctx.pyr_calls and set(ctx.pyr_calls) == {((960, 1280, 3), 1)} and len(ctx.pyr_calls) == nframes
    assert sf.total_f_processed > sf.bg_init_frames and sf.has_sampled
    # the record equals the clip's moves: every stone visible when the clip ends, with its colour, and nothing else
    sym = "EBW"
    got = controller.get_stones()
    want = np.array([[sym[v] for v in row] for row in grids[-1]], dtype=object)
    assert (got == want).all(), np.argwhere(got != want)
    recorded = sorted((m.color, m.y, m.x) for m in controller.kifu.moves)
    assert recorded == sorted((sym[col], r, c) for col, r, c in moves) and len(moves) == 4


# ---------------------------------------------------------------------------------------------- the timing tool
def _tool():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "ingest_timing.py")
    spec = importlib.util.spec_from_file_location("ingest_timing", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ingest_timing_rehearsal(tmp_path):
    """tools/ingest_timing.py at toy size, up to its first device call: the byte counts, the I420 maker, the in-memory clip,
    the plan -- and without a GPU it fails loudly instead of timing something else"""
    import torch
    from camkifu_amd import capi
    tool = _tool()
    by = tool.algorithmic_bytes(2160, 3840)
    assert by["fused"] == 2160 * 3840 * 9 // 4 == 18662400 and by["composition"] == 2160 * 3840 * 33 // 4 == 68428800
    assert by["i420_to_bgr"] + by["pyr_down"] == by["composition"]
    frames = np.random.default_rng(2).integers(0, 256, (3, 8, 12, 3), dtype=np.uint8)
    raw = tool.i420_of(torch.from_numpy(frames)).numpy()
    assert all(np.array_equal(raw[f], synth.bgr_to_i420(frames[f])) for f in range(3))
    clip = tool.I420Clip(raw, 8, 12)
    idx = cap.file_frame_indices(len(clip), clip.fps)
    assert idx == [1, 3, 5] and np.array_equal(clip.read_raw_batch(idx), raw)
    s = tool.spread_of([1.0, 1.2, 0.9, 1.1, 1.0])
    assert s["median_ms"] == 1.0 and s["min_ms"] == 0.9 and s["max_ms"] == 1.2 and abs(s["spread"] - 0.3) < 1e-9
    args = ["--size", "64x48", "--n", "2", "--film", "8", "--out", str(tmp_path / "t.json")]
    with pytest.raises(SystemExit):
        tool.main(args + ["--reps", "3"])                                  # fewer than 5 rounds is not a measurement
    if not torch.cuda.is_available():
        with pytest.raises(capi.CkError):
            tool.main(args)
        assert not (tmp_path / "t.json").exists()

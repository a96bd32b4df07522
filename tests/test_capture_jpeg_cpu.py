"""AviMjpegCapture, ImageCapture, write_mjpeg_avi and open_capture on the CPU: the container work and the capture surface,
with a stub in place of the GPU decoder (the decode itself: test_gpu_jpeg.py)."""
import numpy as np
import pytest

from camkifu_amd.core import capture as cap

from . import jpeg_cases, jpeg_ref


def _stub(streams):
    """stands for Context.jpeg_decode: a (n, 1, 1, 3) 'frame' that identifies the bytes it was given"""
    return np.array([[[[len(bytes(s)) % 251, bytes(s)[-3], 7]]] for s in streams], np.uint8)


class _VM:
    def __init__(self, video):
        self.controller = type("C", (), {"video": video})()


def test_tiny_avi_frames_fps_repeat_seek_and_properties():
    idx, _ = jpeg_cases.avi_reference()
    c = cap.AviMjpegCapture(jpeg_cases.AVI, decode=_stub)
    assert c.isOpened() and c.error is None
    assert len(c) == 6 and (c.h, c.w, c.fps) == (48, 64, 25.0) and c.damaged == 1
    assert c.get(cap.CAP_PROP_FRAME_COUNT) == 6.0 and c.get(cap.CAP_PROP_FPS) == 25.0
    assert c.get(cap.CAP_PROP_FRAME_WIDTH) == 64.0 and c.get(cap.CAP_PROP_FRAME_HEIGHT) == 48.0
    raw = c.read_raw_batch(range(6))
    want = [idx["chunks"][k if k != 3 else 2] for k in range(6)]
    assert [bytes(r) for r in raw] == want                       # the empty chunk repeats the frame before it
    assert all(isinstance(r, np.ndarray) and not r.flags.owndata for r in raw)       # views of the mapping
    frames = []
    while True:
        ok, img = c.read()
        if not ok:
            break
        frames.append(img)
    assert len(frames) == 6 and c.get(cap.CAP_PROP_POS_FRAMES) == 6.0 and c.progress() == 1.0
    assert np.array_equal(frames[3], frames[2]) and not np.array_equal(frames[4], frames[2])
    assert np.array_equal(np.stack(frames), _stub(want))
    c.seek(0.5)
    assert c.pos == 3 and c.get(cap.CAP_PROP_POS_AVI_RATIO) == 0.5
    assert c.set(cap.CAP_PROP_POS_FRAMES, 5) and np.array_equal(c.read()[1], frames[5])
    assert not c.set(cap.CAP_PROP_FPS, 1) and c.get(99) == 0.0
    c.release()
    assert not c.isOpened() and c.read() == (False, None)


def test_write_mjpeg_avi_round_trips(tmp_path):
    cases = jpeg_cases.file_cases()
    good = [cases[n][0] for n in ("ramp_48x64_420_q90_r0", "noise_48x64_420_q90_r3", "ramp_48x64_444_q5_r0")]
    other_size = cases["ramp_17x33_420_q90_r0"][0]
    chunks = [b"", good[0], good[1], b"not a jpeg", other_size, good[2] + b"\0"]      # (odd and even lengths: padding)
    path = str(tmp_path / "clip.avi")
    cap.write_mjpeg_avi(path, chunks, 48, 64, fps=(30000, 1001))
    with open(path, "rb") as f:
        idx = jpeg_ref.avi_index(f.read())
    assert (idx["h"], idx["w"]) == (48, 64) and abs(idx["fps"] - 29.97) < 0.001 and idx["chunks"] == chunks
    c = cap.AviMjpegCapture(path, decode=_stub)
    assert c.isOpened() and len(c) == 6 and abs(c.fps - 29.97) < 0.001 and c.damaged == 3
    assert c.read() == (False, None)                                # nothing good before the first frame
    raw = c.read_raw_batch(range(6))
    assert raw[0] is None and [bytes(r) for r in raw[1:]] == [good[0], good[1], good[1], good[1], good[2] + b"\0"]
    assert c.read()[0] and c.pos == 2


def test_files_that_are_not_mjpeg_avi_do_not_open(tmp_path):
    bad = tmp_path / "bad.avi"
    bad.write_bytes(b"RIFF\x04\0\0\0WAVE")
    assert not cap.AviMjpegCapture(str(bad)).isOpened() and isinstance(cap.AviMjpegCapture(str(bad)).error, cap.AviError)
    assert not cap.AviMjpegCapture(str(tmp_path / "missing.avi")).isOpened()
    with open(jpeg_cases.AVI, "rb") as f:
        data = f.read()
    other = tmp_path / "h264.avi"
    other.write_bytes(data.replace(b"MJPG", b"H264"))
    c = cap.AviMjpegCapture(str(other))
    assert not c.isOpened() and "only MJPG" in str(c.error)


def _chunk(cc, body):
    import struct
    return cc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _lst(kind, body):
    import struct
    return b"LIST" + struct.pack("<I", len(body) + 4) + kind + body


def _rebuilt(tmp_path, name, movi, extra_strl=b""):
    """tiny.avi's header lists around another movi list (and, optionally, a stream list in front of the video's)"""
    import struct
    with open(jpeg_cases.AVI, "rb") as f:
        data = f.read()
    hdrl_len = struct.unpack("<I", data[16:20])[0]
    hdrl = data[12:20 + hdrl_len]
    if extra_strl:                                           # hdrl = LIST size 'hdrl' avih-chunk strl-list
        avih_end = 12 + 8 + struct.unpack("<I", hdrl[16:20])[0]
        body = hdrl[12:avih_end] + extra_strl + hdrl[avih_end:]
        hdrl = _lst(b"hdrl", body)
    body = b"AVI " + hdrl + movi
    path = tmp_path / name
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


def test_rec_lists_other_streams_and_deep_nesting(tmp_path):
    import struct
    cases = jpeg_cases.file_cases()
    a, b = cases["ramp_48x64_420_q90_r0"][0], cases["noise_48x64_420_q90_r3"][0]
    # chunks grouped in 'rec ' lists, with audio between them
    movi = _lst(b"movi", _lst(b"rec ", _chunk(b"00dc", a) + _chunk(b"01wb", b"\1\2\3")) + _lst(b"rec ", _chunk(b"00db", b))
                + _chunk(b"00dc", a))
    c = cap.AviMjpegCapture(_rebuilt(tmp_path, "rec.avi", movi), decode=_stub)
    assert c.isOpened() and [bytes(r) for r in c.read_raw_batch(range(len(c)))] == [a, b, a]
    # an audio stream in front: the video stream is number 01, and chunks of stream 00 are not its frames
    auds = _lst(b"strl", _chunk(b"strh", b"auds" + bytes(52)) + _chunk(b"strf", bytes(18)))
    movi = _lst(b"movi", _chunk(b"00wb", b"\0" * 10) + _chunk(b"01dc", a) + _chunk(b"00dc", b) + _chunk(b"01dc", b))
    c = cap.AviMjpegCapture(_rebuilt(tmp_path, "two.avi", movi, extra_strl=auds), decode=_stub)
    assert c.isOpened() and c.damaged == 0 and [bytes(r) for r in c.read_raw_batch(range(len(c)))] == [a, b]
    # lists nested deeper than any file has them: an error of the capture, not of the interpreter
    deep = _chunk(b"00dc", a)
    for _ in range(3000):
        deep = _lst(b"rec ", deep)
    c = cap.AviMjpegCapture(_rebuilt(tmp_path, "deep.avi", _lst(b"movi", deep)), decode=_stub)
    assert not c.isOpened() and isinstance(c.error, cap.AviError) and "nested" in str(c.error)
    # a chunk whose length runs past the file, and a zero-length list
    movi = _lst(b"movi", _chunk(b"00dc", a) + b"LIST" + struct.pack("<I", 0) + b"00dc" + struct.pack("<I", 1 << 30) + b[:100])
    c = cap.AviMjpegCapture(_rebuilt(tmp_path, "cut.avi", movi), decode=_stub)
    assert c.isOpened() and len(c) == 2 and c.damaged == 1 and bytes(c.read_raw_batch([1])[0]) == a


def test_binding_holds_sizes_and_types_without_a_gpu():
    from camkifu_amd import capi
    for h, w in [(1, 1), (8, 8), (17, 33), (136, 200), (1080, 1920)]:
        for s in (0, 1, 2, 3):
            assert capi.jpeg_blocks(h, w, s) == jpeg_ref.n_blocks(h, w, s)
    with pytest.raises(capi.CkError):
        capi.jpeg_blocks(8, 8, 4)
    capi._check_array(np.zeros((2, 3), np.int16), (2, 3), np.int16, "coef")
    for bad in (np.zeros((2, 4), np.int16), np.zeros((2, 3), np.int32), np.zeros((3, 2), np.int16).T, [[0] * 3] * 2):
        with pytest.raises(capi.CkError, match="coef: "):
            capi._check_array(bad, (2, 3), np.int16, "coef")
    torch = pytest.importorskip("torch")
    capi._check_array(torch.zeros((2, 3), dtype=torch.int16), (2, 3), (np.uint16, np.int16), "quant")
    with pytest.raises(capi.CkError, match="quant: "):
        capi._check_array(torch.zeros((2, 3), dtype=torch.float32), (2, 3), (np.uint16, np.int16), "quant")


def test_reader_thinning_runs_over_the_avi(tmp_path):
    frame = jpeg_cases.file_cases()["ramp_48x64_420_q90_r0"][0]
    path = str(tmp_path / "long.avi")
    cap.write_mjpeg_avi(path, [frame + bytes([0] * (k + 1)) for k in range(60)], 48, 64, fps=(30, 1))
    seen = []

    def decode(streams):
        seen.append(len(bytes(streams[0])) - len(frame) - 1)
        return _stub(streams)

    rd = cap.CaptureReaderBase(cap.AviMjpegCapture(path, decode=decode), _VM(path), fps=5)
    while rd.read()[0]:
        pass
    assert seen == cap.file_frame_indices(60, 30.0, 5) == list(range(6, 60, 7))
    assert rd.get(cap.CAP_PROP_FRAME_COUNT) == 60.0          # every other attribute is the capture's


def test_image_capture_is_capture_reader_img(tmp_path):
    path = tmp_path / "still.JPG"
    path.write_bytes(jpeg_cases.file_cases()["ramp_48x64_420_q90_r0"][0])
    c = cap.ImageCapture(str(path), decode=_stub)
    assert c.isOpened()
    ok, a = c.read()
    ok2, b = c.read()
    assert ok and ok2 and np.array_equal(a, b) and a is not b
    a[:] = 0
    assert c.read()[1].any()                                 # a copy every time
    assert c.get(cap.CAP_PROP_FPS) == 0 and c.get(cap.CAP_PROP_POS_FRAMES) == 0
    assert not cap.ImageCapture(str(tmp_path / "missing.jpg"), decode=_stub).isOpened()


def test_open_capture_dispatches(tmp_path, monkeypatch):
    still = tmp_path / "a.jpeg"
    still.write_bytes(jpeg_cases.file_cases()["ramp_48x64_420_q90_r0"][0])
    from camkifu_amd import capi
    monkeypatch.setattr(capi, "get_context", lambda device=0: type("Ctx", (), {"jpeg_decode": staticmethod(_stub)})())
    assert isinstance(cap.open_capture(jpeg_cases.AVI), cap.AviMjpegCapture)
    assert isinstance(cap.open_capture(str(still)), cap.ImageCapture) and cap.open_capture(str(still)).isOpened()
    assert isinstance(cap.open_capture(str(tmp_path / "x.JPG")), cap.ImageCapture)
    assert isinstance(cap.open_capture(str(tmp_path / "x.y4m")), cap.Y4MCapture)
    assert isinstance(cap.open_capture(np.zeros((2, 4, 4, 3), np.uint8)), cap.ArrayCapture)

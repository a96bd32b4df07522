"""The runs mode of the PNG encoder on the GPU: png_encode(.., runs=True) against the staged host encoder byte for byte (which
tests/test_png_runs_cpu.py holds to the rule token by token), the token statistics against tests/png_runs_ref.py, the
library's own reader on the new streams, mode changes on one context, and the users' entry points."""
import types
import zlib

import numpy as np
import pytest

from . import png_ref, png_runs_ref
from .test_png_cpu import _image
from .test_png_runs_cpu import constructed

pytestmark = pytest.mark.gpu

# those of test_gpu_png: 16 rows of 1 + 3 * 21 = 64 bytes are a band of exactly one tile
ENC_SHAPES = [(1, 1), (1, 17), (17, 1), (15, 6), (16, 6), (17, 6), (33, 5), (3, 341), (3, 342), (16, 21), (16, 22), (40, 90)]


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _equals_staged(ck, frames):
    import torch
    from camkifu_amd import capi
    dev = torch.from_numpy(np.ascontiguousarray(frames)).to("cuda:0")
    for flt in (None, 0, 4):
        want = capi.png_encode_staged(frames, flt, runs=True)
        assert ck.png_encode(frames, flt, runs=True) == want, flt
        assert ck.png_encode(dev, flt, runs=True) == want, flt
    return want


@pytest.mark.parametrize("shape", ENC_SHAPES, ids=["%dx%d" % s for s in ENC_SHAPES])
def test_runs_mode_equals_the_staged_encoder(ck, shape):
    bgr = _image(*shape)
    data = _equals_staged(ck, bgr)
    assert np.array_equal(png_ref.decode(data[0]), bgr) and np.array_equal(ck.png_decode(data)[0], bgr)


@pytest.mark.parametrize("name", sorted(constructed()))
def test_runs_mode_on_constructed_images(ck, name):
    frames = constructed()[name]
    data = _equals_staged(ck, frames)
    assert np.array_equal(ck.png_decode(data), frames if frames.ndim == 4 else frames[None])


def _frame_counts(data, bgr):
    h, w = bgr.shape[:2]
    rows = zlib.decompress(png_ref.walk(data)["idat"])
    step = 16 * (1 + 3 * w)
    lit, match = png_runs_ref.counts([rows[i:i + step] for i in range(0, len(rows), step)])
    return dict(literals=lit, matches=match)


def test_run_stats_are_the_token_counts(ck):
    frames = np.stack([_image(37, 45, 1), np.zeros((37, 45, 3), np.uint8), _image(37, 45, 2)])
    frames[2, 20:, 5:30] = 9
    data = ck.png_encode(frames, runs=True)
    want = [_frame_counts(d, f) for d, f in zip(data, frames)]
    assert ck.png_run_stats() == want and want[1]["matches"] > 0 and want[1]["literals"] < 20
    plain = ck.png_encode(frames)
    assert ck.png_run_stats() == [dict(literals=37 * (1 + 3 * 45), matches=0)] * 3
    assert plain != data


def test_a_mixed_batch_round_trips_through_our_own_reader(ck):
    import torch
    from camkifu_amd import capi
    frames = np.stack([np.zeros((50, 70, 3), np.uint8), _image(50, 70, 2), _image(50, 70, 3)])
    frames[2, 10:30] = frames[2, 10, 0]                       # twenty equal rows: one long run under filter None, zeros under the others
    for src in (frames, torch.from_numpy(frames).to("cuda:0")):
        for flt in (None, 0):
            out = ck.png_encode(src, flt, runs=True)
            assert out == capi.png_encode_staged(frames, flt, runs=True)
            assert np.array_equal(ck.png_decode(out), frames)
    for d in out:
        assert capi.png_inflate(png_ref.walk(d)["idat"]) == zlib.decompress(png_ref.walk(d)["idat"])


def test_mode_switching_on_one_context():
    """stale scratch and stale header room: runs, default, runs at two sizes on a context of its own"""
    import ctypes as C
    from camkifu_amd import capi
    ctx = capi.Context(0)
    try:
        a, b = _image(40, 90), _image(17, 6)
        a[5:30, 10:60] = 0
        assert ctx.png_run_stats() == []                       # nothing encoded yet; the C call says so in words
        L, one = capi.lib(), (C.c_longlong * 1)()
        assert L.ck_png_run_stats(ctx._h, 1, one, one) == capi.CK_ERR_STATE and b"no ck_png_encode" in L.ck_last_error(ctx._h)
        before = {k: ctx.png_encode(x) for k, x in (("a", a), ("b", b))}            # before the mode was ever used
        assert before == {"a": capi.png_encode_staged(a), "b": capi.png_encode_staged(b)}
        for x, k in ((a, "a"), (b, "b"), (a, "a")):
            assert ctx.png_encode(x, runs=True) == capi.png_encode_staged(x, runs=True)
            assert ctx.png_encode(x) == before[k]
            assert ctx.png_encode(x, runs=True) == capi.png_encode_staged(x, runs=True)
        ctx.png_set_encode_matches("runs")                     # the context's own setting, and a call that overrides it
        assert ctx.png_encode(b) == capi.png_encode_staged(b, runs=True) and ctx.png_encode(b, runs=False) == before["b"]
        assert ctx.png_encode(a) == capi.png_encode_staged(a, runs=True)
        ctx.png_set_encode_matches("none")
        assert ctx.png_encode(a) == before["a"]
        with pytest.raises(capi.CkError, match="'none' or 'runs'"):
            ctx.png_set_encode_matches("rle")
        L = capi.lib()
        assert L.ck_png_set_encode_matches(ctx._h, 2) == capi.CK_ERR_ARG and b"match mode 2" in L.ck_last_error(ctx._h)
        assert ctx.png_encode(a) == before["a"]
    finally:
        ctx.close()


def test_write_png_and_snapshot_png_in_runs_mode(ck, tmp_path, monkeypatch):
    import torch
    from camkifu_amd import capi, cvconf
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture
    from camkifu_amd.core.vmanager import VManagerBase
    from camkifu_amd.stone import nn_manager as nm
    monkeypatch.setattr(capi, "get_context", lambda device=0: ck)
    img = _image(45, 61)
    img[10:30, 5:50] = (3, 200, 90)
    path = str(tmp_path / "still.png")
    n = capture.write_png(path, torch.from_numpy(img).to("cuda:0"), runs=True)
    with open(path, "rb") as f:
        data = f.read()
    assert n == len(data) and data == capi.png_encode_staged(img, runs=True)[0]
    assert n < capture.write_png(str(tmp_path / "plain.png"), img)
    ok, got = capture.open_capture(path).read()
    assert ok and np.array_equal(got, img)
    monkeypatch.setattr(cvconf, "snapshot_dir", str(tmp_path))
    vm = VManagerBase(ControllerHeadless(), bf="None", sf="None")
    big = _image(380, 380)
    big[100:200] = 0
    vm.stones_finder = types.SimpleNamespace(goban_img=big)
    snap = vm.snapshot_png(runs=True)
    assert snap == str(tmp_path / "snapshot-0.png")
    with open(snap, "rb") as f:
        assert f.read() == capi.png_encode_staged(big, runs=True)[0]
    assert np.array_equal(nm.NNManager.load_snapshot(snap), big)

"""PNG on the GPU: png_decode against tests/png_ref.py byte for byte -- filters in every row position, every colour type and
depth, heights and row lengths around the seams of the unfilter kernel, batches, damage -- png_encode against the staged
host encoder byte for byte, and the users' entry points end to end."""
import struct
import types
import zlib

import numpy as np
import pytest

from . import png_cases, png_ref
from .test_png_cpu import _fibonacci_band, _image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def seams():
    from camkifu_amd import capi
    s = capi.png_tiles()
    assert s == dict(band_rows=16, tile_bytes=1024, chunk_bytes=24, group_rows=256)       # what the cases below are sized for
    return s


def _decode_one(ck, data):
    return ck.png_decode([data])[0]


# ---- reading ----
@pytest.mark.parametrize("start", range(5))
def test_every_filter_on_row_0_and_after_every_other(ck, start):
    """27 rows: `start` on row 0, then a walk through all 25 ordered pairs; smooth pixels, so that Avg and Paeth chains carry"""
    for ct, depth, w in ((2, 8, 19), (6, 16, 7), (0, 8, 30), (3, 4, 41)):
        data, want = png_cases.image(w, 27, ct, depth, start=start, smooth=True, flavour="rle")
        assert np.array_equal(png_ref.decode(data), want)            # (the two statements of the reference agree)
        assert np.array_equal(_decode_one(ck, data), want), (ct, depth)


@pytest.mark.parametrize("ct,depth", png_cases.TYPES)
def test_every_colour_type_and_depth(ck, ct, depth):
    for w, h in ((1, 1), (13, 11), (70, 5)):
        data, want = png_cases.image(w, h, ct, depth, seed=1)
        assert np.array_equal(_decode_one(ck, data), want), (w, h)
    if ct == 3:                                               # an index beyond the palette gives black
        data, want = png_cases.image(13, 11, ct, depth, seed=2, plte_n=max(1, (1 << depth) // 2))
        assert (want == 0).all(2).any() and np.array_equal(_decode_one(ck, data), want)


@pytest.mark.parametrize("h", [1, 2, 63, 64, 65, 129, 255, 256, 257, 513])
def test_heights_around_the_wave_and_workgroup_seams(ck, seams, h):
    """width 3: one chunk a row, so the rows alone carry the dependency; Up, Avg and Paeth tie every row to the one above"""
    for ct, depth in ((2, 8), (0, 1)):
        data, want = png_cases.image(3, h, ct, depth, seed=3, smooth=True, filters=[(2, 3, 4)[y % 3] for y in range(h)])
        assert np.array_equal(_decode_one(ck, data), want), (ct, depth)


@pytest.mark.parametrize("bpp", [1, 2, 3, 4, 6, 8])
def test_row_lengths_around_the_chunk_size(ck, seams, bpp):
    ct, depth = {1: (0, 8), 2: (4, 8), 3: (2, 8), 4: (6, 8), 6: (2, 16), 8: (6, 16)}[bpp]
    ch = seams["chunk_bytes"]
    widths = sorted({1, (ch - 1) // bpp, ch // bpp, -(-(ch + 1) // bpp), 2 * ch // bpp, 2 * ch // bpp + 1})
    for w in widths:
        data, want = png_cases.image(w, 9, ct, depth, seed=4, smooth=True, filters=[4, 3, 4, 1, 2, 3, 4, 0, 3])
        assert np.array_equal(_decode_one(ck, data), want), w


def test_sub_byte_rows_that_are_no_byte_multiple(ck):
    for w, ct, depth in ((5, 0, 1), (3, 0, 2), (5, 3, 1), (3, 3, 2), (7, 0, 4), (1, 0, 1), (193, 0, 1), (97, 3, 2)):
        data, want = png_cases.image(w, 6, ct, depth, seed=5)
        assert np.array_equal(_decode_one(ck, data), want), (w, ct, depth)


def test_rows_longer_than_the_workgroup_has_lanes(ck, seams):
    """more chunks in a row than rows in flight: the second group of rows starts behind the first one's last chunk"""
    w = (seams["group_rows"] + 2) * seams["chunk_bytes"] // 6 + 1
    h = seams["group_rows"] + 2
    data, want = png_cases.image(w, h, 2, 16, seed=6, smooth=True, filters=[(4, 3, 2, 1)[y % 4] for y in range(h)], flavour="fixed")
    assert np.array_equal(_decode_one(ck, data), want)


def test_a_batch_of_different_types_filters_and_chunkings(ck):
    import torch
    made = [png_cases.image(21, 17, 2, 8, seed=7, start=4, flavour="huffman"),
            png_cases.image(21, 17, 3, 2, seed=8, start=3, idat_split=11),
            png_cases.image(21, 17, 6, 16, seed=9, start=1, flavour="stored")]
    out = ck.png_decode([d for d, _ in made])
    assert out.shape == (3, 17, 21, 3)
    for k, (_, want) in enumerate(made):
        assert np.array_equal(out[k], want), k              # one image does not bleed into the next
    dev = ck.png_decode([d for d, _ in made], to_device="cuda:0")
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), out)
    buf = torch.zeros((3, 17, 21, 3), dtype=torch.uint8, device="cuda:0")
    assert ck.png_decode([d for d, _ in made], out=buf) is buf and np.array_equal(buf.cpu().numpy(), out)
    golden = png_cases.golden()
    names = sorted(golden)
    out = ck.png_decode([golden[k][0] for k in names])
    for k, name in enumerate(names):
        assert np.array_equal(out[k], golden[name][1]), name


def test_a_damaged_frame_in_a_batch_is_named(ck):
    from camkifu_amd import capi
    good = [png_cases.image(9, 8, 2, 8, seed=k)[0] for k in range(3)]
    bad = bytearray(good[1])
    bad[-20] ^= 0x40                                          # inside the zlib stream's tail: IDAT's CRC no longer holds
    with pytest.raises(capi.CkError, match="frame 1: .*CRC") as e:
        ck.png_decode([good[0], bytes(bad), good[2]])
    assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 1
    other = png_cases.image(9, 7, 2, 8)[0]
    with pytest.raises(capi.CkError, match="frame 2: 9x7 where the batch is 9x8") as e:
        ck.png_decode([good[0], good[1], other])
    assert e.value.bad_frame == 2
    flt = bytearray(png_ref.filtered(np.zeros((8, 27), np.uint8), 2, 8, [0] * 8))
    flt[3 * 28] = 7
    wrong = png_ref.SIG + png_ref.chunk(b"IHDR", struct.pack(">IIBBBBB", 9, 8, 8, 2, 0, 0, 0)) + png_ref.chunk(b"IDAT", zlib.compress(bytes(flt))) + png_ref.chunk(b"IEND")
    with pytest.raises(capi.CkError, match="frame 0: row 3: filter type 7"):
        ck.png_decode([wrong, good[0]])
    assert np.array_equal(ck.png_decode(good)[2], png_ref.decode(good[2]))       # and the context still works


# ---- writing ----
ENC_SHAPES = [(1, 1), (1, 17), (17, 1), (15, 6), (16, 6), (17, 6), (33, 5),
              (3, 341), (3, 342), (16, 21), (16, 22), (40, 90)]      # 16 rows of 1 + 3 * 21 = 64 bytes: a band of exactly one tile


@pytest.mark.parametrize("shape", ENC_SHAPES, ids=["%dx%d" % s for s in ENC_SHAPES])
def test_encode_equals_the_staged_encoder(ck, shape):
    import torch
    from camkifu_amd import capi
    bgr = _image(*shape)
    for flt in (None, 0, 4):
        want = capi.png_encode_staged(bgr, flt)
        assert ck.png_encode(bgr, flt) == want, flt
    assert ck.png_encode(torch.from_numpy(bgr).to("cuda:0")) == capi.png_encode_staged(bgr)
    assert np.array_equal(ck.png_decode(capi.png_encode_staged(bgr))[0], bgr)
    assert np.array_equal(ck.png_decode(ck.png_encode(bgr, 3))[0], bgr)


def test_encode_special_bands_and_batches(ck):
    import torch
    from camkifu_amd import capi
    fib = _fibonacci_band()
    assert ck.png_encode(fib, 0) == capi.png_encode_staged(fib, 0)
    assert np.array_equal(png_ref.decode(ck.png_encode(fib, 0)[0]), fib)
    zero = np.zeros((35, 50, 3), np.uint8)
    data = ck.png_encode(zero)
    assert data == capi.png_encode_staged(zero) and np.array_equal(png_ref.decode(data[0]), zero)
    frames = np.stack([_image(37, 45, s) for s in range(3)])
    frames[1] = 0
    for src in (frames, torch.from_numpy(frames).to("cuda:0")):
        out = ck.png_encode(src)
        assert out == capi.png_encode_staged(frames)
        assert np.array_equal(ck.png_decode(out), frames)
    with pytest.raises(capi.CkError, match="filter"):
        ck.png_encode(frames, 9)


# ---- end to end ----
def test_write_png_and_open_capture(ck, tmp_path, monkeypatch):
    import torch
    from camkifu_amd import capi
    from camkifu_amd.core import capture
    monkeypatch.setattr(capi, "get_context", lambda device=0: ck)
    img = _image(45, 61)
    path = str(tmp_path / "still.png")
    n = capture.write_png(path, torch.from_numpy(img).to("cuda:0"))
    with open(path, "rb") as f:
        data = f.read()
    assert n == len(data) and data == capi.png_encode_staged(img)[0]
    cap = capture.open_capture(path)
    assert isinstance(cap, capture.ImageCapture) and cap.isOpened()
    ok, got = cap.read()
    assert ok and np.array_equal(got, img)
    with pytest.raises(ValueError):
        capture.write_png(path, img[None])


def test_png_snapshot_feeds_gen_data(ck, tmp_path, monkeypatch):
    from camkifu_amd import capi, cvconf
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core.vmanager import VManagerBase
    from camkifu_amd.golib_shim import Move, NP_TYPE, B, W
    from camkifu_amd.stone import nn_manager as nm
    monkeypatch.setattr(capi, "get_context", lambda device=0: ck)
    monkeypatch.setattr(cvconf, "snapshot_dir", str(tmp_path))
    ctrl = ControllerHeadless()
    for mv in ((B, 3, 3), (W, 15, 15), (B, 16, 3)):
        ctrl.pipe("append", Move(NP_TYPE, mv))
    vm = VManagerBase(ctrl, bf="None", sf="None")
    assert vm.snapshot_png(True) is None
    img = _image(380, 380)
    vm.stones_finder = types.SimpleNamespace(goban_img=img)
    assert vm.snapshot(True) == str(tmp_path / "snapshot-0.npy")
    assert vm.snapshot_png(True) == str(tmp_path / "snapshot-1.png")       # one counter for every kind
    assert (tmp_path / "game-1.sgf").exists()
    mgr = nm.NNManager()
    assert np.array_equal(nm.NNManager.load_snapshot(str(tmp_path / "snapshot-1.png")), img)
    x0, y0 = mgr.gen_data(str(tmp_path / "snapshot-0.npy"))
    x1, y1 = mgr.gen_data(str(tmp_path / "snapshot-1.png"))
    assert mgr.stones_source == "sgf" and np.array_equal(x1, x0) and np.array_equal(y1, y0)
    with pytest.raises(ValueError, match="npy or jpg"):
        vm.snapshot(fmt="png")

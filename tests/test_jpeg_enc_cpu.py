"""The JPEG encoder without a GPU: the reference (tests/jpeg_enc_ref.py) against the committed Pillow bytes, the library's
host half (quant tables, Huffman coder, size bound) against both, the AVI writer with a stub encoder, snapshot naming."""
import os
import struct
import types

import numpy as np
import pytest

from camkifu_amd import capi
from camkifu_amd.core import capture

from . import jpeg_enc_cases as cases
from . import jpeg_enc_ref as ref
from . import jpeg_ref

ALL = cases.all_cases()
IDS = [cases.name_of(c) for c in ALL]


def _stub_encode(frames, quality=90, sampling=ref.S420):
    return [ref.encode(np.asarray(f), quality, sampling) for f in frames]


def _ref_decode(raws):
    return np.stack([jpeg_ref.decode(bytes(r)) for r in raws])


# ---- the reference against Pillow ---------------------------------------------------------------------------------------
def test_the_goldens_are_complete():
    assert len(cases.goldens()) == len(ALL) + len(cases.BATCH)
    assert len(cases.forward_cases()) == 9 * 4 * 4


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_reference_equals_pillows_bytes(case):
    assert cases.ref_encode(case)[0] == cases.golden(case)


def test_reference_equals_pillows_bytes_on_the_batch():
    for seed, case in enumerate(cases.BATCH):
        assert cases.ref_encode(case, seed)[0] == cases.golden(case, seed)


def test_reference_coefficients_are_what_the_decoder_reads_back():
    for case in ALL[::7]:
        info, coef, quant = jpeg_ref.coefficients(cases.golden(case))
        assert np.array_equal(coef, cases.ref_forward(case)), cases.name_of(case)
        assert info["restart_interval"] == case[5]


def test_the_cases_take_every_path_of_the_coder():
    """the reference counts what it codes: each path the issue names is taken by a named case"""
    st = {cases.name_of(c): cases.ref_encode(c)[1] for c in cases.EXTRA}
    assert st["noise_48x64_420_q90_r1"]["restarts"] == 11                      # RSTn wraps behind RST7
    assert st["ramp_48x64_420_q90_r3"]["restarts"] == 3 and st["noise_48x64_422_q50_r7"]["restarts"] == 3
    assert st["noise_80x24_444_q90_r3"]["restarts"] == 9 and st["ramp_80x24_grey_q50_r3"]["restarts"] == 9    # one per MCU row
    assert st["noise_48x64_444_q100_r0"]["stuffed"] > 0 and st["fine_33x70_444_q100_r7"]["stuffed"] > 0
    assert st["noise_48x64_422_q50_r7"]["zrl"] > 0
    assert st["fine_16x32_444_q100_r0"]["no_eob"] > 0 and st["fine_16x32_444_q100_r0"]["eob"] == 0
    assert st["checker_16x32_444_q100_r0"]["max_dc_size"] == 11 and st["checker_32x32_420_q100_r0"]["max_dc_size"] == 11
    assert st["fine_16x32_444_q100_r0"]["max_ac_size"] == 10 and st["fine_24x24_grey_q100_r0"]["max_ac_size"] == 10
    # and the streams of the restart cases hold the markers in cyclic order
    data = cases.golden(("noise", 48, 64, ref.S420, 90, 1))
    scan = data[jpeg_ref.parse(data).scan_at:]
    marks = [scan[i + 1] - 0xD0 for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [k & 7 for k in range(11)]


def test_fresh_pillow_output_on_random_sizes():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(20)
    for k in range(40):
        h, w = int(rng.integers(1, 121)), int(rng.integers(1, 201))
        s, q = cases.SAMPLINGS[k % 4], int(rng.integers(1, 101))
        ri = int(rng.integers(0, 8)) if k % 3 == 0 else 0
        img = cases.image(cases.CONTENTS[(k // 4) % 4], h, w, seed=k)
        assert ref.encode(img, q, s, ri) == cases.pillow_encode(img, q, s, ri), (h, w, s, q, ri)


# ---- the library's host half ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 2, 49, 50, 51, 99, 100])
def test_quant_tables_equal_the_goldens(q):
    case = next(c for c in ALL if c[4] == q and c[3] != ref.GREY)
    _, _, quant = jpeg_ref.coefficients(cases.golden(case))
    got = capi.jpeg_quant(q)
    assert got.dtype == np.uint16 and got.shape == (3, 64)
    assert np.array_equal(got, quant) and np.array_equal(got, ref.quant_tables(q))


def test_quality_is_clamped():
    assert np.array_equal(capi.jpeg_quant(0), capi.jpeg_quant(1)) and np.array_equal(capi.jpeg_quant(-5), capi.jpeg_quant(1))
    assert np.array_equal(capi.jpeg_quant(1000), capi.jpeg_quant(100))
    for q in range(1, 101):
        assert np.array_equal(capi.jpeg_quant(q), ref.quant_tables(q)), q


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_entropy_encode_gives_the_goldens_bytes(case):
    data = cases.golden(case)
    info, coef, quant = jpeg_ref.coefficients(data)
    out = capi.jpeg_entropy_encode(coef, capi.jpeg_quant(case[4]), case[1], case[2], case[3], case[5])
    assert out == data
    assert len(out) <= capi.jpeg_encode_bound(case[1], case[2], case[3])


def test_entropy_encode_of_a_batch_runs_frames_in_parallel():
    case = cases.BATCH[0]
    coef = np.stack([cases.ref_forward(case, s) for s in range(5)])
    out = capi.jpeg_entropy_encode(coef, capi.jpeg_quant(case[4]), case[1], case[2], case[3])
    assert out == [cases.golden(case, s) for s in range(5)]


def test_size_bound_holds_and_is_reached_within_a_factor():
    """worst-case blocks: every AC value has 10 bits behind a 16-bit code (symbol 0x0A of both tables), 26 bits per
    coefficient.  The bound doubles that for byte stuffing, which only a stream of FF bytes alone would need: the worst
    case reaches the bound within a factor of 2.1."""
    for s in cases.SAMPLINGS:
        h, w = 48, 64
        bound = capi.jpeg_encode_bound(h, w, s)
        assert bound == ref.size_bound(h, w, s)
        coef = np.where(np.arange(capi.jpeg_blocks(h, w, s) * 64) & 1, 1023, -1023).astype(np.int16)
        for ri in (0, 1):
            out = capi.jpeg_entropy_encode(coef, capi.jpeg_quant(100), h, w, s, ri)
            assert out == ref.entropy_encode(coef, ref.quant_tables(100), h, w, s, ri)
            assert len(out) <= bound and len(out) * 2.1 >= bound, (s, len(out), bound)
    assert capi.jpeg_encode_bound(1, 1, ref.GREY) == ref.size_bound(1, 1, ref.GREY)


def test_entropy_encode_refuses_what_baseline_cannot_code():
    h, w, s = 16, 16, ref.S444
    q = capi.jpeg_quant(90)
    nb = capi.jpeg_blocks(h, w, s) * 64
    for coef, what in ((np.full(nb, 32767, np.int16), "DC difference"), (np.full(nb, -32767, np.int16), "DC difference")):
        with pytest.raises(capi.CkError, match=what) as e:
            capi.jpeg_entropy_encode(coef, q, h, w, s)
        assert e.value.code == capi.CK_ERR_ARG
    coef = np.zeros(nb, np.int16)
    coef[5] = 1024
    with pytest.raises(capi.CkError, match="AC value of 11 bits"):
        capi.jpeg_entropy_encode(coef, q, h, w, s)
    coef[5] = 0
    with pytest.raises(capi.CkError, match="restart interval"):
        capi.jpeg_entropy_encode(coef, q, h, w, s, 65536)
    with pytest.raises(capi.CkError, match="sampling"):
        capi.jpeg_entropy_encode(coef, q, h, w, 7)
    with pytest.raises(capi.CkError, match="coef"):
        capi.jpeg_entropy_encode(coef[:-64], q, h, w, s)
    bad = q.copy()
    bad[1, 3] = 0
    with pytest.raises(capi.CkError, match="quant entry"):
        capi.jpeg_entropy_encode(coef, bad, h, w, s)
    with pytest.raises(capi.CkError, match="frame size"):
        capi.jpeg_encode_bound(0, 5, s)
    with pytest.raises(capi.CkError, match="frame size"):
        capi.jpeg_encode_bound(5, 65536, s)


def test_entropy_encode_refuses_a_buffer_below_the_bound():
    import ctypes as C
    h, w, s = 16, 16, ref.S444
    q = capi.jpeg_quant(90)
    coef = np.zeros(capi.jpeg_blocks(h, w, s) * 64, np.int16)
    bound = capi.jpeg_encode_bound(h, w, s)
    out = np.zeros(bound, np.uint8)
    ln = (C.c_size_t * 1)()
    rc = capi.lib().ck_jpeg_entropy_encode(coef.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), 1, h, w, s, 0,
                                           out.ctypes.data_as(C.c_void_p), bound - 1, ln)
    assert rc == capi.CK_ERR_ARG and b"smaller than the bound" in capi.lib().ck_last_error(None)
    assert not out.any()


# ---- the AVI writer -------------------------------------------------------------------------------------------------------
def _film(n, h=24, w=40):
    return np.stack([cases.image(cases.CONTENTS[k % 4], h, w, seed=k) for k in range(n)])


def test_mjpeg_writer_reads_back(tmp_path):
    frames = _film(7)
    path = str(tmp_path / "film.avi")
    with capture.MjpegWriter(path, 24, 40, fps=25, quality=80, sampling=ref.S422, encode=_stub_encode) as wr:
        assert wr.write(frames[:3]) == 3
        assert wr.write(frames[3]) == 1                                  # a single frame
        assert wr.write(frames[4:4]) == 0
        assert wr.write(frames[4:]) == 3
    streams = _stub_encode(frames, 80, ref.S422)
    with open(path, "rb") as f:
        buf = f.read()
    idx = jpeg_ref.avi_index(buf)
    assert (idx["h"], idx["w"], idx["fps"]) == (24, 40, 25.0) and idx["chunks"] == streams
    cap = capture.AviMjpegCapture(path, decode=_ref_decode)
    assert cap.isOpened() and len(cap) == 7 and cap.damaged == 0 and cap.get(capture.CAP_PROP_FPS) == 25.0
    for k in range(7):
        ok, img = cap.read()
        assert ok and np.array_equal(img, jpeg_ref.decode(streams[k]))
    # sizes: RIFF spans the file, movi its chunks, avih / strh count the frames, idx1 points at every chunk
    assert struct.unpack("<I", buf[4:8])[0] == len(buf) - 8
    movi = buf.index(b"movi")
    movi_len = struct.unpack("<I", buf[movi - 4:movi])[0]
    idx1 = movi + movi_len
    assert buf[idx1:idx1 + 4] == b"idx1" and struct.unpack("<I", buf[idx1 + 4:idx1 + 8])[0] == 16 * 7
    assert idx1 + 8 + 16 * 7 == len(buf)
    avih = buf.index(b"avih")
    assert struct.unpack("<I", buf[avih + 8 + 16:avih + 8 + 20])[0] == 7            # dwTotalFrames
    assert struct.unpack("<I", buf[avih + 8 + 12:avih + 8 + 16])[0] & 0x10           # AVIF_HASINDEX
    strh = buf.index(b"strh")
    assert struct.unpack("<I", buf[strh + 8 + 32:strh + 8 + 36])[0] == 7            # dwLength
    assert struct.unpack("<I", buf[strh + 8 + 36:strh + 8 + 40])[0] == max(len(s) for s in streams)
    for k in range(7):
        cc, flags, off, ln = struct.unpack("<4sIII", buf[idx1 + 8 + 16 * k:idx1 + 24 + 16 * k])
        assert cc == b"00dc" and flags == 0x10 and ln == len(streams[k])
        assert buf[movi + off:movi + off + 8] == b"00dc" + struct.pack("<I", ln)
        assert buf[movi + off + 8:movi + off + 8 + ln] == streams[k]
        assert (movi + off) % 2 == 0


def test_mjpeg_writer_of_no_frames_is_a_valid_file(tmp_path):
    path = str(tmp_path / "empty.avi")
    capture.MjpegWriter(path, 24, 40, encode=_stub_encode).close()
    with open(path, "rb") as f:
        buf = f.read()
    assert struct.unpack("<I", buf[4:8])[0] == len(buf) - 8 and jpeg_ref.avi_index(buf)["chunks"] == []
    cap = capture.AviMjpegCapture(path, decode=_ref_decode)
    assert cap.isOpened() and len(cap) == 0 and (cap.w, cap.h) == (40, 24) and cap.read() == (False, None)


def test_mjpeg_writer_refuses_what_the_reader_cannot_read_back(tmp_path):
    class Big:                                      # a stream that only reports a size
        def __len__(self):
            return 600 << 20

    path = str(tmp_path / "big.avi")
    wr = capture.MjpegWriter(path, 24, 40, encode=lambda frames, quality, sampling: [Big() for _ in frames])
    with pytest.raises(capture.AviError, match="1 GiB"):
        wr.write(_film(2))
    assert wr.frames == 0 and os.path.getsize(path) < 4096          # nothing of the batch was written
    wr.encode = _stub_encode
    wr.write(_film(2))
    wr.close()
    wr.close()                                                       # (closing twice is harmless)
    with pytest.raises(capture.AviError, match="closed"):
        wr.write(_film(1))
    assert len(capture.AviMjpegCapture(path, decode=_ref_decode)) == 2
    with pytest.raises(ValueError, match="frames of"):
        with capture.MjpegWriter(str(tmp_path / "other.avi"), 24, 40, encode=_stub_encode) as w2:
            w2.write(_film(1, 24, 48))


def test_write_jpeg_with_a_stub(tmp_path):
    img = cases.image("ramp", 17, 33)
    path = str(tmp_path / "still.jpg")
    n = capture.write_jpeg(path, img, quality=70, encode=_stub_encode)
    with open(path, "rb") as f:
        data = f.read()
    assert n == len(data) and data == ref.encode(img, 70, ref.S420)
    with pytest.raises(ValueError):
        capture.write_jpeg(path, img[None], encode=_stub_encode)


# ---- snapshots --------------------------------------------------------------------------------------------------------------
def test_jpg_snapshots_are_numbered_with_the_npy_ones(tmp_path, monkeypatch):
    from camkifu_amd import cvconf
    from camkifu_amd.core.vmanager import VManagerBase
    from camkifu_amd.golib_shim import Kifu, Move, NP_TYPE, B
    from camkifu_amd.controller import ControllerHeadless
    monkeypatch.setattr(cvconf, "snapshot_dir", str(tmp_path))
    ctrl = ControllerHeadless()
    ctrl.pipe("append", Move(NP_TYPE, (B, 3, 3)))
    vm = VManagerBase(ctrl, bf="None", sf="None")
    assert vm.snapshot(True, fmt="jpg", encode=_stub_encode) is None
    img = cases.image("ramp", 380, 380)
    vm.stones_finder = types.SimpleNamespace(goban_img=img)
    assert vm.snapshot(True) == str(tmp_path / "snapshot-0.npy")
    assert vm.snapshot(True, fmt="jpg", encode=_stub_encode) == str(tmp_path / "snapshot-1.jpg")
    assert (tmp_path / "game-0.sgf").exists() and (tmp_path / "game-1.sgf").exists()
    assert Kifu(str(tmp_path / "game-1.sgf")).moves == [Move(NP_TYPE, (B, 3, 3))]
    assert vm.snapshot() == str(tmp_path / "snapshot-2.npy")
    vm.stones_finder.goban_img = img[None]                    # a batch of one, as the warp returns it
    assert vm.snapshot(fmt="jpg", encode=_stub_encode) == str(tmp_path / "snapshot-3.jpg") and not (tmp_path / "game-3.sgf").exists()
    with open(tmp_path / "snapshot-1.jpg", "rb") as f:
        data = f.read()
    assert data == ref.encode(img, 95, ref.S444)              # quality 95, 4:4:4
    assert data == open(tmp_path / "snapshot-3.jpg", "rb").read()
    with pytest.raises(ValueError, match="npy or jpg"):
        vm.snapshot(fmt="png")

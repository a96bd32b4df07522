"""The host half of the PNG reader and writer against tests/png_ref.py and zlib: capi.png_inflate (the library's own inflate,
whose verdict has to be zlib's), capi.png_probe (the chunk walk and its refusals) and capi.png_encode_staged (the steps the GPU
kernels run, in plain loops).  No GPU."""
import io
import os
import struct
import zlib

import numpy as np
import pytest

from camkifu_amd import capi

from . import png_cases, png_ref


def _verdict(fn, data):
    try:
        return fn(data)
    except (zlib.error, capi.CkError):
        return None


@pytest.mark.parametrize("name", sorted(png_cases.inflate_streams()))
def test_inflate_equals_zlib(name):
    z, payload = png_cases.inflate_streams()[name]
    assert zlib.decompress(z) == payload                   # (the case is what it says)
    assert capi.png_inflate(z) == payload


def test_inflate_cases_hold_what_their_names_say():
    """every stream really holds the construct it is named for: png_cases.trace walks the blocks with a decoder of its own and
    reports block types, the longest match, the farthest distance and whether a code-length repeat spans the boundary"""
    S = png_cases.inflate_streams()
    traces = {k: png_cases.trace(z) for k, (z, _) in S.items()}
    for k, (z, payload) in S.items():
        assert traces[k]["payload"] == payload, k           # (the walker reads the stream right)
    assert traces["empty stored block"]["types"] == [0] and S["empty stored block"][1] == b""
    assert {0, 1, 2} <= set(traces["stored, fixed and dynamic blocks"]["types"])
    assert traces["a match of length 258"]["max_length"] == 258
    far = traces["a match at distance 32768"]
    assert far["max_distance"] == 32768 and far["max_length"] == 258 and far["distance_symbols"] == {28, 29}
    assert traces["repeats across the boundary"]["repeats_span"] and traces["repeats across the boundary"]["types"] == [2]
    assert traces["zeros across the boundary"]["repeats_span"]
    small = {k: png_cases.trace(z) for k, z in png_cases.small_streams().items()}
    assert [small[k]["types"][0] for k in ("stored", "fixed", "dynamic, literals only")] == [0, 1, 2]
    assert small["dynamic, literals only"]["max_length"] == 0 and small["dynamic, runs"]["max_distance"] == 1
    assert small["dynamic, matches"]["max_distance"] > 1


@pytest.mark.parametrize("name", sorted(png_cases.small_streams()))
def test_inflate_verdict_is_zlibs_on_every_truncation_and_mutation(name):
    z = png_cases.small_streams()[name]
    assert len(z) <= 620
    assert capi.png_inflate(z) == zlib.decompress(z)
    for cut in range(len(z)):
        assert _verdict(capi.png_inflate, z[:cut]) == _verdict(zlib.decompress, z[:cut]), "cut at %d" % cut
    refused = 0
    for at in range(len(z)):
        for x in (0x01, 0x80, 0xFF):
            m = bytearray(z)
            m[at] ^= x
            want = _verdict(zlib.decompress, bytes(m))
            assert _verdict(capi.png_inflate, bytes(m)) == want, "byte %d xor %#x" % (at, x)
            refused += want is None
    assert refused > len(z)                                 # (most damage is noticed: the test compares refusals too)


def test_inflate_ignores_what_follows_the_stream_and_reports_the_size_beyond_the_room():
    z, payload = png_cases.inflate_streams()["a match at distance 32768"]
    assert capi.png_inflate(z + b"trailing") == payload
    import ctypes as C
    buf = np.frombuffer(z, np.uint8)
    assert zlib.decompress(z) == payload and len(payload) == 32768 + 258 + 3 + 100 + 12 + 25
    # the stream's matches reach back 32768, 24577 and 24576 bytes.  cap 0 .. 100: every match copies from bytes that found no
    # room to bytes that find none, the first ones over the whole window; 32768: from kept bytes to dropped ones; 32768 + 100
    # and + 259: a match runs across the end of the room; 33000: matches read kept bytes and dropped ones
    for cap in (0, 1, 100, 24577, 32767, 32768, 32769, 32768 + 100, 32768 + 258, 32768 + 259, 33000, len(payload) - 1, len(payload)):
        out, total = np.full(cap + 8, 0xAB, np.uint8), C.c_size_t(0)
        rc = capi.lib().ck_png_inflate(C.c_void_p(buf.ctypes.data), buf.size, out.ctypes.data_as(C.c_void_p), cap, C.byref(total))
        assert rc == 0 and total.value == len(payload)      # (the Adler-32 covers the bytes that found no room, too)
        assert out[:cap].tobytes() == payload[:cap] and (out[cap:] == 0xAB).all()


# ---- the chunk walk ----
def _good():
    return png_cases.image(5, 4, 2, 8, flavour="fixed")[0]


def _rechunk(data, edit):
    """the file with its chunk list [(kind, body)] passed through `edit`, CRCs made afresh"""
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        chunks.append((kind, data[at + 8:at + 8 + n]))
        at += 12 + n
    return png_ref.SIG + b"".join(png_ref.chunk(k, b) for k, b in edit(chunks))


def _ihdr(**kw):
    def edit(chunks):
        f = dict(zip(("w", "h", "depth", "ct", "comp", "flt", "lace"), struct.unpack(">IIBBBBB", chunks[0][1])))
        f.update(kw)
        return [(b"IHDR", struct.pack(">IIBBBBB", *[f[k] for k in ("w", "h", "depth", "ct", "comp", "flt", "lace")]))] + chunks[1:]
    return _rechunk(_good(), edit)


def _idat(payload):
    return _rechunk(_good(), lambda chunks: [(k, zlib.compress(payload) if k == b"IDAT" else b) for k, b in chunks])


REFUSALS = {
    "a bad signature": (lambda: b"\x89PNG\r\n\x1a\r" + _good()[8:], "signature"),
    "a bad CRC": (lambda: _good()[:40] + bytes([_good()[40] ^ 1]) + _good()[41:], "CRC"),
    "a missing IHDR": (lambda: _rechunk(_good(), lambda chunks: chunks[1:]), "IHDR"),
    "Adam7": (lambda: _ihdr(lace=1), "Adam7"),
    "zero width": (lambda: _ihdr(w=0), "zero width"),
    "depth 3": (lambda: _ihdr(depth=3), "bit depth 3"),
    "colour type 5": (lambda: _ihdr(ct=5), "colour type 5"),
    "a filter byte of 5": (lambda: _idat(bytes([0] * 16 + [5] + [0] * 15 + [0] * 32)), "filter type 5"),
    "short IDAT data": (lambda: _idat(bytes(16 * 4 - 1)), "too short"),
    "an unknown critical chunk": (lambda: _rechunk(_good(), lambda c: c[:1] + [(b"ABCD", b"x")] + c[1:]), "critical chunk ABCD"),
    "IDAT chunks with another chunk between them": (lambda: _rechunk(png_cases.image(5, 4, 2, 8, idat_split=9)[0],
                                                                   lambda c: c[:2] + [(b"tEXt", b"k\0v")] + c[2:]), "not consecutive"),
    "a second PLTE": (lambda: _rechunk(png_cases.image(5, 4, 3, 8)[0], lambda c: c[:2] + [c[1]] + c[2:]), "second PLTE"),
    "PLTE behind IDAT": (lambda: _rechunk(png_cases.image(5, 4, 3, 8)[0], lambda c: [c[0], c[2], c[1]] + c[3:]), "PLTE"),
    "a damaged zlib stream": (lambda: _rechunk(_good(), lambda c: [(k, b[:-1] + bytes([b[-1] ^ 1]) if k == b"IDAT" else b) for k, b in c]), "Adler"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_probe_refuses_with_the_cause(name):
    make, cause = REFUSALS[name]
    with pytest.raises(capi.CkError, match=cause) as e:
        capi.png_probe(make())
    assert e.value.code == capi.CK_ERR_DATA


def test_probe_reads_what_the_standard_allows():
    for ct, depth in png_cases.TYPES:
        data, _ = png_cases.image(5, 3, ct, depth, flavour="stored")
        info = capi.png_probe(data)
        assert (info["h"], info["w"], info["color_type"], info["bit_depth"]) == (3, 5, ct, depth)
        assert info["rowbytes"] == png_ref.rowbytes(5, ct, depth)
    # ancillary chunks are skipped, tRNS among them; several IDAT chunks are joined; bytes beyond the last row are ignored
    extra = (png_ref.chunk(b"gAMA", struct.pack(">I", 45455)), png_ref.chunk(b"tRNS", b"\x00\x01\x00\x02\x00\x03"))
    data, _ = png_cases.image(9, 7, 2, 8, idat_split=5, extra=extra)
    assert capi.png_probe(data)["w"] == 9 and capi.png_header(data)["h"] == 7
    # libpng's leniencies: a PLTE in a grey image is passed over, palette entries beyond 2^depth are dropped
    grey = _rechunk(png_cases.image(5, 3, 0, 8)[0], lambda c: c[:1] + [(b"PLTE", bytes(30))] + c[1:])
    assert capi.png_probe(grey)["palette_entries"] == 0
    assert capi.png_probe(png_cases.image(5, 3, 3, 2, plte_n=7)[0])["palette_entries"] == 4
    assert capi.png_probe(png_cases.image(5, 3, 3, 2, plte_n=3)[0])["palette_entries"] == 3
    long = _idat(bytes(16 * 4 + 9))
    assert capi.png_probe(long)["h"] == 4
    for name, (data, _) in png_cases.golden().items():
        assert capi.png_probe(data)["h"] == 29, name


# ---- the staged encoder ----
def _fibonacci_band(w=400, h=16):
    """one band whose symbols occur with Fibonacci counts: the end-of-block symbol once, 18 byte values 1, 2, 3, 5 .. 4181
    times, and value 0 -- the filter bytes of filter None among them -- for the rest of a 16-row band of 1 + 3w bytes a row,
    above 6765 times: every merge of the Huffman build takes the tree so far and the next symbol, 19 levels deep"""
    fib = [1, 2]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    assert fib[-1] == 4181 and 3 * w * h - sum(fib) + h > 6765
    vals = np.concatenate([np.full(c, 1 + i, np.uint8) for i, c in enumerate(fib)])
    flat = np.concatenate([vals, np.zeros(3 * w * h - len(vals), np.uint8)])
    return np.ascontiguousarray(np.random.RandomState(3).permutation(flat).reshape(h, w, 3)[:, :, ::-1])


def _huffman_depth(counts):
    """the longest code of a plain Huffman tree over the counts"""
    import heapq
    heap = [(c, i, 0) for i, c in enumerate(counts) if c]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], k, max(a[2], b[2]) + 1))
        k += 1
    return heap[0][2]


SHAPES = [(1, 1), (1, 17), (17, 1), (15, 6), (16, 6), (17, 6), (33, 5), (5, 341), (5, 342), (20, 40)]


def _image(h, w, seed=0):
    rng = np.random.RandomState(100 * h + w + seed)
    smooth = np.cumsum(rng.randint(-3, 4, (h, w, 3)), 1) + np.cumsum(rng.randint(-3, 4, (h, 1, 3)), 0) + 128
    return np.where(rng.rand(h, w, 1) < 0.8, smooth, rng.randint(0, 256, (h, w, 3))).astype(np.uint8)


def _check_file(data, bgr):
    c = png_ref.walk(data)                                  # (every CRC)
    assert (c["w"], c["h"], c["depth"], c["ct"], c["interlace"]) == (bgr.shape[1], bgr.shape[0], 8, 2, 0)
    assert data.count(b"IDAT") >= 1 and len(zlib.decompress(c["idat"])) == bgr.shape[0] * (1 + 3 * bgr.shape[1])     # (and the Adler-32)
    assert np.array_equal(png_ref.decode(data), bgr)
    try:
        from PIL import Image
    except ImportError:
        return c
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1], bgr)
    return c


@pytest.mark.parametrize("shape", SHAPES)
def test_staged_encoder_round_trips_with_every_filter(shape):
    bgr = _image(*shape)
    raw, picks = png_ref.encoder_rows(bgr)
    for flt in (None, 0, 1, 2, 3, 4):
        data = capi.png_encode_staged(bgr, flt)[0]
        c = _check_file(data, bgr)
        rows = zlib.decompress(c["idat"])
        used = [rows[y * (1 + raw.shape[1])] for y in range(shape[0])]
        assert used == (picks if flt is None else [flt] * shape[0])        # the heuristic, row by row
        assert len(data) <= capi.png_encode_bound(*shape)


def test_staged_encoder_batch_and_arguments():
    frames = np.stack([_image(18, 9, s) for s in range(3)])
    out = capi.png_encode_staged(frames)
    assert len(out) == 3 and all(np.array_equal(png_ref.decode(d), f) for d, f in zip(out, frames))
    assert out == [capi.png_encode_staged(f)[0] for f in frames]
    with pytest.raises(capi.CkError, match="filter"):
        capi.png_encode_staged(frames, 5)
    with pytest.raises(capi.CkError):
        capi.png_encode_staged(frames[:, :, :, :2])


def test_adaptive_filter_halves_a_horizontal_ramp():
    """Sub leaves a constant residual, None leaves 256 equiprobable values"""
    bgr = np.ascontiguousarray(np.broadcast_to((np.arange(768) % 256).astype(np.uint8)[None, :, None], (32, 768, 3)))
    adaptive, plain = capi.png_encode_staged(bgr)[0], capi.png_encode_staged(bgr, 0)[0]
    _check_file(adaptive, bgr)
    assert len(adaptive) < len(plain) / 2, (len(adaptive), len(plain))


def test_a_band_deeper_than_15_bits_is_limited_and_decodes():
    bgr = _fibonacci_band()
    rows = np.concatenate([np.zeros((16, 1), np.uint8), bgr[:, :, ::-1].reshape(16, -1)], 1)
    counts = np.bincount(rows.reshape(-1), minlength=256).tolist() + [1]
    assert _huffman_depth(counts) > 15                      # a plain Huffman code of this band does not fit deflate
    assert capi.png_tiles()["band_rows"] == 16
    data = capi.png_encode_staged(bgr, 0)[0]
    _check_file(data, bgr)


# ---- the users' entry points, with the host encoder and the reference decoder standing in for the GPU ----
def _stub_context():
    import types
    return types.SimpleNamespace(png_encode=lambda frames, filter=None: capi.png_encode_staged(np.asarray(frames), filter),
                                 png_decode=lambda streams: np.stack([png_ref.decode(bytes(s)) for s in streams]),
                                 jpeg_decode=None)


def test_write_png_open_capture_and_png_snapshots(tmp_path, monkeypatch):
    import types
    from camkifu_amd import cvconf
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture
    from camkifu_amd.core.vmanager import VManagerBase
    from camkifu_amd.golib_shim import Move, NP_TYPE, B
    from camkifu_amd.stone import nn_manager as nm
    stub = _stub_context()
    monkeypatch.setattr(capi, "get_context", lambda device=0: stub)
    img = _image(380, 380)
    path = str(tmp_path / "still.PNG")
    assert capture.write_png(path, img[:30, :40], filter=4) == os.path.getsize(path)
    cap = capture.open_capture(path)
    assert isinstance(cap, capture.ImageCapture) and cap.isOpened() and np.array_equal(cap.read()[1], img[:30, :40])
    with pytest.raises(ValueError):
        capture.write_png(path, img[None])
    assert not capture.open_capture(str(tmp_path / "missing.png")).isOpened()
    # snapshots: one counter for .npy, .jpg and .png; the game beside the picture; gen_data reads the picture back
    assert ".png" in nm.SNAPSHOT_SUFFIXES
    monkeypatch.setattr(cvconf, "snapshot_dir", str(tmp_path))
    ctrl = ControllerHeadless()
    ctrl.pipe("append", Move(NP_TYPE, (B, 3, 3)))
    vm = VManagerBase(ctrl, bf="None", sf="None")
    assert vm.snapshot_png(True) is None
    vm.stones_finder = types.SimpleNamespace(goban_img=img[None])
    assert vm.snapshot(True) == str(tmp_path / "snapshot-0.npy")
    assert vm.snapshot_png(True, encode=stub.png_encode) == str(tmp_path / "snapshot-1.png")
    assert vm.snapshot_png() == str(tmp_path / "snapshot-2.png") and not (tmp_path / "game-2.sgf").exists()
    assert vm.snapshot() == str(tmp_path / "snapshot-3.npy")
    assert nm.NNManager.get_ref_game(str(tmp_path / "snapshot-1.png")) == str(tmp_path / "game-1.sgf")
    assert np.array_equal(nm.NNManager.load_snapshot(str(tmp_path / "snapshot-1.png")), img)
    mgr = nm.NNManager()
    x0, y0 = mgr.gen_data(str(tmp_path / "snapshot-0.npy"))
    x1, y1 = mgr.gen_data(str(tmp_path / "snapshot-1.png"))
    assert mgr.stones_source == "sgf" and np.array_equal(x1, x0) and np.array_equal(y1, y0)
    with pytest.raises(ValueError, match="npy, .jpg or .png"):
        nm.NNManager.load_snapshot(str(tmp_path / "snapshot-1.gif"))

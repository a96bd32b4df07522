"""The runs mode of the PNG encoder on the host: capi.png_encode_staged(.., runs=True) against tests/png_runs_ref.py -- the
rule restated in plain Python and an inflate of its own that reports every block's header and tokens -- against zlib,
tests/png_ref.py and Pillow for the pixels, and the default mode's bytes, which must not move.  No GPU."""
import zlib

import numpy as np
import pytest

from camkifu_amd import capi

from . import png_ref, png_runs_ref
from .test_png_cpu import SHAPES, _check_file, _fibonacci_band, _huffman_depth, _image

RUN_LENGTHS = [1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 263, 516, 517, 518, 519, 520]


def _bgr(raw):
    """RGB rows (h, 3w) -> the BGR image whose filter-None rows they are"""
    return np.ascontiguousarray(raw.reshape(raw.shape[0], -1, 3)[:, :, ::-1])


def _noise_rows(h, w):
    """RGB rows (h, 3w) without two equal neighbours and without the values 0 and 7"""
    i = np.arange(h * 3 * w)
    return (8 + (i * 37) % 241 + (i % 2)).astype(np.uint8).reshape(h, 3 * w)


def constructed():
    """name -> BGR image (or a batch of them) whose rows under filter None hold the runs the name says"""
    out = {}
    one = []
    for n in RUN_LENGTHS:                                   # a run of n sevens from byte 100 of a row of 1026 bytes
        raw = _noise_rows(1, 342)
        raw[0, 100:100 + n] = 7
        one.append(_bgr(raw))
    out["runs of every length in one row"] = np.stack(one)
    out["zeros 35x50"] = np.zeros((35, 50, 3), np.uint8)    # one run a band: through the filter bytes, rows and the seam at byte 1024
    out["zeros 17x6"] = np.zeros((17, 6, 3), np.uint8)      # the second band has one row; its first byte is a literal
    raw = _noise_rows(5, 341)                               # a row is exactly one tile
    raw[0, -40:] = 7                                        # ends on the last byte of tile 0
    raw[1, :30] = 0                                         # starts, with the filter byte, on the first byte of tile 1
    raw[2, -50:] = 0                                        # the end of tile 2, all of tile 3, the start of tile 4
    raw[3] = 0
    raw[4, :60] = 0
    out["tile edges 5x341"] = _bgr(raw)
    # the Fibonacci band of test_png_cpu with zeros behind every row.  Its values lie in random order, so equal neighbours
    # become runs and the token counts are no Fibonacci numbers any more: the plain Huffman code of this one is 14 deep
    fib = _fibonacci_band()
    out["fibonacci band and a zero run"] = np.concatenate([fib, np.zeros((16, 120, 3), np.uint8)], 1)
    # so Fibonacci counts once more with a zero between any two values -- no run but the one appended, every value a
    # literal as often as it occurs -- and 678 zeros behind them, a run of 1 + 258 + 258 + 162: the end-of-block symbol and
    # the match of 162 once, the match of 258 twice, then the values 3, 5, 8 .. 4181 times: deeper than 15 bits
    counts = [3, 5]
    while len(counts) < 16:
        counts.append(counts[-1] + counts[-2])
    vals = np.random.RandomState(5).permutation(np.concatenate([np.full(c, 1 + i, np.uint8) for i, c in enumerate(counts)]))
    raw = np.zeros(16 * 3 * 470, np.uint8)
    raw[0:2 * len(vals):2] = vals
    out["fibonacci literals and a zero run"] = _bgr(raw.reshape(16, -1))
    return out


def _bands(idat, h, w):
    rows = zlib.decompress(idat)
    assert len(rows) == h * (1 + 3 * w)
    step = 16 * (1 + 3 * w)
    return [rows[i:i + step] for i in range(0, len(rows), step)]


def check_runs_file(data, bgr):
    """a file of the runs mode: its blocks hold the tokens of the rule, band by band; the pixels come back; the bound holds"""
    h, w = bgr.shape[:2]
    c = _check_file(data, bgr)
    bands, blocks = _bands(c["idat"], h, w), png_runs_ref.trace(c["idat"])
    assert len(blocks) == len(bands) == -(-h // 16)
    for band, blk in zip(bands, blocks):
        assert (blk["hlit"], blk["hdist"], blk["dist_lens"]) == (29, 1, [1, 1])
        assert len(blk["lit_lens"]) == 286 and max(blk["lit_lens"]) <= 15
        assert blk["tokens"] == png_runs_ref.tokens(band)
    assert len(data) <= capi.png_encode_bound(h, w)
    return bands


def test_the_rule_itself():
    T = png_runs_ref.tokens
    assert T(b"") == [] and T(b"a") == [("L", 97)] and T(b"aa") == [("L", 97)] * 2 and T(b"aaa") == [("L", 97)] * 3
    assert T(b"aaaa") == [("L", 97), ("M", 3)]
    assert T(bytes(259)) == [("L", 0), ("M", 258)] and T(bytes(260)) == [("L", 0), ("M", 258), ("L", 0)]
    assert T(bytes(262)) == [("L", 0), ("M", 258), ("M", 3)] and T(bytes(517)) == [("L", 0), ("M", 258), ("M", 258)]
    assert T(b"ab" + bytes(5) + b"b") == [("L", 97), ("L", 98), ("L", 0), ("M", 4), ("L", 98)]
    # zlib's own Z_RLE streams pass the walker: it reads matches, extra bits and both codes right
    data = bytes(1000) + bytes(range(256)) * 3 + b"\x05" * 300
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    blocks = png_runs_ref.trace(co.compress(data) + co.flush())
    assert sum(1 if k == "L" else v for b in blocks for k, v in b["tokens"]) == len(data)


@pytest.mark.parametrize("shape", SHAPES)
def test_tokens_of_every_shape_and_filter(shape):
    bgr = _image(*shape)
    for flt in (None, 0, 4):
        check_runs_file(capi.png_encode_staged(bgr, flt, runs=True)[0], bgr)


@pytest.mark.parametrize("name", sorted(constructed()))
def test_tokens_of_constructed_images(name):
    frames = constructed()[name]
    frames = frames if frames.ndim == 4 else frames[None]
    for flt in (None, 0, 4):
        out = capi.png_encode_staged(frames, flt, runs=True)
        for f, (data, bgr) in enumerate(zip(out, frames)):
            bands = check_runs_file(data, bgr)
            if flt != 0:
                continue
            toks = [t for b in bands for t in png_runs_ref.tokens(b)]
            if name == "runs of every length in one row":   # (the cases are what their names say)
                k, t = divmod(RUN_LENGTHS[f] - 1, 258)
                want = [("L", 7)] + [("M", 258)] * k + ([("M", t)] if t >= 3 else [("L", 7)] * t)
                at = toks.index(("L", 7))
                assert toks[at:at + len(want)] == want and ("L", 7) not in toks[at + len(want):]
                assert sum(kind == "M" for kind, _ in toks) == k + (t >= 3)
            elif name == "zeros 35x50":                     # 16 rows of 151 zeros: 1 + 9 * 258 + 93; the last band has 3 rows
                assert toks[:11] == [("L", 0)] + [("M", 258)] * 9 + [("M", 93)] and len(toks) == 11 + 11 + 1 + 1 + 1
            elif name == "zeros 17x6":
                assert toks == [("L", 0), ("M", 258), ("M", 45), ("L", 0), ("M", 18)]
            elif name == "tile edges 5x341":
                assert toks.count(("M", 39)) == 1 and toks.count(("M", 30)) == 1 and ("M", 258) in toks
                assert sum(v for k, v in toks if k == "M" and v != 39 and v != 30) == 50 + 1024 + 61 - 1
            elif name == "fibonacci literals and a zero run":
                syms = [v if k == "L" else 257 + max(i for i, b in enumerate(png_runs_ref.LEN_BASE) if b <= v) for k, v in toks]
                hist = np.bincount(syms + [256], minlength=286).tolist()
                assert sum(hist[257:]) > 0 and _huffman_depth(hist) > 15       # deeper than deflate allows, length symbols present
                assert max(png_runs_ref.trace(png_ref.walk(data)["idat"])[0]["lit_lens"]) == 15


@pytest.mark.parametrize("shape", SHAPES)
def test_the_default_mode_is_untouched(shape):
    bgr = _image(*shape)
    for flt in (None, 0, 4):
        plain = capi.png_encode_staged(bgr, flt)
        assert plain == capi.png_encode_staged(bgr, flt, runs=False) == capi.png_encode_staged(bgr, flt, runs=capi.CK_PNG_MATCH_NONE)
        assert plain != capi.png_encode_staged(bgr, flt, runs=True)     # (another header, whatever the tokens)


def test_a_flat_image_shrinks():
    zero = np.zeros((64, 64, 3), np.uint8)
    runs, plain = capi.png_encode_staged(zero, runs=True)[0], capi.png_encode_staged(zero)[0]
    assert len(runs) < len(plain), (len(runs), len(plain))
    bands = check_runs_file(runs, zero)
    blocks = png_runs_ref.trace(png_ref.walk(runs)["idat"])
    assert sum(len(b["tokens"]) for b in blocks) == sum(png_runs_ref.counts(bands)) == 4 * (1 + 12)       # 16 * 193 = 1 + 11 * 258 + 249


def test_a_bad_mode_is_refused():
    x = _image(5, 7)
    for bad in (2, -1, 7):
        with pytest.raises(capi.CkError, match="match mode %d" % bad) as e:
            capi.png_encode_staged(x, runs=bad)
        assert e.value.code == capi.CK_ERR_ARG
    assert capi.png_encode_staged(x, runs=capi.CK_PNG_MATCH_RUNS) == capi.png_encode_staged(x, runs=True)
    for bad in (None, "runs", 1.0):                          # (the context's setting is no answer for a call without a context)
        with pytest.raises(capi.CkError, match="png runs"):
            capi.png_encode_staged(x, runs=bad)


def test_write_png_and_snapshot_png_hand_the_keyword_on_only_when_asked(tmp_path, monkeypatch):
    import types
    from camkifu_amd import cvconf
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture
    from camkifu_amd.core.vmanager import VManagerBase
    seen = []

    def encode(frames, filter=None, **kw):
        seen.append(dict(kw))
        return capi.png_encode_staged(np.asarray(frames), filter, **kw)

    img = np.zeros((40, 30, 3), np.uint8)
    img[5:9, 3:20] = (10, 200, 30)
    p = str(tmp_path / "a.png")
    n_plain = capture.write_png(p, img, encode=encode)
    n_runs = capture.write_png(p, img, encode=encode, runs=True)
    assert seen == [{}, {"runs": True}] and n_runs < n_plain
    with open(p, "rb") as f:
        assert np.array_equal(png_ref.decode(f.read()), img)
    capture.write_png(p, img, encode=encode, runs=False)
    assert seen[-1] == {"runs": False}
    monkeypatch.setattr(cvconf, "snapshot_dir", str(tmp_path))
    assert cvconf.png_runs is False
    vm = VManagerBase(ControllerHeadless(), bf="None", sf="None")
    vm.stones_finder = types.SimpleNamespace(goban_img=img)
    del seen[:]
    vm.snapshot_png(encode=encode)
    vm.snapshot_png(encode=encode, runs=True)
    monkeypatch.setattr(cvconf, "png_runs", True)
    path = vm.snapshot_png(encode=encode)
    assert seen == [{}, {"runs": True}, {"runs": True}]
    with open(path, "rb") as f:
        assert np.array_equal(png_ref.decode(f.read()), img)

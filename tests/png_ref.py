"""A plain restatement of PNG for the tests: a chunk walker, zlib.decompress, a bytewise unfilter, the expansion to BGR that
cv2.imread's default mode performs, libpng's filter heuristic, and a small writer that forces a filter type per row and a
deflate flavour.  Shares no code with the library."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
FLAVOURS = ("stored", "fixed", "huffman", "rle", "best")


def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def walk(data):
    """-> dict(w, h, depth, ct, interlace, plte, idat): every CRC checked, IHDR first, IEND last"""
    assert data[:8] == SIG, "signature"
    at, out, first = 8, dict(plte=b"", idat=b""), True
    while True:
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert len(body) == n, "chunk runs past the end"
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff, "CRC of %r" % kind
        assert first == (kind == b"IHDR"), "IHDR first"
        first = False
        if kind == b"IHDR":
            out["w"], out["h"], out["depth"], out["ct"], comp, flt, out["interlace"] = struct.unpack(">IIBBBBB", body)
            assert comp == 0 and flt == 0
        elif kind == b"PLTE":
            out["plte"] = body
        elif kind == b"IDAT":
            out["idat"] += body
        elif kind == b"IEND":
            return out
        at += 12 + n


def rowbytes(w, ct, depth):
    return (w * CHANNELS[ct] * depth + 7) // 8


def filter_unit(ct, depth):
    return max(1, CHANNELS[ct] * depth // 8)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def predict(ft, a, b, c):
    return (0, a, b, (a + b) // 2, paeth(a, b, c))[ft]


def unfilter(inflated, h, rb, bpp):
    """filtered rows (h * (1 + rb) bytes) -> raw rows (h, rb) uint8, byte by byte"""
    out = np.zeros((h, rb), np.uint8)
    prev = [0] * rb
    for y in range(h):
        ft = inflated[y * (rb + 1)]
        assert ft <= 4, "filter byte %d" % ft
        src = inflated[y * (rb + 1) + 1:(y + 1) * (rb + 1)]
        cur = [0] * rb
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            c = prev[i - bpp] if i >= bpp else 0
            cur[i] = (src[i] + predict(ft, a, prev[i], c)) & 255
        out[y] = cur
        prev = cur
    return out


def filter_row(ft, cur, prev, bpp):
    """raw row and the raw row above (lists of ints; zeros above the first) -> the filtered bytes"""
    return bytes((cur[i] - predict(ft, cur[i - bpp] if i >= bpp else 0, prev[i], prev[i - bpp] if i >= bpp else 0)) & 255
                 for i in range(len(cur)))


def heuristic(cur, prev, bpp):
    """libpng's choice: the filter whose residuals, read as signed bytes, have the least sum of absolute values; the lowest
    number among equals"""
    sums = [sum(v if v < 128 else 256 - v for v in filter_row(ft, cur, prev, bpp)) for ft in range(5)]
    return sums.index(min(sums))


def expand(raw, w, ct, depth, plte=b""):
    """raw rows (h, rb) -> BGR (h, w, 3) as cv2.imread's default mode: alpha dropped, 16 bits cut to the high byte, grey
    below 8 bits scaled to 0 .. 255, palette entries looked up (black beyond PLTE)"""
    h = raw.shape[0]
    ch = CHANNELS[ct]
    if depth < 8:
        bits = np.unpackbits(raw, axis=1)[:, :w * depth].reshape(h, w, depth)
        samples = (bits * (1 << np.arange(depth - 1, -1, -1))).sum(2).reshape(h, w, 1)
    else:
        samples = raw.reshape(h, w, ch, depth // 8)[:, :, :, 0].astype(np.int64)
    if ct == 3:
        pal = np.zeros((256, 3), np.uint8)
        pal[:len(plte) // 3] = np.frombuffer(plte, np.uint8).reshape(-1, 3)
        rgb = pal[samples[:, :, 0]]
    elif ct in (0, 4):
        g = samples[:, :, 0] * (255 // ((1 << depth) - 1) if depth < 8 else 1)
        rgb = np.stack([g, g, g], 2)
    else:
        rgb = samples[:, :, :3]
    return np.ascontiguousarray(rgb[:, :, ::-1], np.uint8)


def decode(data):
    """a PNG file -> BGR (h, w, 3)"""
    c = walk(data)
    assert c["interlace"] == 0
    rb = rowbytes(c["w"], c["ct"], c["depth"])
    inflated = zlib.decompress(c["idat"])
    assert len(inflated) >= c["h"] * (rb + 1), "short IDAT"
    return expand(unfilter(inflated, c["h"], rb, filter_unit(c["ct"], c["depth"])), c["w"], c["ct"], c["depth"], c["plte"])


def deflate(data, flavour):
    """zlib streams of the five kinds: stored blocks, fixed codes, dynamic codes without matches, runs only, long matches"""
    co = {"stored": lambda: zlib.compressobj(0),
          "fixed": lambda: zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED),
          "huffman": lambda: zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY),
          "rle": lambda: zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE),
          "best": lambda: zlib.compressobj(9)}[flavour]()
    return co.compress(data) + co.flush()


def filtered(raw, ct, depth, filters):
    """raw rows (h, rb) and a filter type per row -> the bytes IDAT deflates"""
    bpp = filter_unit(ct, depth)
    h, rb = raw.shape
    x = raw.astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if rb > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp] if rb > bpp else 0
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    pred = [np.zeros_like(x), a, b, (a + b) // 2, np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))]
    out = np.zeros((h, rb + 1), np.uint8)
    for y in range(h):                                       # (filtering reads raw bytes only: whole rows at once)
        out[y, 0] = filters[y]
        out[y, 1:] = (x[y] - pred[filters[y]][y]) & 255
    return out.tobytes()


def write(w, ct, depth, raw, filters, flavour="best", plte=b"", idat_split=0, extra=()):
    """raw rows (h, rowbytes) -> a PNG file with the given filter type in each row; idat_split > 0 cuts the stream into IDAT
    chunks of that many bytes; extra: chunks put between IHDR and the rest"""
    h = raw.shape[0]
    z = deflate(filtered(raw, ct, depth, filters), flavour)
    parts = [z[i:i + idat_split] for i in range(0, len(z), idat_split)] if idat_split else [z]
    return (SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, 0)) + b"".join(extra)
            + (chunk(b"PLTE", plte) if plte else b"") + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND"))


def encoder_rows(bgr):
    """a BGR image -> (raw RGB rows (h, 3w), the filter the heuristic picks for each row)"""
    raw = np.ascontiguousarray(bgr[:, :, ::-1]).reshape(bgr.shape[0], -1)
    prev, picks = [0] * raw.shape[1], []
    for y in range(raw.shape[0]):
        cur = raw[y].tolist()
        picks.append(heuristic(cur, prev, 3))
        prev = cur
    return raw, picks

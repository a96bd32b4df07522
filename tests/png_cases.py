"""Cases for the PNG tests, built with the writer of png_ref: images of every colour type and depth with chosen filter rows and
deflate flavours, the zlib streams of the inflate tests, and the committed Pillow-written files of tests/golden/png_cases.npz."""
import functools
import os
import struct
import zlib

import numpy as np

from . import png_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_cases.npz")
TYPES = [(ct, d) for ct in (0, 2, 3, 4, 6) for d in png_ref.DEPTHS[ct]]
# every filter on row 0 and every filter after every other one: 5 starts, then a walk over all 25 ordered pairs
FILTER_WALK = [0, 0, 1, 0, 2, 0, 3, 0, 4, 1, 1, 2, 1, 3, 1, 4, 2, 2, 3, 2, 4, 3, 3, 4, 4, 0]


def filters_for(h, start=0, seed=0):
    """h filter types: row 0 has `start`, then the walk that holds every ordered pair, then random ones"""
    rng = np.random.RandomState(seed + 17 * start + h)
    walk = [start] + FILTER_WALK
    return [walk[y] if y < len(walk) else int(rng.randint(5)) for y in range(h)]


def image(w, h, ct, depth, seed=0, flavour="best", filters=None, start=0, plte_n=None, smooth=False, **kw):
    """-> (file bytes, BGR reference (h, w, 3))"""
    rng = np.random.RandomState(1000 * seed + 31 * w + 7 * h + ct + depth)
    rb = png_ref.rowbytes(w, ct, depth)
    raw = rng.randint(0, 256, (h, rb)).astype(np.uint8)
    if smooth:                                           # neighbouring bytes close to one another: Avg and Paeth carry far
        raw = (np.cumsum(rng.randint(-2, 3, (h, rb)), 1) + np.cumsum(rng.randint(-2, 3, (h, 1)), 0) + 128).astype(np.uint8)
    plte = b""
    if ct == 3:
        plte_n = (1 << depth if depth < 8 else 200) if plte_n is None else plte_n
        plte = rng.randint(0, 256, plte_n * 3).astype(np.uint8).tobytes()
    filters = filters_for(h, start, seed) if filters is None else filters
    data = png_ref.write(w, ct, depth, raw, filters, flavour, plte, **kw)
    return data, png_ref.expand(raw, w, ct, depth, plte)


@functools.lru_cache(None)
def golden():
    """name -> (file bytes, BGR (h, w, 3)) of the committed Pillow-written files: every colour type and depth Pillow writes
    (it has no grey of 2 or 4 bits and no 16-bit colour or alpha: those come from png_ref's writer alone)"""
    with np.load(GOLDEN) as z:
        return {k: (z[k].tobytes(), z[k + "__bgr"]) for k in z.files if not k.endswith("__bgr")}


def write_golden(path=GOLDEN):
    """how tests/golden/png_cases.npz was made (needs Pillow): 37 x 29 images, the expected pixels from the arrays Pillow was
    given"""
    import io
    from PIL import Image
    rng = np.random.RandomState(11)
    h, w = 29, 37
    ramp = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + np.array([0, 60, 120]) + rng.randint(0, 4, (h, w, 3))).astype(np.uint8)
    out = {}

    def put(name, im, bgr, **kw):
        buf = io.BytesIO()
        im.save(buf, "PNG", **kw)
        out[name], out[name + "__bgr"] = np.frombuffer(buf.getvalue(), np.uint8), np.ascontiguousarray(bgr, np.uint8)

    grey = ramp[:, :, 0]
    g3 = lambda g: np.stack([g, g, g], 2)
    put("grey 1 bit", Image.fromarray(grey > 100), g3((grey > 100) * 255))
    put("grey 8 bit", Image.fromarray(grey), g3(grey))
    g16 = (grey.astype(np.uint16) << 8) | rng.randint(0, 256, (h, w)).astype(np.uint16)
    put("grey 16 bit", Image.fromarray(g16), g3(g16 >> 8))
    put("rgb 8 bit", Image.fromarray(ramp), ramp[:, :, ::-1])
    put("rgb 8 bit optimised", Image.fromarray(ramp), ramp[:, :, ::-1], optimize=True)
    pal = rng.randint(0, 256, (256, 3)).astype(np.uint8)
    for bits in (1, 2, 4, 8):
        idx = (grey.astype(np.int64) * 7 + rng.randint(0, 2, (h, w))) % (1 << bits)
        im = Image.fromarray(idx.astype(np.uint8), "P")
        im.putpalette(pal[:1 << bits].tobytes())
        put("palette %d bit" % bits, im, pal[idx][:, :, ::-1], bits=bits)
    alpha = rng.randint(0, 256, (h, w)).astype(np.uint8)
    put("grey alpha 8 bit", Image.fromarray(np.stack([grey, alpha], 2), "LA"), g3(grey))
    put("rgb alpha 8 bit", Image.fromarray(np.dstack([ramp, alpha]), "RGBA"), ramp[:, :, ::-1])
    np.savez(path, **out)


# ---- zlib streams for the inflate tests ----
class BitWriter:
    """deflate's bit order: values LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.bits(int(format(v, "0%db" % n)[::-1], 2) if n else 0, n)

    def flush(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)

    def stored(self, data, final=0):
        """a stored block of up to 65535 bytes"""
        self.bits(final, 1)
        self.bits(0, 2)
        self.flush()
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xffff) + data

    def fixed_match(self, length_symbol, length_extra, dist_symbol, dist_extra):
        """a length / distance pair in the fixed code; (symbol, extra value) each"""
        if length_symbol < 280:
            self.code(length_symbol - 256, 7)
        else:
            self.code(0xC0 + length_symbol - 280, 8)
        self.bits(length_extra, LENGTH_EXTRA_BITS[length_symbol - 257])
        self.code(dist_symbol, 5)
        self.bits(dist_extra, DIST_EXTRA_BITS[dist_symbol])


LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA_BITS = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA_BITS = [0, 0, 0, 0] + [b for b in range(1, 14) for _ in (0, 1)]


def far_matches(far):
    """written by hand, because zlib's deflate never looks back further than 32768 - 262: the 32768 bytes of `far` in a stored
    block, then a fixed block of three length / distance pairs at distance 32768 -- distance symbol 29 with all 13 extra bits
    set, the whole window -- of lengths 258, 3 and 100, and a pair at distance 24577 (symbol 29, extra 0) and one at 24576
    (symbol 28, extra 8191) -> (zlib stream, payload)"""
    assert len(far) == 32768
    w = BitWriter()
    w.stored(far)
    w.bits(1, 1)
    w.bits(1, 2)
    payload = bytearray(far)
    for lsym, lextra, dsym, dextra in ((285, 0, 29, 8191), (257, 0, 29, 8191), (279, 1, 29, 8191), (265, 1, 29, 0), (270, 2, 28, 8191)):
        w.fixed_match(lsym, lextra, dsym, dextra)
        length, dist = LENGTH_BASE[lsym - 257] + lextra, DIST_BASE[dsym] + dextra
        for _ in range(length):
            payload.append(payload[-dist])
    w.code(0, 7)
    return zwrap(w.flush(), bytes(payload)), bytes(payload)


def trace(z):
    """a walk through the blocks of a zlib stream by a small decoder of this file's own -> dict(types: the block types in
    order, max_length, max_distance: over all length / distance pairs, distance_symbols: the set used, repeats_span: whether a
    code-length repeat (16, 17 or 18) of a dynamic block starts among the literal/length lengths and ends among the distance
    lengths, payload)"""
    pos = [16]                                           # bit position; behind the two bytes of the wrapper

    def bits(n):
        v = 0
        for i in range(n):
            v |= ((z[pos[0] >> 3] >> (pos[0] & 7)) & 1) << i
            pos[0] += 1
        return v

    def decoder(lengths):
        table = {(l, c): s for s, (c, l) in canonical(lengths).items()}

        def symbol():
            code = 0
            for l in range(1, 16):
                code = code << 1 | bits(1)
                if (l, code) in table:
                    return table[(l, code)]
            raise ValueError("no code")
        return symbol

    out = bytearray()
    res = dict(types=[], max_length=0, max_distance=0, distance_symbols=set(), repeats_span=False)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    while True:
        final, kind = bits(1), bits(2)
        res["types"].append(kind)
        if kind == 0:
            pos[0] = (pos[0] + 7) & ~7
            n = bits(16)
            assert bits(16) == n ^ 0xffff
            out += z[pos[0] >> 3:(pos[0] >> 3) + n]
            pos[0] += 8 * n
        else:
            if kind == 1:
                lit, dist = decoder([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), decoder([5] * 30)
            else:
                nlen, ndist, ncode = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(ncode):
                    cl[order[i]] = bits(3)
                sym, lens = decoder(cl), []
                while len(lens) < nlen + ndist:
                    s, start = sym(), len(lens)
                    if s < 16:
                        lens.append(s)
                        continue
                    lens += [lens[-1]] * (3 + bits(2)) if s == 16 else [0] * (3 + bits(3)) if s == 17 else [0] * (11 + bits(7))
                    res["repeats_span"] |= start < nlen < len(lens)
                lit, dist = decoder(lens[:nlen]), decoder(lens[nlen:nlen + ndist])
            while True:
                s = lit()
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    length = LENGTH_BASE[s - 257] + bits(LENGTH_EXTRA_BITS[s - 257])
                    ds = dist()
                    d = DIST_BASE[ds] + bits(DIST_EXTRA_BITS[ds])
                    res["max_length"], res["max_distance"] = max(res["max_length"], length), max(res["max_distance"], d)
                    res["distance_symbols"].add(ds)
                    for _ in range(length):
                        out.append(out[-d])
        if final:
            res["payload"] = bytes(out)
            return res


def zwrap(deflated, payload):
    return b"\x78\x9c" + deflated + struct.pack(">I", zlib.adler32(payload) & 0xffffffff)


def canonical(lengths):
    """code lengths -> {symbol: (code, length)}"""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


def repeats_across_boundary():
    """a dynamic block whose code-length repeats (16, 17 and 18) run across the literal/length | distance boundary: 257
    literal/length lengths and 3 distance lengths, written by hand -> (zlib stream, payload)"""
    # literals 0..255: 'a' (97) and 'b' (98) of length 2, end-of-block of length 2, a length code 257 of length 2;
    # distance codes 0 .. 2 of length 2, 2, 1 -- so the run of 2s at the end of the literal lengths goes on into the distances
    lit = [0] * 258
    lit[97] = lit[98] = lit[256] = lit[257] = 2
    dist = [2, 2, 1]
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2); w.bits(258 - 257, 5); w.bits(3 - 1, 5)
    # the code-length alphabet: symbols 0 and 2 with two bits, 1, 16, 17 and 18 with three
    cl = {0: 2, 2: 2, 1: 3, 16: 3, 17: 3, 18: 3}          # 1/4 + 1/4 + 4/8 = 1: complete
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    w.bits(19 - 4, 4)
    for s in order:
        w.bits(cl.get(s, 0), 3)
    cc = canonical([cl.get(s, 0) for s in range(19)])
    seq = []                                             # (symbol, extra value, extra bits)
    seq += [(18, 97 - 11, 7)]                            # 97 zeros: literals 0 .. 96
    seq += [(2, 0, 0), (2, 0, 0)]                        # 97, 98
    seq += [(18, 138 - 11, 7), (17, 10 - 3, 3)]          # 99 .. 246: 148 zeros as 138 + 10
    seq += [(17, 9 - 3, 3)]                              # 247 .. 255
    seq += [(2, 0, 0)]                                   # 256
    seq += [(16, 3 - 3, 2)]                              # 257 and distance codes 0, 1: a repeat of 2 across the boundary
    seq += [(1, 0, 0)]                                   # distance code 2
    for s, ev, eb in seq:
        w.code(*cc[s])
        w.bits(ev, eb)
    lc, dc = canonical(lit), canonical(dist)
    # 'a' 'b' 'a' 'b', then twice a match of length 3 at distance 2
    w.code(*lc[97]); w.code(*lc[98]); w.code(*lc[97]); w.code(*lc[98])
    for _ in range(2):
        w.code(*lc[257]); w.code(*dc[1])                 # length 3 (code 257), distance 2 (code 1)
    w.code(*lc[256])
    payload = b"abab" + b"aba" + b"bab"
    return zwrap(w.flush(), payload), payload


def zeros_then_repeat_across():
    """a run of zeros (18) from the last literal/length lengths into an all-zero distance set"""
    lit = [0] * 260
    lit[120] = 1
    lit[256] = 1
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2); w.bits(260 - 257, 5); w.bits(30 - 1, 5)
    cl = {1: 1, 18: 2, 0: 2}
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    w.bits(19 - 4, 4)
    for s in order:
        w.bits(cl.get(s, 0), 3)
    cc = canonical([cl.get(s, 0) for s in range(19)])
    for s, ev, eb in [(18, 120 - 11, 7), (1, 0, 0), (18, 135 - 11, 7), (1, 0, 0), (18, 33 - 11, 7)]:   # 120 zeros, 120, 121 .. 255, 256, then 257 .. 259 and the 30 distance lengths
        w.code(*cc[s])
        w.bits(ev, eb)
    lc = canonical(lit)
    for _ in range(5):
        w.code(*lc[120])
    w.code(*lc[256])
    return zwrap(w.flush(), b"x" * 5), b"x" * 5


@functools.lru_cache(None)
def inflate_streams():
    """name -> (zlib stream, its payload): every construct the inflate tests name"""
    rng = np.random.RandomState(5)
    text = bytes(rng.randint(97, 105, 3000).astype(np.uint8))
    out = {}
    co = zlib.compressobj(0)
    out["empty stored block"] = (co.compress(b"") + co.flush(), b"")
    # stored, fixed and dynamic blocks in one stream: a full flush between changes of level and strategy
    co = zlib.compressobj(0)
    mixed = co.compress(text[:700]) + co.flush(zlib.Z_FULL_FLUSH)
    raw = mixed[2:]                                      # (no final block yet: Z_FULL_FLUSH ends on an empty stored block)
    fx = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    raw += fx.compress(text[700:1400]) + fx.flush(zlib.Z_FULL_FLUSH)
    dy = zlib.compressobj(9, zlib.DEFLATED, -15)
    raw += dy.compress(text[1400:] * 2) + dy.flush()
    payload = text[:1400] + text[1400:] * 2
    out["stored, fixed and dynamic blocks"] = (zwrap(raw, payload), payload)
    p = b"\x00" * 300 + text[:50] + b"\x07" * 600
    out["a match of length 258"] = (zlib.compress(p, 9), p)
    far = bytes(rng.randint(0, 256, 32768).astype(np.uint8))
    out["a match at distance 32768"] = far_matches(far)
    out["repeats across the boundary"] = repeats_across_boundary()
    out["zeros across the boundary"] = zeros_then_repeat_across()
    return out


@functools.lru_cache(None)
def small_streams():
    """six streams of at most about 600 bytes for the truncation and mutation test: the wrapper and all three block types"""
    rng = np.random.RandomState(9)
    text = bytes(rng.randint(97, 101, 400).astype(np.uint8))
    skew = bytes((rng.randint(0, 256, 500) * rng.randint(0, 2, 500) // 3).astype(np.uint8))
    return {"stored": png_ref.deflate(text[:150], "stored"),
            "fixed": png_ref.deflate(text + text[:90], "fixed"),
            "dynamic, literals only": png_ref.deflate(skew, "huffman"),
            "dynamic, runs": png_ref.deflate(b"\x00" * 90 + skew[:300] + b"\x05" * 70, "rle"),
            "dynamic, matches": zlib.compress(text * 3 + skew[:200], 9),
            "repeats across the boundary": repeats_across_boundary()[0]}

"""Streams for the tests of the staged and the device inflate, written with png_cases.BitWriter around the seams of the
window step: where a window ends, where half a ring leaves (flush_bytes) and where the ring wraps (2 * flush_bytes).  Every
dynamic block here has the header the project's encoder writes: all 19 code-length codes, the symbols 0 .. 15 with four bits
each, so a code length l is sent as the four bits of l."""
import functools
import zlib

import numpy as np

from . import png_cases
from .png_cases import DIST_BASE, DIST_EXTRA_BITS, LENGTH_BASE, LENGTH_EXTRA_BITS, BitWriter, canonical, zwrap


def _symbol(value, base):
    return max(s for s in range(len(base)) if base[s] <= value)


class Block:
    """a dynamic block of literals ("lit", byte), matches ("match", length, distance) and, last, its end-of-block code"""

    def __init__(self, lit, dist):
        """lit: {literal/length symbol: code length}, dist: {distance symbol: code length}"""
        self.nlen, self.ndist = max(257, max(lit) + 1), max(dist) + 1
        self.lit = [lit.get(s, 0) for s in range(self.nlen)]
        self.dist = [dist.get(s, 0) for s in range(self.ndist)]
        self.lc, self.dc = canonical(self.lit), canonical(self.dist)

    def write(self, w, tokens, final=1, eob=True):
        w.bits(final, 1); w.bits(2, 2); w.bits(self.nlen - 257, 5); w.bits(self.ndist - 1, 5); w.bits(15, 4)
        for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
            w.bits(0 if s >= 16 else 4, 3)
        for l in self.lit + self.dist:
            w.code(l, 4)
        n = 0
        for t in tokens:
            n += 1
            if t[0] == "lit":
                w.code(*self.lc[t[1]])
                continue
            ls, ds = _symbol(t[1], LENGTH_BASE), _symbol(t[2], DIST_BASE)
            if t[1] == 258:
                ls = 28
            w.code(*self.lc[257 + ls])
            w.bits(t[1] - LENGTH_BASE[ls], LENGTH_EXTRA_BITS[ls])
            w.code(*self.dc[ds])
            w.bits(t[2] - DIST_BASE[ds], DIST_EXTRA_BITS[ds])
        if eob:
            w.code(*self.lc[256])
        return n


def apply(payload, tokens):
    """the tokens on a bytearray; stops in front of a distance too far -> False"""
    for t in tokens:
        if t[0] == "lit":
            payload.append(t[1])
        else:
            if t[2] > len(payload):
                return False
            for _ in range(t[1]):
                payload.append(payload[-t[2]])
    return True


# 'a' one bit, 'b' two, end-of-block and the length 3 three bits; one distance code (distance 1) of one bit
ONES = Block({97: 1, 98: 2, 256: 3, 257: 3}, {0: 1})
# every code length 1 .. 15: the literals 97 .. 110 have 1 .. 14 bits, end-of-block and length symbol 284 (227 .. 257, five
# extra bits) 15; the distance symbols 0 .. 13 have 1 .. 14 bits, 28 and 29 (13 extra bits) 15: a pair of 15 + 5 + 15 + 13 bits
ALL = Block(dict([(97 + i, 1 + i) for i in range(14)] + [(256, 15), (284, 15)]), dict([(i, 1 + i) for i in range(14)] + [(28, 15), (29, 15)]))
# two bits for 'a', 'b' and the length 258, three for end-of-block and the length 3; distances 1, 2, 257 .. 384 and 24577 .. 32768
PAIRS = Block({97: 2, 98: 2, 285: 2, 256: 3, 257: 3}, {0: 2, 1: 2, 16: 2, 29: 2})
A, B = ("lit", 97), ("lit", 98)


@functools.lru_cache(None)
def seam_streams(window):
    """name -> (zlib stream, payload or None where the stream is refused, tokens: its literals and matches that are applied)"""
    rng = np.random.RandomState(3)
    far = bytes(rng.randint(0, 256, 32768).astype(np.uint8))
    out = {}

    def add(name, blocks, stored=b""):
        w, payload, n, ok = BitWriter(), bytearray(stored), 0, True
        if stored:
            w.stored(stored)
        for i, (block, tokens) in enumerate(blocks):
            block.write(w, tokens, final=int(i == len(blocks) - 1))
            before = len(payload)
            ok = ok and apply(payload, tokens)
            if not ok:
                # the tokens in front of the refused one count
                part = bytearray(payload[:before])
                for t in tokens:
                    if not apply(part, [t]):
                        break
                    n += 1
                break
            n += len(tokens)
        out[name] = (zwrap(w.flush(), bytes(payload)), bytes(payload) if ok else None, n)

    W = window
    add("a token on the last bit of a window", [(ONES, [A] * (W - 1) + [B] + [A] * 5)])
    add("a token on the first bit of the next window", [(ONES, [A] * W + [B] + [A] * 3)])
    add("a pair of 48 bits from inside a window to outside it", [(ALL, [A] * (W - 10) + [("match", 227 + 30, 24577 + 8000), A, ("lit", 98)])], stored=far)
    add("end-of-block as the only token of a window", [(ONES, []), (ONES, [A, B]), (ONES, [])])
    add("end-of-block as the first token of a window", [(ONES, [A] * W), (ONES, [B] * 3)])
    add("end-of-block as the last token of a window", [(ONES, [A] * (W - 1)), (ONES, [B] * (W // 2 - 2) + [A]), (ONES, [A])])
    add("windows of one-bit codes", [(ONES, [A] * (3 * W + 1) + [B])])
    add("every code length 1 .. 15", [(ALL, [("lit", 97 + i) for i in range(14)] * 3 + [("match", 227, 24577), ("match", 257, 32768), ("match", 240, 1), ("lit", 110)])],
        stored=far)
    pairs = []
    for length in (3, 258):
        for d in (1, 2, 257, 32767, 32768):
            pairs += [A, B, ("match", length, d), B, A]
    add("matches at distances 1, 2, 257, 32767 and 32768 between literals", [(PAIRS, pairs)], stored=far)
    add("a distance one byte too far as a later token of a window", [(PAIRS, [A, ("match", 3, 2), A])])
    add("a distance one byte too far as the first token of a window", [(PAIRS, [A] * (W // 2) + [("match", 3, 257), A])], stored=far[:256 - W // 2])
    return out


@functools.lru_cache(None)
def sized_streams(flush):
    """payload length -> (zlib stream of level 6, payload): lengths around the flush (half a ring) and the ring's size"""
    rng = np.random.RandomState(8)
    text = bytes((rng.randint(0, 6, 70000) * rng.randint(0, 2, 70000) + rng.randint(0, 2, 70000) * 90).astype(np.uint8))
    return {n: (zlib.compress(text[:n], 6), text[:n]) for n in (flush - 1, flush, flush + 1, 2 * flush - 1, 2 * flush, 2 * flush + 1, 4 * flush + 1)}


def damaged():
    """every truncation and the three changes of every byte of png_cases.small_streams(): (name, stream), about 5 000"""
    for name, z in sorted(png_cases.small_streams().items()):
        for cut in range(len(z)):
            yield "%s cut at %d" % (name, cut), z[:cut]
        for at in range(len(z)):
            for x in (0x01, 0x80, 0xFF):
                m = bytearray(z)
                m[at] ^= x
                yield "%s byte %d xor %#x" % (name, at, x), bytes(m)


def count_tokens(z):
    """the literals and matches of a zlib stream, counted by a decoder of this file's own (end-of-block codes and the bytes of
    stored blocks are no tokens) -> (tokens, payload bytes)"""
    pos = 16
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    word = int.from_bytes(z, "little")

    def bits(n):
        nonlocal pos
        v = (word >> pos) & ((1 << n) - 1)
        pos += n
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

    tokens = produced = 0
    while True:
        final, kind = bits(1), bits(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            bits(16)
            pos += 8 * n
            produced += n
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
                    s = sym()
                    lens += [s] if s < 16 else [lens[-1]] * (3 + bits(2)) if s == 16 else [0] * (3 + bits(3)) if s == 17 else [0] * (11 + bits(7))
                lit, dist = decoder(lens[:nlen]), decoder(lens[nlen:nlen + ndist])
            while True:
                s = lit()
                if s == 256:
                    break
                tokens += 1
                if s < 256:
                    produced += 1
                    continue
                produced += LENGTH_BASE[s - 257] + bits(LENGTH_EXTRA_BITS[s - 257])
                bits(DIST_EXTRA_BITS[dist()])
        if final:
            return tokens, produced

"""A plain restatement of the PNG encoder's runs mode for the tests: the rule that turns the filtered bytes of a band into
literals and matches of distance 1, and a small inflate that walks a zlib stream of dynamic blocks and reports their headers
and tokens.  Shares no code with the library."""
import zlib

MAX_MATCH = 258
# RFC 1951, 3.2.5: the length symbols 257 .. 285
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def tokens(band):
    """the filtered bytes of one band -> [("L", byte) | ("M", length)]: of every maximal run of n equal bytes the first is
    a literal; the n - 1 behind it are 258 k + t: k matches of length 258, then one of length t where t >= 3, else t literals"""
    out, i, n = [], 0, len(band)
    while i < n:
        j = i
        while j < n and band[j] == band[i]:
            j += 1
        out.append(("L", band[i]))
        k, t = divmod(j - i - 1, MAX_MATCH)
        out += [("M", MAX_MATCH)] * k
        out += [("M", t)] if t >= 3 else [("L", band[i])] * t
        i = j
    return out


def counts(band_list):
    """-> (literal tokens, match tokens) of a frame's bands"""
    toks = [t for b in band_list for t in tokens(b)]
    return sum(k == "L" for k, _ in toks), sum(k == "M" for k, _ in toks)


class _Bits:
    def __init__(self, data, at):
        self.data, self.pos = data, 8 * at

    def take(self, n):
        v = 0
        for i in range(n):
            assert self.pos < 8 * len(self.data), "the stream ends inside a block"
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _decoder(lens):
    """code lengths -> {(length, code): symbol} of the canonical code (codes as numbers, first bit the highest)"""
    table, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise AssertionError("15 bits that are no code")


def _kraft(lens):
    return sum(2 ** (15 - l) for l in lens if l)


def trace(z):
    """a zlib stream of dynamic blocks -> [dict(hlit, hdist, lit_lens, dist_lens, tokens)], one per deflate block, tokens as
    tokens() gives them.  Asserts that both codes of every block satisfy Kraft with equality, that every distance is 1, and
    that the stream ends where the Adler-32 begins (which is that of the bytes the tokens stand for)."""
    assert z[0] & 15 == 8 and (z[0] << 8 | z[1]) % 31 == 0 and not z[1] & 0x20, "zlib header"
    bits, out, blocks, last = _Bits(z, 2), bytearray(), [], 0
    while not last:
        last, kind = bits.take(1), bits.take(2)
        assert kind == 2, "block type %d" % kind
        hlit, hdist, hclen = bits.take(5), bits.take(5), bits.take(4)
        cl = [0] * 19
        for i in range(hclen + 4):
            cl[CL_ORDER[i]] = bits.take(3)
        assert _kraft(cl) == 1 << 15, "code-length code"
        cl_table, lens = _decoder(cl), []
        while len(lens) < hlit + 257 + hdist + 1:
            s = _symbol(bits, cl_table)
            if s < 16:
                lens.append(s)
            elif s == 16:
                lens += [lens[-1]] * (3 + bits.take(2))
            else:
                lens += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
        assert len(lens) == hlit + 257 + hdist + 1
        lit_lens, dist_lens = lens[:hlit + 257], lens[hlit + 257:]
        assert _kraft(lit_lens) == 1 << 15, "literal/length code: Kraft sum %d / 32768" % _kraft(lit_lens)
        assert _kraft(dist_lens) == 1 << 15, "distance code: Kraft sum %d / 32768" % _kraft(dist_lens)
        assert lit_lens[256], "no end-of-block code"
        lit_table, dist_table, toks = _decoder(lit_lens), _decoder(dist_lens), []
        while True:
            s = _symbol(bits, lit_table)
            if s < 256:
                toks.append(("L", s))
                out.append(s)
            elif s == 256:
                break
            else:
                length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                d = _symbol(bits, dist_table)
                dist = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                assert dist == 1, "a match at distance %d" % dist
                assert out, "a match with nothing before it"
                toks.append(("M", length))
                out += bytes([out[-1]]) * length
        blocks.append(dict(hlit=hlit, hdist=hdist, lit_lens=lit_lens, dist_lens=dist_lens, tokens=toks))
    end = (bits.pos + 7) // 8
    assert end + 4 == len(z), "the deflate data ends at byte %d of %d: the Adler-32 does not begin there" % (end, len(z))
    assert int.from_bytes(z[end:], "big") == zlib.adler32(bytes(out)), "Adler-32"
    return blocks

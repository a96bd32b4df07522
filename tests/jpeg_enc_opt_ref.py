"""Optimised Huffman tables in plain Python: libjpeg's optimize_coding restated, the reference the optimised-table tests hold
the library against.  It shares no code with camkifu_amd; the colour conversion, the DCT, the headers around the DHT segments
and the bit writer are those of jpeg_enc_ref.

  symbols(coef, h, w, sampling, restart_interval)  -> [(table, symbol, value bits, size)] in the coder's order,
                                                      table 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma
  histogram(coef, h, w, sampling, restart_interval) -> (4, 256) int64
  code_sizes(freq)                                  -> the 257 code sizes of jpeg_gen_optimal_table before they are limited
  optimal_table(freq)                               -> (bits[16], vals): jpeg_gen_optimal_table
  code_lengths(bits, vals)                          -> {symbol: (code, length)}
  entropy_encode(coef, quant, h, w, sampling, restart_interval=0) -> bytes
  encode(bgr, quality, sampling, restart_interval=0)              -> bytes
"""
import numpy as np

from . import jpeg_enc_ref as ref


def symbols(coef, h, w, sampling, restart_interval=0):
    """what the coder emits, MCU by MCU: (table, symbol, value, size) and ("rst", k) between restart intervals"""
    mx, my, grids = ref.geometry(h, w, sampling)
    fx, fy = ref.reductions(sampling)
    coef = np.asarray(coef).reshape(-1, 64).astype(np.int64)
    assert coef.shape[0] == ref.n_blocks(h, w, sampling)
    planes, at = [], 0
    for gx, gy in grids:
        planes.append(coef[at:at + gx * gy].reshape(gy, gx, 64)[:, :, ref.ZIGZAG])
        at += gx * gy
    out, pred, since, nrst = [], [0, 0, 0], 0, 0
    for mcu in range(mx * my):
        if restart_interval and since == restart_interval:
            out.append(("rst", nrst))
            nrst += 1
            since, pred = 0, [0, 0, 0]
        since += 1
        mcy, mcx = divmod(mcu, mx)
        for c in range(len(grids)):
            bh, bv = (fx, fy) if c == 0 else (1, 1)
            chroma = 2 if c else 0
            for v in range(bv):
                for u in range(bh):
                    blk = planes[c][mcy * bv + v, mcx * bh + u]
                    diff = int(blk[0]) - pred[c]
                    pred[c] = int(blk[0])
                    s = abs(diff).bit_length()
                    if s > 11:
                        raise ValueError("DC difference of %d bits (MCU %d): baseline JPEG has 11" % (s, mcu))
                    out.append((chroma, s, diff if diff >= 0 else diff - 1, s))
                    run = 0
                    for k in range(1, 64):
                        val = int(blk[k])
                        if val == 0:
                            run += 1
                            continue
                        while run > 15:
                            out.append((chroma + 1, 0xF0, 0, 0))
                            run -= 16
                        s = abs(val).bit_length()
                        if s > 10:
                            raise ValueError("AC value of %d bits (MCU %d): baseline JPEG has 10" % (s, mcu))
                        out.append((chroma + 1, (run << 4) | s, val if val >= 0 else val - 1, s))
                        run = 0
                    if run:
                        out.append((chroma + 1, 0, 0, 0))
    return out


def histogram(coef, h, w, sampling, restart_interval=0):
    freq = np.zeros((4, 256), np.int64)
    for item in symbols(coef, h, w, sampling, restart_interval):
        if item[0] != "rst":
            freq[item[0], item[1]] += 1
    return freq


def code_sizes(freq):
    """the first half of jpeg_gen_optimal_table: 256 counts -> the code size of every symbol and of the pseudo-symbol 256,
    before any limit (0: the symbol does not occur)"""
    freq = [int(v) for v in freq] + [1]                    # the pseudo-symbol 256: no real symbol gets the code of all ones
    assert len(freq) == 257
    codesize, others = [0] * 257, [-1] * 257

    def least(skip):
        c, v = -1, None
        for i in range(257):
            if i != skip and freq[i] and (v is None or freq[i] <= v):     # `<=`: the largest index among equals
                c, v = i, freq[i]
        return c

    while True:
        c1 = least(-1)
        c2 = least(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def optimal_table(freq):
    """jpeg_gen_optimal_table over 256 counts -> (bits, vals): bits[l - 1] codes of l bits, vals in code order"""
    codesize = code_sizes(freq)
    assert max(codesize) <= 32, "libjpeg gives up on a code of more than 32 bits"
    bits = [0] * 33
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for length in range(1, 33) for s in range(256) if codesize[s] == length]
    assert sum(bits[1:17]) == len(vals) and not any(bits[17:])
    return bits[1:17], vals


def code_lengths(bits, vals):
    return ref._code_table(list(bits), list(vals))


def headers(quant, h, w, sampling, restart_interval, tables):
    """jpeg_enc_ref's header with the frame's own tables in its DHT segments: [(bits, vals)] DC0, AC0(, DC1, AC1)"""
    std = ref.headers(quant, h, w, sampling, restart_interval)
    first = std.index(b"\xff\xc4")
    at = first
    while std[at:at + 2] == b"\xff\xc4":
        at += 2 + int.from_bytes(std[at + 2:at + 4], "big")
    ids = [0x00, 0x10, 0x01, 0x11]
    dht = b"".join(ref._segment(0xC4, bytes([ids[t]]) + bytes(b) + bytes(v)) for t, (b, v) in enumerate(tables))
    return std[:first] + dht + std[at:]


def entropy_encode(coef, quant, h, w, sampling, restart_interval=0):
    items = symbols(coef, h, w, sampling, restart_interval)                # refusals come from here, before any table
    freq = np.zeros((4, 256), np.int64)
    for item in items:
        if item[0] != "rst":
            freq[item[0], item[1]] += 1
    ntab = 2 if sampling == ref.GREY else 4
    tables = [optimal_table(freq[t]) for t in range(ntab)]
    codes = [code_lengths(*t) for t in tables]
    out = bytearray(headers(quant, h, w, sampling, restart_interval, tables))
    bw = ref._BitWriter(out, ref.new_stats())
    for item in items:
        if item[0] == "rst":
            bw.flush()
            out += bytes([0xFF, 0xD0 + (item[1] & 7)])
            continue
        t, sym, val, size = item
        bw.put(*codes[t][sym])
        if size:
            bw.put(val, size)
    bw.flush()
    out += b"\xff\xd9"
    return bytes(out)


def encode(bgr, quality, sampling, restart_interval=0):
    bgr = np.asarray(bgr)
    q = ref.quant_tables(quality)
    return entropy_encode(ref.forward(bgr, q, sampling), q, bgr.shape[0], bgr.shape[1], sampling, restart_interval)

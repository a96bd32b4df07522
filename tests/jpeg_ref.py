"""A plain numpy baseline-JPEG decoder and AVI walker: the reference the JPEG tests hold the library against.

It restates libjpeg's default decode path (slow-integer IDCT, "fancy" chroma upsampling, fixed-point YCbCr -> RGB), which
is what cv2.imread and Pillow run, and shares no code with camkifu_amd.  Everything is computed in int64 and every
intermediate is asserted to fit int32, so a case that leaves the domain of the GPU kernel fails when the cases are built.

  parse(data)                    -> Frame (geometry, tables, the entropy-coded segment)
  coefficients(data)             -> (info, coef int16 flat, quant uint16 (3, 64))   the layout of ck_jpeg_coefficients
  reconstruct(coef, quant, h, w, sampling) -> (h, w, 3) BGR
  decode(data)                   -> (h, w, 3) BGR
  avi_index(buf)                 -> dict(h, w, fps, chunks=[bytes, ...])
"""
import struct

import numpy as np

GREY, S444, S422, S420 = 0, 1, 2, 3

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                   46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.3: (bits, values) of the default tables -- DC luma, DC chroma, AC luma, AC chroma
_DC_VALS = list(range(12))
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], _DC_VALS)
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], _DC_VALS)
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
    0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
    0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])


class JpegError(ValueError):
    pass


def _codes(bits, vals):
    """(length, code) -> symbol"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


STD_TABLES = {(0, 0): _codes(*STD_DC_LUMA), (0, 1): _codes(*STD_DC_CHROMA),
              (1, 0): _codes(*STD_AC_LUMA), (1, 1): _codes(*STD_AC_CHROMA)}


class Frame:
    pass


def segments(data):
    """[(marker, payload offset, payload length)] up to and including SOS (whose payload is its header)"""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise JpegError("no SOI")
    out, p = [], 2
    while True:
        if p + 4 > len(data):
            raise JpegError("ran past the end in the headers")
        if data[p] != 0xFF:
            raise JpegError("marker expected at byte %d" % p)
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        ln = struct.unpack(">H", data[p + 2:p + 4])[0]
        if ln < 2 or p + 2 + ln > len(data):
            raise JpegError("segment past the end")
        out.append((m, p + 4, ln - 2))
        p += 2 + ln
        if m == 0xDA:
            return out, p


def parse(data):
    data = bytes(data)
    segs, scan_at = segments(data)
    f = Frame()
    f.qt, f.huff, f.ri, f.comps, f.scan = {}, {}, 0, None, None
    for m, o, ln in segs:
        seg = data[o:o + ln]
        if m == 0xDB:
            p = 0
            while p < ln:
                pq, tq = seg[p] >> 4, seg[p] & 15
                p += 1
                if pq:
                    f.qt[tq] = np.array(struct.unpack(">64H", seg[p:p + 128]))
                    p += 128
                else:
                    f.qt[tq] = np.frombuffer(seg[p:p + 64], np.uint8).astype(np.int64)
                    p += 64
        elif m == 0xC0:
            prec, f.h, f.w, nc = struct.unpack(">BHHB", seg[:6])
            if prec != 8:
                raise JpegError("precision")
            f.comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise JpegError("frame type")
        elif m == 0xC4:
            p = 0
            while p < ln:
                tc, th = seg[p] >> 4, seg[p] & 15
                bits = list(seg[p + 1:p + 17])
                n = sum(bits)
                f.huff[(tc, th)] = _codes(bits, list(seg[p + 17:p + 17 + n]))
                p += 17 + n
        elif m == 0xDD:
            f.ri = struct.unpack(">H", seg[:2])[0]
        elif m == 0xDA:
            ns = seg[0]
            f.scan = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
    if f.comps is None or f.scan is None or len(f.scan) != len(f.comps):
        raise JpegError("no frame, or not one interleaved scan")
    if not f.huff:
        f.huff = dict(STD_TABLES)
    nc = len(f.comps)
    if nc == 1:
        f.sampling = GREY
    else:
        hv = (f.comps[0][1], f.comps[0][2])
        if nc != 3 or hv not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in f.comps[1:]):
            raise JpegError("sampling")
        f.sampling = {(1, 1): S444, (2, 1): S422, (2, 2): S420}[hv]
    f.data, f.scan_at = data, scan_at
    return f


def geometry(h, w, sampling):
    """-> (mcus across, mcus down, [(blocks across, blocks down) per component], blocks of luma per MCU (across, down))"""
    hs, vs = {GREY: (1, 1), S444: (1, 1), S422: (2, 1), S420: (2, 2)}[sampling]
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    grids = [(mx * hs, my * vs)] + ([(mx, my)] * 2 if sampling != GREY else [])
    return mx, my, grids, (hs, vs)


def n_blocks(h, w, sampling):
    return sum(a * b for a, b in geometry(h, w, sampling)[2])


def _unstuff(data, p):
    """the entropy-coded segment from byte p on -> list of restart intervals (bytes), as the RSTn markers cut it"""
    parts, cur, n = [], bytearray(), len(data)
    expect = 0
    while p < n:
        b = data[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
            continue
        if p + 1 >= n:
            break
        m = data[p + 1]
        if m == 0:
            cur.append(0xFF)
            p += 2
        elif 0xD0 <= m <= 0xD7:
            if m - 0xD0 != expect:
                raise JpegError("restart marker out of order")
            expect = (expect + 1) & 7
            parts.append(bytes(cur))
            cur = bytearray()
            p += 2
        elif m == 0xFF:
            p += 1
        else:
            break
    parts.append(bytes(cur))
    return parts


class _Bits:
    def __init__(self, buf):
        self.buf, self.pos, self.acc, self.n = buf, 0, 0, 0

    def bit(self):
        if self.n == 0:
            if self.pos >= len(self.buf):
                raise JpegError("ran past the end of the entropy-coded data")
            self.acc = self.buf[self.pos]
            self.pos += 1
            self.n = 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise JpegError("unknown code")

    def value(self, k):
        if k == 0:
            return 0
        v = self.bits(k)
        return v if v >= (1 << (k - 1)) else v - (1 << k) + 1


def coefficients(data):
    """-> (info dict, coef, quant): coef int16, component-planar, blocks in raster order over the MCU-padded grid, 64 values
    per block in natural order, not dequantised; quant uint16 (3, 64) in natural order, by component"""
    f = parse(data)
    mx, my, grids, (hs, vs) = geometry(f.h, f.w, f.sampling)
    nc = len(f.comps)
    planes = [np.zeros((gy, gx, 64), np.int64) for gx, gy in grids]
    quant = np.zeros((3, 64), np.int64)
    for c in range(nc):
        q = f.qt.get(f.comps[c][3])
        if q is None:
            raise JpegError("missing quantisation table")
        quant[c, ZIGZAG] = q
    tables = []
    for c in range(nc):
        sid, td, ta = f.scan[c]
        if (0, td) not in f.huff or (1, ta) not in f.huff:
            raise JpegError("missing Huffman table")
        tables.append((f.huff[(0, td)], f.huff[(1, ta)]))
    parts = _unstuff(f.data, f.scan_at)
    total = mx * my
    ri = f.ri or total
    if len(parts) < -(-total // ri):
        raise JpegError("missing restart marker")
    mcu = 0
    for part in parts:
        if mcu >= total:
            break
        br, pred = _Bits(part), [0] * nc
        for _ in range(min(ri, total - mcu)):
            mcy, mcx = divmod(mcu, mx)
            for c in range(nc):
                bh, bv = (hs, vs) if (c == 0 and nc == 3) else (1, 1)
                for v in range(bv):
                    for u in range(bh):
                        blk = planes[c][mcy * bv + v, mcx * bh + u]
                        s = br.symbol(tables[c][0])
                        if s > 11:
                            raise JpegError("DC size")
                        pred[c] += br.value(s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = br.symbol(tables[c][1])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise JpegError("coefficient index above 63")
                            blk[ZIGZAG[k]] = br.value(s)
                            k += 1
            mcu += 1
    coef = np.concatenate([p.reshape(-1) for p in planes])
    assert np.abs(coef).max() < 32768
    info = dict(h=f.h, w=f.w, sampling=f.sampling, restart_interval=f.ri, blocks=int(coef.size // 64))
    return info, coef.astype(np.int16), quant.astype(np.uint16)


# ---- reconstruction --------------------------------------------------------------------------------------------
def _i32(x):
    assert np.abs(x).max(initial=0) < 2 ** 31, "an intermediate leaves int32"
    return x


def _butterfly(x, shift):
    """the 8-point pass of jidctint (CONST_BITS 13) along the LAST axis of x (int64), descaled by `shift`"""
    i0, i1, i2, i3, i4, i5, i6, i7 = [x[..., k] for k in range(8)]
    z1 = _i32((i2 + i6) * 4433)
    t2 = _i32(z1 + _i32(i6 * -15137))
    t3 = _i32(z1 + _i32(i2 * 6270))
    t0 = _i32((i0 + i4) << 13)
    t1 = _i32((i0 - i4) << 13)
    t10, t13, t11, t12 = _i32(t0 + t3), _i32(t0 - t3), _i32(t1 + t2), _i32(t1 - t2)
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = _i32((z3 + z4) * 9633)
    o0, o1, o2, o3 = _i32(o0 * 2446), _i32(o1 * 16819), _i32(o2 * 25172), _i32(o3 * 12299)
    z1, z2, z3, z4 = _i32(z1 * -7373), _i32(z2 * -20995), _i32(z3 * -16069), _i32(z4 * -3196)
    z3, z4 = _i32(z3 + z5), _i32(z4 + z5)
    o0, o1, o2, o3 = _i32(o0 + _i32(z1 + z3)), _i32(o1 + _i32(z2 + z4)), _i32(o2 + _i32(z2 + z3)), _i32(o3 + _i32(z1 + z4))
    rnd = 1 << (shift - 1)
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([_i32(_i32(v) + rnd) >> shift for v in out], axis=-1)


RANGE_TABLE = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, np.int64), np.arange(0, 128)]).astype(np.int64)


def idct_plane(coef, quant):
    """coef (gy, gx, 64) of one component, quant (64,) -> samples (gy*8, gx*8) int64 in 0..255"""
    gy, gx, _ = coef.shape
    x = _i32(coef.astype(np.int64) * quant.astype(np.int64)).reshape(gy, gx, 8, 8)
    ws = _butterfly(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)      # pass 1: down the columns
    px = RANGE_TABLE[_butterfly(ws, 18) & 1023]                    # pass 2: along the rows
    return px.transpose(0, 2, 1, 3).reshape(gy * 8, gx * 8)


def upsample_h2v2(c, h, w):
    """fancy upsampling of one chroma plane of the REAL size (ceil(h/2), ceil(w/2)) -> (h, w); libjpeg takes the fancy
    path only for planes more than 2 samples wide (jdsample.c: downsampled_width > 2) and replicates samples otherwise"""
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w]
    rows = np.arange(2 * ch)
    near = rows >> 1
    far = np.clip(np.where(rows & 1, near + 1, near - 1), 0, ch - 1)
    s = 3 * c[near] + c[far]
    cols = np.arange(2 * cw)
    cc = cols >> 1
    nb = np.clip(np.where(cols & 1, cc + 1, cc - 1), 0, cw - 1)
    out = (3 * s[:, cc] + s[:, nb] + np.where(cols & 1, 7, 8)) >> 4
    return out[:h, :w]


def upsample_h2v1(c, h, w):
    ch, cw = c.shape
    if cw <= 2:                                            # as above
        return np.repeat(c, 2, axis=1)[:h, :w]
    cols = np.arange(2 * cw)
    cc = cols >> 1
    nb = np.clip(np.where(cols & 1, cc + 1, cc - 1), 0, cw - 1)
    out = (3 * c[:, cc] + c[:, nb] + np.where(cols & 1, 2, 1)) >> 2
    return out[:h, :w]


def reconstruct(coef, quant, h, w, sampling):
    _, _, grids, _ = geometry(h, w, sampling)
    coef = np.asarray(coef).reshape(-1, 64)
    planes, at = [], 0
    for c, (gx, gy) in enumerate(grids):
        planes.append(idct_plane(coef[at:at + gx * gy].reshape(gy, gx, 64), np.asarray(quant)[c]))
        at += gx * gy
    assert at == coef.shape[0], "coefficient count does not match the geometry"
    y = planes[0][:h, :w]
    if sampling == GREY:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    if sampling == S444:
        cb, cr = planes[1][:h, :w], planes[2][:h, :w]
    elif sampling == S422:
        cw = (w + 1) // 2
        cb, cr = upsample_h2v1(planes[1][:h, :cw], h, w), upsample_h2v1(planes[2][:h, :cw], h, w)
    else:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        cb, cr = upsample_h2v2(planes[1][:ch, :cw], h, w), upsample_h2v2(planes[2][:ch, :cw], h, w)
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=2), 0, 255).astype(np.uint8)


def decode(data):
    info, coef, quant = coefficients(data)
    return reconstruct(coef, quant, info["h"], info["w"], info["sampling"])


# ---- AVI ----------------------------------------------------------------------------------------------------------
def avi_index(buf):
    """walk a RIFF 'AVI ' file: -> dict(h, w, fps, chunks): the ##dc / ##db chunks of the first movi list, in file order"""
    buf = bytes(buf)
    if buf[:4] != b"RIFF" or buf[8:12] != b"AVI ":
        raise JpegError("not an AVI file")
    out = dict(h=0, w=0, fps=0.0, chunks=[])
    end = min(len(buf), 8 + struct.unpack("<I", buf[4:8])[0])

    def walk(p, stop, in_movi):
        while p + 8 <= stop:
            cc, ln = buf[p:p + 4], struct.unpack("<I", buf[p + 4:p + 8])[0]
            body = p + 8
            if cc == b"LIST":
                walk(body + 4, min(stop, body + ln), buf[body:body + 4] == b"movi")
            elif cc == b"strh" and buf[body:body + 4] == b"vids" and not out["fps"]:
                scale, rate = struct.unpack("<II", buf[body + 20:body + 28])
                out["fps"] = rate / scale if scale else 0.0
            elif cc == b"strf" and not out["w"]:
                out["w"], out["h"] = struct.unpack("<ii", buf[body + 4:body + 12])
                out["h"] = abs(out["h"])
            elif in_movi and cc[2:4] in (b"dc", b"db"):
                out["chunks"].append(buf[body:min(stop, body + ln)])
            p = body + ln + (ln & 1)

    walk(12, end, False)
    return out

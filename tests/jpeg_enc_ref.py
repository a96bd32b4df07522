"""A plain numpy / Python baseline-JPEG encoder: the reference the JPEG encoder tests hold the library against.

It restates libjpeg's default compressor (16-bit fixed-point RGB -> YCbCr, box downsampling without smoothing, the
slow-integer forward DCT, quantisation by truncating division, the Annex K.3 Huffman tables, JFIF headers), which is what
PIL.Image.save(buf, "JPEG", quality=q, subsampling=s) runs, byte for byte, and shares no code with camkifu_amd.

  quant_tables(quality)                         -> (3, 64) uint16, natural order, by component (Y, Cb, Cr)
  ycc(bgr)                                      -> (y, cb, cr) int64 planes
  forward(bgr, quant, sampling)                 -> coef int16 flat, the layout of ck_jpeg_coefficients
  entropy_encode(coef, quant, h, w, sampling, restart_interval=0, stats=None) -> bytes
  encode(bgr, quality, sampling, restart_interval=0, stats=None)              -> bytes
  size_bound(h, w, sampling)                    -> the library's bound on a stream, restated
"""
import struct

import numpy as np

GREY, S444, S422, S420 = 0, 1, 2, 3

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                   46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.1 and K.2, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# Annex K.3: (bits, values) -- DC luma, DC chroma, AC luma, AC chroma
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


def _fix(x):
    return int(x * 65536 + 0.5)


def _i32(x):
    assert np.abs(x).max(initial=0) < 2 ** 31, "an intermediate leaves int32"
    return x


def reductions(sampling):
    """(fx, fy): how much chroma is reduced across and down = luma blocks per MCU across and down"""
    return {GREY: (1, 1), S444: (1, 1), S422: (2, 1), S420: (2, 2)}[sampling]


def geometry(h, w, sampling):
    """-> (mcus across, mcus down, [(blocks across, blocks down) per component] on the MCU-padded grid)"""
    fx, fy = reductions(sampling)
    mx, my = -(-w // (8 * fx)), -(-h // (8 * fy))
    return mx, my, [(mx * fx, my * fy)] + ([(mx, my)] * 2 if sampling != GREY else [])


def n_blocks(h, w, sampling):
    return sum(a * b for a, b in geometry(h, w, sampling)[2])


# ---- tables ---------------------------------------------------------------------------------------------------------------
def quant_tables(quality):
    """jpeg_set_quality(q, force_baseline)"""
    q = min(100, max(1, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    lum = np.clip((BASE_LUMA * scale + 50) // 100, 1, 255)
    chr_ = np.clip((BASE_CHROMA * scale + 50) // 100, 1, 255)
    return np.stack([lum, chr_, chr_]).astype(np.uint16)


# ---- colour, edges, downsampling ----------------------------------------------------------------------------------------
def ycc(bgr):
    b, g, r = [bgr[..., k].astype(np.int64) for k in range(3)]
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(a, rows, cols):
    """replicate the last row and the last column up to (rows, cols)"""
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def component_plane(full, fx, fy):
    """a full-size plane (h, w) -> the component's samples over its REAL blocks (hb * 8, wb * 8), libjpeg's edge order: widen
    the full-size columns, rows only to a multiple of fy, downsample, then replicate the DOWNSAMPLED rows"""
    h, w = full.shape
    cw, ch = -(-w // fx), -(-h // fy)
    wb, hb = -(-cw // 8), -(-ch // 8)
    a = _pad(full, ch * fy, wb * 8 * fx)
    if (fx, fy) == (2, 1):
        a = (a[:, 0::2] + a[:, 1::2] + (np.arange(wb * 8) & 1)) >> 1
    elif (fx, fy) == (2, 2):
        a = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 1 + (np.arange(wb * 8) & 1)) >> 2
    else:
        assert (fx, fy) == (1, 1)
    return _pad(a, hb * 8, wb * 8)


# ---- forward DCT and quantisation ---------------------------------------------------------------------------------------
def _descale(x, n):
    return _i32(_i32(x) + (1 << (n - 1))) >> n


def _fdct_pass(x, first):
    """jfdctint's 8-point pass (CONST_BITS 13, PASS1_BITS 2) along the LAST axis of x (int64)"""
    d = [x[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = _i32((t12 + t13) * 4433)
    o2 = _descale(z1 + _i32(t13 * 6270), n)
    o6 = _descale(z1 + _i32(t12 * -15137), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = _i32((z3 + z4) * 9633)
    t4, t5, t6, t7 = _i32(t4 * 2446), _i32(t5 * 16819), _i32(t6 * 25172), _i32(t7 * 12299)
    z1, z2, z3, z4 = _i32(z1 * -7373), _i32(z2 * -20995), _i32(z3 * -16069), _i32(z4 * -3196)
    z3, z4 = z3 + z5, z4 + z5
    o7, o5 = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n)
    o3, o1 = _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=-1)


def fdct_quant(plane, quant):
    """samples (hb * 8, wb * 8) -> quantised coefficients (hb, wb, 64), natural order"""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    x = _fdct_pass(x, True)                                        # rows
    x = _fdct_pass(x.swapaxes(-1, -2), False).swapaxes(-1, -2)     # columns
    x = x.reshape(hb, wb, 64)
    qv = quant.astype(np.int64) << 3
    mag = (np.abs(x) + (qv >> 1)) // qv
    return np.where(x < 0, -mag, mag)


def forward(bgr, quant, sampling):
    """one BGR frame (h, w, 3) (for GREY: only Y is used) -> coef int16, component-planar over the MCU-padded grids"""
    bgr = np.asarray(bgr)
    h, w = bgr.shape[:2]
    fx, fy = reductions(sampling)
    mx, my, grids = geometry(h, w, sampling)
    planes = ycc(bgr)
    out = []
    for c, (gx, gy) in enumerate(grids):
        rx, ry = (1, 1) if c == 0 else (fx, fy)
        real = fdct_quant(component_plane(planes[c], rx, ry), np.asarray(quant)[c])
        hb, wb = real.shape[:2]
        grid = np.zeros((gy, gx, 64), np.int64)
        grid[:hb, :wb] = real
        bw = gx // mx                                              # blocks of this component per MCU, across
        for by in range(gy):
            for bx in range(gx):
                if by < hb and bx >= wb:                           # dummy at the right edge: the block to its left
                    grid[by, bx, 0] = grid[by, bx - 1, 0]
                elif by >= hb:                                     # at the bottom: the last block of the row above, same MCU
                    grid[by, bx, 0] = grid[by - 1, (bx // bw) * bw + bw - 1, 0]
        out.append(grid.reshape(-1))
    coef = np.concatenate(out)
    assert np.abs(coef).max(initial=0) < 32768
    return coef.astype(np.int16)


# ---- entropy coding and headers -----------------------------------------------------------------------------------------
def _code_table(bits, vals):
    """symbol -> (code, length)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class _BitWriter:
    def __init__(self, out, stats):
        self.out, self.acc, self.n, self.stats = out, 0, 0, stats

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
                self.stats["stuffed"] += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _size(v):
    return int(abs(int(v))).bit_length()


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def headers(quant, h, w, sampling, restart_interval):
    grey = sampling == GREY
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    q = np.asarray(quant)
    for t in range(1 if grey else 2):
        out += _segment(0xDB, bytes([t]) + bytes(int(v) for v in q[t][ZIGZAG]))
    fx, fy = reductions(sampling)
    comps = [(1, fx * 16 + fy, 0)] + ([] if grey else [(2, 0x11, 1), (3, 0x11, 1)])
    out += _segment(0xC0, struct.pack(">BHHB", 8, h, w, len(comps)) + b"".join(bytes(c) for c in comps))
    tables = [(0x00, STD_DC_LUMA), (0x10, STD_AC_LUMA)] + ([] if grey else [(0x01, STD_DC_CHROMA), (0x11, STD_AC_CHROMA)])
    for tc_th, (bits, vals) in tables:
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    if restart_interval:
        out += _segment(0xDD, struct.pack(">H", restart_interval))
    sel = [(1, 0x00)] + ([] if grey else [(2, 0x11), (3, 0x11)])
    out += _segment(0xDA, bytes([len(sel)]) + b"".join(bytes(s) for s in sel) + bytes([0, 63, 0]))
    return out


def new_stats():
    return dict(stuffed=0, zrl=0, no_eob=0, eob=0, max_dc_size=0, max_ac_size=0, restarts=0)


def entropy_encode(coef, quant, h, w, sampling, restart_interval=0, stats=None):
    stats = new_stats() if stats is None else stats
    mx, my, grids = geometry(h, w, sampling)
    fx, fy = reductions(sampling)
    coef = np.asarray(coef).reshape(-1, 64).astype(np.int64)
    assert coef.shape[0] == n_blocks(h, w, sampling)
    planes, at = [], 0
    for gx, gy in grids:
        planes.append(coef[at:at + gx * gy].reshape(gy, gx, 64)[:, :, ZIGZAG])
        at += gx * gy
    dc = [_code_table(*STD_DC_LUMA)] + [_code_table(*STD_DC_CHROMA)] * 2
    ac = [_code_table(*STD_AC_LUMA)] + [_code_table(*STD_AC_CHROMA)] * 2
    out = bytearray(headers(quant, h, w, sampling, restart_interval))
    bw = _BitWriter(out, stats)
    pred, since, nrst = [0, 0, 0], 0, 0
    for mcu in range(mx * my):
        if restart_interval and since == restart_interval:
            bw.flush()
            out += bytes([0xFF, 0xD0 + (nrst & 7)])
            nrst += 1
            since, pred = 0, [0, 0, 0]
        since += 1
        mcy, mcx = divmod(mcu, mx)
        for c in range(len(grids)):
            bh, bv = (fx, fy) if c == 0 else (1, 1)
            for v in range(bv):
                for u in range(bh):
                    blk = planes[c][mcy * bv + v, mcx * bh + u]
                    diff = int(blk[0]) - pred[c]
                    pred[c] = int(blk[0])
                    s = _size(diff)
                    stats["max_dc_size"] = max(stats["max_dc_size"], s)
                    bw.put(*dc[c][s])
                    if s:
                        bw.put(diff if diff >= 0 else diff - 1, s)
                    run = 0
                    for k in range(1, 64):
                        val = int(blk[k])
                        if val == 0:
                            run += 1
                            continue
                        while run > 15:
                            bw.put(*ac[c][0xF0])
                            stats["zrl"] += 1
                            run -= 16
                        s = _size(val)
                        stats["max_ac_size"] = max(stats["max_ac_size"], s)
                        bw.put(*ac[c][(run << 4) | s])
                        bw.put(val if val >= 0 else val - 1, s)
                        run = 0
                    if run:
                        bw.put(*ac[c][0])
                        stats["eob"] += 1
                    else:
                        stats["no_eob"] += 1
    bw.flush()
    stats["restarts"] = nrst
    out += b"\xff\xd9"
    return bytes(out)


def encode(bgr, quality, sampling, restart_interval=0, stats=None):
    bgr = np.asarray(bgr)
    q = quant_tables(quality)
    return entropy_encode(forward(bgr, q, sampling), q, bgr.shape[0], bgr.shape[1], sampling, restart_interval, stats)


# ---- the library's bound, restated ----------------------------------------------------------------------------------------
HEADER_BOUND = 1024


def size_bound(h, w, sampling):
    """at most 16 + 10 bits per coefficient, doubled for stuffing, plus 2 bytes per MCU for restart markers and padding,
    plus the headers (623 bytes with every segment) rounded up"""
    mx, my, _ = geometry(h, w, sampling)
    return HEADER_BOUND + n_blocks(h, w, sampling) * 64 * 26 // 8 * 2 + mx * my * 4

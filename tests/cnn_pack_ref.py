"""The classifier's weight packs restated in numpy, from the layout comments of csrc/ck_cnn_pack.cpp and the kernels'
fragment addressing (k_cnn.hip, k_cnn_bf16.hip, k_cnn_q8.hip), for tests/test_cnn_pack_cpu.py.

Every MFMA fragment here is [...][lane 64][elements]: lane = kslot * 16 + column, the k-slot being one of the four
quarter-rows of the K dimension a lane holds and the column an output channel (or output unit) of the 16-wide tile.
A convolution's kernel arrives as Keras [kh][kw][cin][cout] and is flipped in both spatial axes (Theano convolves, the
kernels correlate).  All index arithmetic is on whole arrays; padding elements are zero bytes."""
import numpy as np

PACKS = ("c1w", "c1b", "c2w", "c2b", "c3w", "c3b", "c4w", "c4b", "d1w", "d1b", "d2w", "d2b",
         "c2w_bf", "c3w_bf", "c4w_bf", "c1w_f16", "d1w_bfp",
         "c1w_h2", "c2w_h2", "c3w_h2", "c4w_h2", "d1w_h2", "c1w_q8", "c2x_q8", "c3x_q8", "c4x_q8")

WSCALE = np.float32(256)         # the split and the e4m3 packs hold w x 2^8
SW = np.float32(4)               # block scale 2^2 of the e4m3 weight operands


# ---- encoders --------------------------------------------------------------------------------------------------------
def bf16(x):
    """float32 -> bf16 bits, round to nearest even on the integer (finite values)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def split(w):
    """-> (hi, lo) float16 of w x 2^8: hi the nearest fp16, lo the nearest fp16 of what hi leaves"""
    with np.errstate(over="ignore", invalid="ignore"):
        wv = np.asarray(w, np.float32) * WSCALE
        hi = wv.astype(np.float16)
        lo = (wv - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def e4m3_values():
    """the value of each of the 256 OCP e4m3 codes (0x7F / 0xFF: NaN): 1 sign, 4 exponent bits (bias 7), 3 mantissa bits,
    no infinities, exponent field 0 = subnormals in steps of 2^-9"""
    code = np.arange(256)
    ex, man = (code >> 3) & 15, code & 7
    mag = np.where(ex == 0, man * 2.0 ** -9, (1 + man / 8.0) * 2.0 ** (ex - 7.0))
    mag[(code & 0x7F) == 0x7F] = np.nan
    return np.where(code >= 128, -mag, mag)


def e4m3(v):
    """float -> e4m3 code: the nearest representable magnitude (ties to the even code), saturated at 448, the sign on
    top; exact zero and NaN give code 0"""
    v = np.asarray(v, np.float64)
    mags = e4m3_values()[:0x7F]                                   # codes 0 .. 0x7E ascend from 0 to 448
    a = np.minimum(np.abs(np.nan_to_num(v, nan=0.0)), 448.0)
    up = np.clip(np.searchsorted(mags, a, side="left"), 1, 0x7E)  # mags[up - 1] <= a <= mags[up] (a > 0)
    dn = up - 1
    d_up, d_dn = mags[up] - a, a - mags[dn]
    code = np.where(d_up < d_dn, up, np.where(d_dn < d_up, dn, np.where(up % 2 == 0, up, dn)))
    code = np.where(np.signbit(v), code | 0x80, code)
    return np.where((v == 0) | np.isnan(v), 0, code).astype(np.uint8)


# ---- index maps ------------------------------------------------------------------------------------------------------
def _lane():
    lane = np.arange(64)
    return lane // 16, lane % 16


def _take(src, idx, valid):
    """src (float32, any shape) at the tuple of index arrays `idx` where `valid`, 0.0 elsewhere"""
    idx = np.broadcast_arrays(*idx)
    valid = np.broadcast_to(valid, idx[0].shape)
    safe = tuple(np.where(valid, i, 0) for i in idx)
    return np.where(valid, src[safe], np.float32(0)).astype(np.float32)


def _flip(k):
    return np.ascontiguousarray(k[::-1, ::-1])


def conv_f32(k):
    """B operand of conv_mfma16_f32_kernel: [channel tile][group of 4 k-steps][lane][4]; K runs over (kh, kw, cin padded to
    a multiple of 4), lane (kslot, column) of k-step s holds k = 4 s + kslot"""
    kh, kw, cin, cout = k.shape
    cinp = (cin + 3) // 4 * 4
    ks = kh * kw * cinp // 4
    kslot, col = _lane()
    nt, sg, e = np.ogrid[:(cout + 15) // 16, :(ks + 3) // 4, :4]
    nt, sg, e = nt[..., None], sg[..., None], e[:, :, None, :]          # [nt][sg][lane][e]
    kidx = 4 * (4 * sg + e) + kslot[None, None, :, None]
    tap, c = kidx // cinp, kidx % cinp
    o = nt * 16 + col[None, None, :, None]
    valid = (tap < kh * kw) & (c < cin) & (o < cout)
    return _take(_flip(k), (tap // kw, tap % kw, c, o), valid)


def conv1_f32(k):
    """A operand of conv1_mfma16_kernel: [channel tile 2][step 19][lane]; K = 75 dense in (kh, kw, cin) order, k = 4 step + kslot"""
    kslot, col = _lane()
    n, s = np.ogrid[:2, :19]
    kk = 4 * s[..., None] + kslot
    o = n[..., None] * 16 + col
    return _take(_flip(k).reshape(75, 32), (kk, o), kk < 75)


def fc1_f32(w):
    """A operand of fc1_mfma16_kernel: [output tile 10][pair of k-steps 405][lane][2], k = 4 step + kslot"""
    kslot, col = _lane()
    nt, sg = np.ogrid[:10, :405]
    e = np.arange(2)
    k = 4 * (2 * sg[..., None, None] + e) + kslot[:, None]
    o = nt[..., None, None] * 16 + col[:, None]
    return _take(w, (k, o), True)


def conv_k32(k, cinp, couts):
    """source values in the 16-bit fragment order [channel tile][k-step][lane][8]: a k-step is 32 input channels of one
    kernel tap (step = tap * cinp / 32 + block), lane (kslot, channel) holds the 8 consecutive cin from 32 block + 8 kslot"""
    kh, kw, cin, cout = k.shape
    nb = cinp // 32
    kslot, col = _lane()
    nt, st = np.ogrid[:couts // 16, :kh * kw * nb]
    nt, st = nt[..., None, None], st[..., None, None]
    tap, cc = st // nb, st % nb
    c = 32 * cc + 8 * kslot[:, None] + np.arange(8)
    o = nt * 16 + col[:, None]
    return _take(_flip(k), (tap // kw, tap % kw, c, o), (c < cin) & (o < cout))


def conv1_rows(k):
    """conv1 in conv12_bf16_kernel's fragment order [channel tile 2][k-step 4][lane][8]: the 15 (kernel row, pair of kernel
    columns) units f = 3 row + pair, f = 4 step + kslot; the 8 elements are two columns x cin padded 3 -> 4"""
    kslot, col = _lane()
    nt, s = np.ogrid[:2, :4]
    nt, s = nt[..., None, None], s[..., None, None]
    e = np.arange(8)
    f = 4 * s + kslot[:, None]
    j, c = 2 * (f % 3) + e // 4, e % 4
    o = nt * 16 + col[:, None]
    return _take(_flip(k), (f // 3, j, c, o), (f < 15) & (j < 5) & (c < 3))


def conv1_h2_rows(k):
    """conv1 for the fused conv1 + conv2 kernel of the split mode, [channel tile 2][step 3][lane][8]: kernel row 2 step + kslot / 2,
    and within the row the 15 (kw, cin) slots, slot = 8 (kslot % 2) + e"""
    kslot, col = _lane()
    nt, st = np.ogrid[:2, :3]
    nt, st = nt[..., None, None], st[..., None, None]
    i = 2 * st + kslot[:, None] // 2
    slot = 8 * (kslot[:, None] % 2) + np.arange(8)
    o = nt * 16 + col[:, None]
    return _take(_flip(k), (i, slot // 3, slot % 3, o), (i < 5) & (slot < 15))


def fc1_k32(w, padded):
    """dense 1 as [output tile 10][k-step][lane][8], k = 32 step + 8 kslot + e; `padded`: k counts over the bf16 maps
    [pixel 36][channel 96] (108 steps), else over the 3240 inputs themselves (104 steps, the tail zero)"""
    kslot, col = _lane()
    t, st = np.ogrid[:10, :108 if padded else 104]
    t, st = t[..., None, None], st[..., None, None]
    k = 32 * st + 8 * kslot[:, None] + np.arange(8)
    o = 16 * t + col[:, None]
    if padded:
        return _take(w, ((k // 96) * 90 + k % 96, o), k % 96 < 90)
    return _take(w, (k, o), k < 3240)


# the units (kernel row, kernel column, block of 32 input channels) of every scaled MFMA's two halves, None = empty half
def _pairs2():
    rows = [[((i, 0, 0), (i, 1, 0)), ((i, 2, 0), (i, 3, 0)), ((i, 4, 0), None)] for i in range(5)]       # fragment 3 i + pair
    return sum(rows, []) + [((0, 4, 0), (1, 4, 0)), ((2, 4, 0), (3, 4, 0)), ((4, 4, 0), None)]            # last column, vertical


def _pairs3():
    rows = [[((i, 0, 0), (i, 1, 0)), ((i, 2, 0), None)] for i in range(3)]                                # fragment 2 i + pair
    return sum(rows, []) + [((0, 2, 0), (1, 2, 0)), ((2, 2, 0), None)]


def _pairs4():
    unit = lambda s: (s // 9, (s // 3) % 3, s % 3)             # k-step = tap * 3 + channel block
    return [(unit(2 * u), unit(2 * u + 1) if 2 * u + 1 < 27 else None) for u in range(14)]


def cross(k, ntile, pairs):
    """e4m3 cross-term operand [channel tile][unit pair][lane][32 bytes]: bytes 0..15 the pair's first unit, 16..31 its
    second; lane = group * 16 + output channel; groups 0 / 1 hold w_lo x 2^11 / 4 of the unit's input channels 0..15 / 16..31,
    groups 2 / 3 hold w_hi / 4 of the same"""
    kh, kw, cin, cout = k.shape
    unit = np.array([[un if un else (-1, 0, 0) for un in p] for p in pairs])           # [pair][half][3]
    ui, uj, ucc = (unit[None, :, None, :, None, n] for n in range(3))                  # [nt][pair][lane][half][e]
    g, col = _lane()
    g, col = g[None, None, :, None, None], col[None, None, :, None, None]
    c = 32 * ucc + 16 * (g & 1) + np.arange(16)
    o = np.arange(ntile)[:, None, None, None, None] * 16 + col
    valid = (ui >= 0) & (c < cin) & (o < cout)
    hi, lo = split(_take(_flip(k), (ui, uj, c, o), valid))
    term = np.where(g < 2, lo.astype(np.float32) * np.float32(2048) / SW, hi.astype(np.float32) / SW)
    return np.where(valid, e4m3(term), 0).astype(np.uint8).reshape(ntile, len(pairs), 64, 32)


def _planes(src, axis):
    """the hi and lo planes of a fragment array stacked along a new axis"""
    return np.stack(split(src), axis=axis)


def pack_all(W):
    """W: dict of the twelve float32 arrays -> (dict pack name -> bytes, q8_ok)"""
    W = {k: np.ascontiguousarray(v, np.float32) for k, v in W.items()}
    out = {k: W[k] for k in ("c1b", "c2b", "c3b", "c4b", "d1b", "d2w", "d2b")}
    out["c1w"] = conv1_f32(W["c1w"])
    out["c2w"], out["c3w"], out["c4w"] = conv_f32(W["c2w"]), conv_f32(W["c3w"]), conv_f32(W["c4w"])
    out["d1w"] = fc1_f32(W["d1w"])
    out["c2w_bf"] = bf16(conv_k32(W["c2w"], 32, 32))
    out["c3w_bf"] = bf16(conv_k32(W["c3w"], 32, 96))
    out["c4w_bf"] = bf16(conv_k32(W["c4w"], 96, 96))
    out["c1w_f16"] = conv1_rows(W["c1w"]).astype(np.float16)
    out["d1w_bfp"] = bf16(fc1_k32(W["d1w"], True))
    out["c1w_h2"] = _planes(conv1_h2_rows(W["c1w"]), 2)              # [tile][step][plane][lane][8]
    out["c2w_h2"] = _planes(conv_k32(W["c2w"], 32, 32), 2)
    out["c3w_h2"] = _planes(conv_k32(W["c3w"], 32, 96), 2)
    out["c4w_h2"] = _planes(conv_k32(W["c4w"], 96, 96), 2)
    out["d1w_h2"] = _planes(fc1_k32(W["d1w"], False), 2)
    out["c1w_q8"] = _planes(conv1_rows(W["c1w"]), 0)                 # [plane][tile][step][lane][8]
    out["c2x_q8"] = cross(W["c2w"], 2, _pairs2())
    out["c3x_q8"] = cross(W["c3w"], 6, _pairs3())
    out["c4x_q8"] = cross(W["c4w"], 6, _pairs4())
    biggest = max(float(np.abs(split(W[k])[0].astype(np.float32)).max()) for k in ("c2w", "c3w", "c4w"))
    return {k: np.ascontiguousarray(out[k]).tobytes() for k in PACKS}, biggest <= 448.0 * float(SW)

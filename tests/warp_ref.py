"""Plain references for K7 (ck_get_perspective_transform) and K8 (warp_kernel), used by tests/test_perspective_cpu.py
and tests/test_gpu_warp.py.

`reference` is the warp as the operation is defined, not as the library evaluates it: M inverted exactly (rationals,
rounded once to float64), each destination pixel's source coordinate computed on its own (no 64 x 16 blocks), 32.x and
32.y rounded half-to-even, bilinear interpolation of the four taps with a zero border, rounded half up.  Where 32.x or
32.y lies within `band` of a .5 boundary, evaluation order decides the tap, so both neighbouring taps are candidates.

`kernel_taps` is the other side: the library's own evaluation order (inverse by adjugate, block-associated sums,
`W ? 32 / W : 0`, the int and short clamps) restated in numpy float64.  numpy rounds every operation and never fuses
a multiply-add, as k_warp.hip (`fp contract(off)`) and ck_host_geom.cpp (`-ffp-contract=off`) do, so it reproduces
the kernel's taps bit for bit.  With form="direct" or "bx0" it evaluates the same sums in another order; `flip_search`
uses that to find transforms on which the order changes a tap, which only such transforms can show."""
from fractions import Fraction

import numpy as np

SHORT_MIN, SHORT_MAX = -32768, 32767
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def host_inverse(M):
    """ck_invert3x3 (and the oracle's invert3x3): adjugate times 1/det, zeros when det == 0"""
    s = [float(v) for v in np.asarray(M, np.float64).reshape(9)]
    det = s[0] * (s[4] * s[8] - s[5] * s[7]) - s[1] * (s[3] * s[8] - s[5] * s[6]) + s[2] * (s[3] * s[7] - s[4] * s[6])
    if det == 0:
        return np.zeros(9)
    det = 1. / det
    return np.array([(s[4] * s[8] - s[5] * s[7]) * det, (s[2] * s[7] - s[1] * s[8]) * det, (s[1] * s[5] - s[2] * s[4]) * det,
                     (s[5] * s[6] - s[3] * s[8]) * det, (s[0] * s[8] - s[2] * s[6]) * det, (s[2] * s[3] - s[0] * s[5]) * det,
                     (s[3] * s[7] - s[4] * s[6]) * det, (s[1] * s[6] - s[0] * s[7]) * det, (s[0] * s[4] - s[1] * s[3]) * det])


def exact_inverse(M):
    """M^-1 in rationals, each entry rounded once to float64; zeros for a singular M (the library's rule: cv::invert
    leaves zeros when det == 0, and the warp then maps every pixel to source (0, 0))"""
    s = [Fraction(float(v)) for v in np.asarray(M, np.float64).reshape(9)]
    det = s[0] * (s[4] * s[8] - s[5] * s[7]) - s[1] * (s[3] * s[8] - s[5] * s[6]) + s[2] * (s[3] * s[7] - s[4] * s[6])
    if det == 0:
        return np.zeros(9)
    adj = [s[4] * s[8] - s[5] * s[7], s[2] * s[7] - s[1] * s[8], s[1] * s[5] - s[2] * s[4],
           s[5] * s[6] - s[3] * s[8], s[0] * s[8] - s[2] * s[6], s[2] * s[3] - s[0] * s[5],
           s[3] * s[7] - s[4] * s[6], s[1] * s[6] - s[0] * s[7], s[0] * s[4] - s[1] * s[3]]
    return np.array([float(a / det) for a in adj])


def _grid(dsize):
    dy, dx = np.mgrid[0:dsize, 0:dsize]
    return dx.astype(np.float64), dy.astype(np.float64)


def kernel_taps(Minv, dsize, form="block"):
    """(X, Y): the kernel's source coordinates in 1/32 px (int64, before the >> 5), from the inverse it uses.
    form "block": (X0 + M0*x1) * (32/W) with X0 = M0*bx + M1*dy + M2 at the block origin bx, as k_warp.hip;
    "bx0": the same with every block at bx = 0; "direct": (M0*dx + M1*dy + M2) * (32/W)."""
    m = np.asarray(Minv, np.float64).reshape(9)
    dx, dy = _grid(dsize)
    bh0 = min(16, dsize)
    bw0 = min(1024 // bh0, dsize)
    if form == "direct":
        X = m[0] * dx + m[1] * dy + m[2]
        Y = m[3] * dx + m[4] * dy + m[5]
        W = m[6] * dx + m[7] * dy + m[8]
    else:
        bx = np.floor(dx / bw0) * bw0 if form == "block" else np.zeros_like(dx)
        x1 = dx - bx
        X = (m[0] * bx + m[1] * dy + m[2]) + m[0] * x1
        Y = (m[3] * bx + m[4] * dy + m[5]) + m[3] * x1
        W = (m[6] * bx + m[7] * dy + m[8]) + m[6] * x1
    nz = W != 0
    q = np.zeros_like(W)
    q[nz] = 32.0 / W[nz]
    with np.errstate(invalid="ignore", over="ignore"):
        fX, fY = X * q, Y * q
    return (np.rint(np.clip(fX, INT_MIN, INT_MAX)).astype(np.int64),
            np.rint(np.clip(fY, INT_MIN, INT_MAX)).astype(np.int64))


def bilinear(src, X, Y):
    """the destination image from taps in 1/32 px: four neighbours, weights (32 - f) / 32 and f / 32 per axis, zero
    outside the frame, the weighted sum rounded half up"""
    src = np.asarray(src)
    h, w = src.shape[:2]
    sx = np.clip(X >> 5, SHORT_MIN, SHORT_MAX)
    sy = np.clip(Y >> 5, SHORT_MIN, SHORT_MAX)
    fx, fy = X & 31, Y & 31
    acc = np.zeros(X.shape + (3,), np.int64)
    for oy, wy in ((0, 32 - fy), (1, fy)):
        for ox, wx in ((0, 32 - fx), (1, fx)):
            yy, xx = sy + oy, sx + ox
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            v = src[np.where(inside, yy, 0), np.where(inside, xx, 0)].astype(np.int64)
            acc += np.where(inside, wy * wx, 0)[..., None] * v
    return ((acc + 512) >> 10).astype(np.uint8)


def emulate(src, M, dsize, form="block"):
    """the kernel's output restated: host inverse, `form` evaluation order, bilinear"""
    return bilinear(src, *kernel_taps(host_inverse(M), dsize, form))


def reference(src, M, dsize, band=1e-6):
    """-> (candidates (k, dsize, dsize, 3), number of pixels with a coordinate in the band).  A correct warp equals
    candidates[j] at each pixel for some j.  band=0: the transform's arithmetic is exact (dyadic), one candidate."""
    m = exact_inverse(M)
    dx, dy = _grid(dsize)
    X = m[0] * dx + m[1] * dy + m[2]
    Y = m[3] * dx + m[4] * dy + m[5]
    W = m[6] * dx + m[7] * dy + m[8]
    nz = W != 0
    u, v = np.zeros_like(W), np.zeros_like(W)
    with np.errstate(over="ignore"):
        u[nz] = 32.0 * (X[nz] / W[nz])
        v[nz] = 32.0 * (Y[nz] / W[nz])
    u, v = np.clip(u, INT_MIN, INT_MAX), np.clip(v, INT_MIN, INT_MAX)
    taps, near = [], np.zeros(W.shape, bool)
    for c in (u, v):
        lo = np.floor(c)
        nb = np.abs(c - lo - 0.5) < band
        near |= nb
        r = np.rint(c)
        taps.append((r.astype(np.int64), np.where(nb, lo, r).astype(np.int64), np.where(nb, lo + 1, r).astype(np.int64)))
    (ux, lx, hx), (uy, ly, hy) = taps
    cands = [bilinear(src, ux, uy)]
    if near.any():
        cands += [bilinear(src, a, b) for a in (lx, hx) for b in (ly, hy)]
    return np.stack(cands), int(near.sum())


def mismatch(out, cands):
    """pixels of `out` that equal no candidate (all three channels from one candidate)"""
    ok = np.zeros(out.shape[:2], bool)
    for c in cands:
        ok |= (c == out).all(-1)
    return ~ok


def flip_search(dsize=380, want=3):
    """affine transforms whose taps change with the evaluation order.  M = s*I plus a translation of k*s/64 px: the
    inverse scales by 1/s (inexact in binary) and sets every s-th pixel on a .5 tie of the 1/32 grid in exact
    arithmetic, where the rounding errors of each order decide the side.  -> [(M, taps block != direct, block != bx0)]
    for the first `want` with both counts positive"""
    found = []
    for s in (3, 5, 7, 11, 6, 10, 12):
        for k in (-7, -3, 1, 5, 3, 7):
            M = np.array([[s, 0, k * s / 64], [0, s, -k * s / 64 + s / 128], [0, 0, 1]], np.float64)
            m = host_inverse(M)
            b, d, z = (kernel_taps(m, dsize, f) for f in ("block", "direct", "bx0"))
            nd = int(((b[0] != d[0]) | (b[1] != d[1])).sum())
            nz = int(((b[0] != z[0]) | (b[1] != z[1])).sum())
            if nd and nz:
                found.append((M, nd, nz))
                if len(found) == want:
                    return found
                break
    return found


# degenerate quads for K7: three corners on one line, corner 1 among them (the one tests lift by d px off the line).
# Horizontal lines: the x axis away from the origin, the x axis through it, y = -3.  Slanted lines (slopes 0.33, 0.5,
# 1), where elimination meets no exact zero, as on a real near-degenerate board.
COLLINEAR = [[(-200, 0), (13, 0), (217, 0), (-50, 300)],
             [(40, 500), (0, 0), (300, 0), (600, 0)],
             [(0, -3), (250, -3), (500, -3), (100, 400)],
             [(10, 20), (110, 53), (310, 119), (40, 400)],
             [(100, 100), (200, 150), (400, 250), (50, 400)],
             [(17, 3), (117, 103), (317, 303), (600, 10)]]


def exact_perspective(src4, dst4):
    """the 8 x 8 system of getPerspectiveTransform solved in rationals from the float32 corners -> 9 Fractions (M[8] = 1),
    or None when the system is singular"""
    src = np.asarray(src4, np.float32).reshape(4, 2)
    dst = np.asarray(dst4, np.float32).reshape(4, 2)
    a = []
    for i in range(4):
        sx, sy = Fraction(float(src[i, 0])), Fraction(float(src[i, 1]))
        dx, dy = Fraction(float(dst[i, 0])), Fraction(float(dst[i, 1]))
        a.append([sx, sy, 1, 0, 0, 0, -sx * dx, -sy * dx, dx])
        a.append([0, 0, 0, sx, sy, 1, -sx * dy, -sy * dy, dy])
    a = [[Fraction(v) for v in row] for row in a]
    for c in range(8):
        piv = next((r for r in range(c, 8) if a[r][c] != 0), None)
        if piv is None:
            return None
        a[c], a[piv] = a[piv], a[c]
        for r in range(8):
            if r != c and a[r][c] != 0:
                f = a[r][c] / a[c][c]
                a[r] = [x - f * y for x, y in zip(a[r], a[c])]
    return [a[i][8] / a[i][i] for i in range(8)] + [Fraction(1)]

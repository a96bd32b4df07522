"""Plain references for K3..K6 (k_contours.hip, k_board_lines) that share no code with the oracle or the kernels.

* External contours from scipy.ndimage.label, by the set definition: clear the 1-px frame; label the edge pixels
  8-connected and the background 4-connected; S0 is the background component that holds the frame; a component is
  top-level when one of its pixels is 4-adjacent to S0, and those pixels are its outer border.  The discovery key is
  the component's first pixel in raster order; cv2.findContours hands contours back in reverse discovery order.
* minAreaRect area in float64: scipy ConvexHull, every hull-edge orientation.  Collinear points, or fewer than 3
  distinct ones, give 0.
* Selection as bf_auto.py does it: bisect.insort in cv2 order, the top three s[-3:], the gate h*w/3 < s[-1].area; the
  ghost is the outer borders of the three.
* cv2.HoughLines(ghost, 1, pi/180, thr) as OpenCV 3.1 computes it, vectorised: float32 tables built by ang += theta,
  votes at rint(f32(x*cos) + f32(y*sin)), a zero guard cell around the accumulator, the > / >= peak test, peaks sorted
  by votes descending then accumulator index ascending, rho and theta in float32.

_hough_naive and _min_area_brute are the loop forms the vectorised ones are checked against."""
import bisect
import math

import numpy as np
from scipy import ndimage

NUMANGLE = 180
THETA = np.float32(math.pi / 180)
LINES, NO_CONTOUR, TOO_SMALL = 0, 1, 2            # ck_board_result.status


# ---------------------------------------------------------------- K3 external contours
def external_contours(edges):
    """-> list of dicts {key: first pixel (raster index), ys, xs: the outer border} in DISCOVERY order"""
    e = np.asarray(edges) != 0
    e[0, :] = e[-1, :] = e[:, 0] = e[:, -1] = False
    lab, n = ndimage.label(e, structure=np.ones((3, 3), bool))
    if n == 0:
        return []
    bg, _ = ndimage.label(~e)                                    # 4-connected
    s0 = bg == bg[0, 0]
    near = np.zeros_like(s0)
    near[1:, :] |= s0[:-1, :]
    near[:-1, :] |= s0[1:, :]
    near[:, 1:] |= s0[:, :-1]
    near[:, :-1] |= s0[:, 1:]
    border = e & near
    flat = lab.ravel()
    ids, first = np.unique(flat, return_index=True)
    key = dict(zip(ids.tolist(), first.tolist()))
    blab = lab[border]
    by, bx = np.nonzero(border)
    order = np.argsort(blab, kind="stable")
    blab, by, bx = blab[order], by[order], bx[order]
    tops, starts = np.unique(blab, return_index=True)
    ends = list(starts[1:]) + [len(blab)]
    out = [dict(key=key[int(c)], ys=by[s:t], xs=bx[s:t]) for c, s, t in zip(tops, starts, ends)]
    out.sort(key=lambda c: c["key"])
    return out


def hull_candidates(edges):
    """[h][w] bool: the outer-border pixels without two opposite edge neighbours (8 directions, frame cleared) -- the
    points k_board_lines gathers for the calipers: a pixel in the middle of a straight run is no hull vertex"""
    e = np.asarray(edges) != 0
    e[0, :] = e[-1, :] = e[:, 0] = e[:, -1] = False
    h, w = e.shape
    border = np.zeros_like(e)
    for c in external_contours(edges):
        border[c["ys"], c["xs"]] = True
    p = np.pad(e, 1)
    nb = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    mid = (nb(0, -1) & nb(0, 1)) | (nb(-1, 0) & nb(1, 0)) | (nb(-1, -1) & nb(1, 1)) | (nb(-1, 1) & nb(1, -1))
    return border & ~mid


# ---------------------------------------------------------------- K4 minAreaRect
def min_area(xs, ys):
    """float64 area of the minimum-area enclosing rectangle of the points"""
    pts = np.unique(np.stack([np.asarray(xs, np.float64), np.asarray(ys, np.float64)], 1), axis=0)
    if len(pts) < 3:
        return 0.0
    from scipy.spatial import ConvexHull, QhullError
    try:
        hull = pts[ConvexHull(pts).vertices]
    except QhullError:                                           # collinear
        return 0.0
    d = np.roll(hull, -1, 0) - hull
    d /= np.linalg.norm(d, axis=1)[:, None]
    u = hull @ d.T                                               # [point, edge]
    v = hull @ np.stack([-d[:, 1], d[:, 0]], 1).T
    return float(((u.max(0) - u.min(0)) * (v.max(0) - v.min(0))).min())


def _min_area_brute(pts):
    pts = np.unique(np.asarray(pts, np.float64), axis=0)
    if len(pts) < 3:
        return 0.0
    from scipy.spatial import ConvexHull, QhullError
    try:
        hull = pts[ConvexHull(pts).vertices]
    except QhullError:
        return 0.0
    best = np.inf
    for i in range(len(hull)):
        d = hull[(i + 1) % len(hull)] - hull[i]
        d /= np.linalg.norm(d)
        nrm = np.array([-d[1], d[0]])
        u, v = hull @ d, hull @ nrm
        best = min(best, (u.max() - u.min()) * (v.max() - v.min()))
    return best


# ---------------------------------------------------------------- K4 selection
class _Box:
    def __init__(self, area, pos):
        self.area, self.pos = area, pos

    def __lt__(self, other):
        return self.area < other.area


def select(areas_cv):
    """areas in cv2 order -> (positions of s[-3:] in cv2 order, s[-1].area, the insort list's areas)"""
    s = []
    for i, a in enumerate(areas_cv):
        bisect.insort(s, _Box(a, i))
    return [b.pos for b in s[-3:]], s[-1].area, [b.area for b in s]


def round_wants(rnd, ub, area, known):
    """which components k_board_lines measures in exact-area round `rnd` -> (must, may, count): it takes `count`
    components, all of `must` and the rest from `may`.  Round 0: the 16 largest bounding boxes `ub` among the unknown
    components (boxes equal to the 16th may stand in for each other); later rounds: every unknown component whose box,
    times 1 + 1e-5, reaches the third best known area (-1 while fewer than three are known)."""
    unknown = [s for s in range(len(ub)) if not known[s]]
    if rnd == 0:
        k = min(16, len(unknown))
        if k == 0:
            return set(), set(), 0
        cut = sorted((ub[s] for s in unknown), reverse=True)[k - 1]
        return {s for s in unknown if ub[s] > cut}, {s for s in unknown if ub[s] == cut}, k
    best = sorted((area[s] for s in range(len(ub)) if known[s]), reverse=True)
    third = best[2] if len(best) >= 3 else -1.0
    must = {s for s in unknown if ub[s] * (1.0 + 1e-5) >= third}
    return must, set(), len(must)


def peaks(img, thr):
    """the peaks of hough_accum(img) as (accumulator index, votes) pairs, int32 [k][2], in raster order of the cells"""
    acc = hough_accum(img)
    n, r = np.nonzero(peak_mask(acc, thr))
    return np.stack([(n + 1) * acc.shape[1] + r + 1, acc[n + 1, r + 1]], 1).astype(np.int32).reshape(-1, 2)


# ---------------------------------------------------------------- K6 HoughLines
def trig_tables():
    ang = np.float32(0)
    ts, tc = [], []
    for _ in range(NUMANGLE):
        ts.append(np.float32(math.sin(float(ang))))
        tc.append(np.float32(math.cos(float(ang))))
        ang = np.float32(ang + THETA)
    return np.array(tc, np.float32), np.array(ts, np.float32)


def hough_accum(img):
    """-> int32 accumulator [NUMANGLE + 2][numrho + 2] with its zero guard cells"""
    h, w = img.shape
    numrho = 2 * (w + h) + 1
    tc, ts = trig_tables()
    ys, xs = np.nonzero(img)
    acc = np.zeros((NUMANGLE + 2) * (numrho + 2), np.int64)
    rows = np.arange(1, NUMANGLE + 1, dtype=np.int64)[:, None] * (numrho + 2)
    for k in range(0, len(xs), 8192):
        x = xs[k:k + 8192].astype(np.float32)
        y = ys[k:k + 8192].astype(np.float32)
        s = (tc[:, None] * x[None, :]) + (ts[:, None] * y[None, :])   # float32 products, float32 sum
        assert s.dtype == np.float32
        r = np.rint(s).astype(np.int64) + (numrho - 1) // 2
        acc += np.bincount((rows + r + 1).ravel(), minlength=acc.size)
    return acc.reshape(NUMANGLE + 2, numrho + 2).astype(np.int32)


def peak_mask(acc, thr):
    """[NUMANGLE][numrho] bool: cv2's local-maximum test on the inner cells"""
    c = acc[1:-1, 1:-1]
    return ((c > thr) & (c > acc[1:-1, :-2]) & (c >= acc[1:-1, 2:]) & (c > acc[:-2, 1:-1]) & (c >= acc[2:, 1:-1]))


def hough_lines(img, thr, want_accum=False):
    h, w = img.shape
    numrho = 2 * (w + h) + 1
    acc = hough_accum(img)
    n, r = np.nonzero(peak_mask(acc, thr))
    idx = (n + 1) * (numrho + 2) + r + 1
    order = np.lexsort((idx, -acc[n + 1, r + 1]))
    n, r = n[order], r[order]
    lines = np.stack([r.astype(np.float32) - np.float32(numrho - 1) * np.float32(0.5),
                      np.float32(0) + n.astype(np.float32) * THETA], 1).astype(np.float32).reshape(-1, 2)
    return (lines, acc) if want_accum else lines


def _hough_naive(img, thr):
    h, w = img.shape
    theta = np.float32(math.pi / 180)
    numangle, numrho = 180, 2 * (w + h) + 1
    ang = np.float32(0)
    ts, tc = [], []
    for _ in range(numangle):
        ts.append(np.float32(math.sin(float(ang))))
        tc.append(np.float32(math.cos(float(ang))))
        ang = np.float32(ang + theta)
    ts, tc = np.array(ts, np.float32), np.array(tc, np.float32)
    acc = np.zeros((numangle + 2, numrho + 2), np.int32)
    ys, xs = np.nonzero(img)
    for y, x in zip(ys, xs):
        v = (np.float32(x) * tc + np.float32(y) * ts).astype(np.float32)
        r = np.rint(v.astype(np.float64)).astype(np.int64) + (numrho - 1) // 2
        acc[np.arange(1, numangle + 1), r + 1] += 1
    peaks = []
    for r in range(numrho):
        for n in range(numangle):
            a = acc[n + 1, r + 1]
            if a > thr and a > acc[n + 1, r] and a >= acc[n + 1, r + 2] and a > acc[n, r + 1] and a >= acc[n + 2, r + 1]:
                peaks.append((-int(a), (n + 1) * (numrho + 2) + r + 1, r, n))
    peaks.sort()
    lines = [((np.float32(r) - np.float32(numrho - 1) * np.float32(0.5)), np.float32(0) + np.float32(n) * theta)
             for _, _, r, n in peaks]
    return np.array(lines, np.float32).reshape(-1, 2), acc


# ---------------------------------------------------------------- K3..K6
def board_lines(edges, thr=None, tol=1e-5):
    """-> dict(status, n_contours, biggest_area, ghost, lines, areas, close): status as ck_board_result; `areas` the
    float64 areas in cv2 order; `close` says that the 3rd and 4th areas of the insort list (other than two zeros), or
    the biggest area and the gate, lie within `tol` (relative): there the kernel's float32 calipers may rank otherwise.
    Exact ties count as close: congruent shapes in other positions or orientations need not get equal float32 areas."""
    edges = np.asarray(edges)
    h, w = edges.shape
    if thr is None:
        thr = int(min(h, w) / 5)
    cs = external_contours(edges)[::-1]                          # cv2 order
    ghost = np.zeros((h, w), np.uint8)
    out = dict(n_contours=len(cs), biggest_area=0.0, ghost=ghost, lines=np.zeros((0, 2), np.float32), areas=[],
               close=False)
    if not cs:
        out["status"] = NO_CONTOUR
        return out
    areas = [min_area(c["xs"], c["ys"]) for c in cs]
    pos, big, s = select(areas)
    out.update(areas=areas, biggest_area=big)
    gate = h * w / 3
    near = lambda a, b: abs(a - b) <= tol * max(abs(a), abs(b), 1.0)
    out["close"] = (len(s) > 3 and near(s[-3], s[-4]) and s[-3] != 0.0) or near(big, gate)   # (area 0 is exact)
    if not gate < big:
        out["status"] = TOO_SMALL
        return out
    for p in pos:
        ghost[cs[p]["ys"], cs[p]["xs"]] = 255
    out["status"] = LINES
    out["lines"] = hough_lines(ghost, thr)
    return out


# ---------------------------------------------------------------- Hough slab geometry of k_board_lines
def hough_slab(n, h, w, small_n=32, threads=1024):
    """(rb, threads) as k_board_lines picks them: S = w + h + 2 dwords per LDS row of 16-bit counters,
    rb = min(10, 36864 // S - 2) on a 144 KB slab; a call of at most `small_n` frames takes min(rb, 18432 // S - 2)
    rows on a 72 KB slab with 512 threads when that is at least 1"""
    S = w + h + 2
    rb = min(10, 36864 // S - 2)
    if n <= small_n and 18432 // S - 2 >= 1:
        return min(rb, 18432 // S - 2), min(threads, 512)
    return rb, threads


def slab_classes(acc, thr, rb):
    """which slab-edge situations the accumulator's peaks meet, for a slab of rb theta rows"""
    numrho = acc.shape[1] - 2
    pk = peak_mask(acc, thr)
    n, r = np.nonzero(pk)
    c = acc[1:-1, 1:-1]
    last = (n % rb == rb - 1) | (n == NUMANGLE - 1)
    first = n % rb == 0
    # a cell above the threshold and the cell below it, in the next slab, with the same count: the halo row decides
    nb = np.arange(rb - 1, NUMANGLE - 1, rb)
    tie = (c[nb] > thr) & (c[nb] == c[nb + 1]) & ((c[nb] > acc[1:-1, :-2][nb]) | (c[nb + 1] > acc[1:-1, :-2][nb + 1]))
    partial = NUMANGLE % rb != 0 and bool((n >= NUMANGLE - NUMANGLE % rb).any())
    return dict(first_row=bool(first.any()), last_row=bool(last.any()), tie_across=bool(tie.any()),
                theta_0_179=bool(((n == 0) | (n == NUMANGLE - 1)).any()), partial_slab=partial,
                rho_negative=bool((r < (numrho - 1) // 2).any()))


# ---------------------------------------------------------------- edge maps
def draw_line(e, x0, y0, x1, y1):
    """a 1-px 8-connected segment, clipped to the image"""
    k = int(max(abs(x1 - x0), abs(y1 - y0))) + 1
    xs = np.rint(np.linspace(x0, x1, k)).astype(np.int64)
    ys = np.rint(np.linspace(y0, y1, k)).astype(np.int64)
    ok = (xs >= 0) & (xs < e.shape[1]) & (ys >= 0) & (ys < e.shape[0])
    e[ys[ok], xs[ok]] = 255
    return e


def outline(e, y0, x0, y1, x1):
    """a closed axis-aligned rectangle through pixel centres (y0, x0) .. (y1, x1): minAreaRect area (y1-y0)(x1-x0)"""
    e[y0, x0:x1 + 1] = e[y1, x0:x1 + 1] = 255
    e[y0:y1 + 1, x0] = e[y0:y1 + 1, x1] = 255
    return e


def slab_map(rng, h, w):
    """an outline open at the top (the gate passes; the interior is S0) and two or three stars of 1-px rays at random
    angles: no line meets the frame, and a ray near the vertical gives peaks at theta 179"""
    e = np.zeros((h, w), np.uint8)
    e[3:h - 3, 3] = e[3:h - 3, w - 4] = 255
    e[h - 4, 3:w - 3] = 255
    for _ in range(int(rng.integers(2, 4))):
        cy, cx = rng.integers(6, h - 6), rng.integers(6, w - 6)
        for _ in range(int(rng.integers(2, 5))):
            a = rng.uniform(0, np.pi) if rng.random() < 0.7 else np.pi / 2 + rng.uniform(-0.03, 0.03)
            ln = rng.uniform(0.3, 1.5) * max(h, w)
            s = rng.choice([-1, 1])
            draw_line(e, cx, cy, cx + s * ln * math.cos(a), cy + s * ln * math.sin(a))
    e[:2, :] = e[-2:, :] = 0
    e[:, :2] = e[:, -2:] = 0
    return e


def equal_combs(h=100, w=200):
    """four combs of equal minAreaRect area (88 x 88, axis-aligned hulls: exact in float32) at different raster
    positions, interleaved in pairs without touching; the gate (h*w/3) passes"""
    e = np.zeros((h, w), np.uint8)
    for x0 in (4, 104):
        y0, A, B = 4, 88, 88
        e[y0, x0:x0 + B + 1] = 255                           # top bar, teeth down
        e[y0:y0 + A + 1, x0:x0 + B + 1:4] = 255
        e[y0 + A + 2, x0 + 2:x0 + B + 3] = 255               # bottom bar, teeth up
        e[y0 + 2:y0 + A + 3, x0 + 2:x0 + B + 3:4] = 255
    return e


GATE_HW = (40, 42)                                           # h*w/3 = 560 = 16 * 35, and 561 = 17 * 33


def gate_map(above):
    """one outline of area exactly h*w/3 (TOO_SMALL), or of the next integer area (LINES), plus a stroke"""
    e = np.zeros(GATE_HW, np.uint8)
    if above:
        outline(e, 3, 3, 3 + 17, 3 + 33)
    else:
        outline(e, 3, 3, 3 + 16, 3 + 35)
    e[30, 5:30] = 255
    return e


def decoy_map(k=17, h=100, w=240):
    """k parallel 45-degree strokes (minAreaRect area 0, bounding box 93 x 93) beside an outline of area 85 x 95 that
    passes the gate: the strokes' boxes beat the outline's, so the first round of exact areas holds only strokes"""
    e = np.zeros((h, w), np.uint8)
    for i in range(k):
        draw_line(e, 3 + 3 * i, 3, 3 + 3 * i + 93, 96)
    outline(e, 2, 150, 97, 235)
    e[50, 160:220] = 255
    return e


def comb(h, w, step):
    """1-px vertical teeth every `step` columns joined by one horizontal stroke: every tooth pixel touches background
    that reaches the frame, so the whole comb is outer border"""
    e = np.zeros((h, w), np.uint8)
    e[2:h - 2, 2:w - 2:step] = 255
    e[2, 2:w - 2] = 255
    return e


def zigzag(h, w):
    """horizontal zigzag strokes, the pixels (x, y0 + (x & 1)), one every third row, joined by one column at the left
    into a single component: every stroke pixel is outer border and has no two opposite neighbours"""
    e = np.zeros((h, w), np.uint8)
    xs = np.arange(3, w - 3)
    for y0 in range(3, h - 4, 3):
        e[y0 + (xs & 1), xs] = 255
    e[3:h - 3, 2] = 255
    return e


def dot_lattice(h, w):
    """isolated pixels on a 2-px lattice: h*w/4 top-level contours"""
    e = np.zeros((h, w), np.uint8)
    e[1:h - 1:2, 1:w - 1:2] = 255
    return e

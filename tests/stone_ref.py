"""Plain references for the rank-3 finders that share no code with oracle/ or with the library: the grid-line search
(ck_find_intersections: k_gridlines.hip, update_grid of ck_stonegeom.cpp), the external-contour survey
(ck_contours_external: the dense labelling kernels and the two border followers of k_contours.hip) and the contour stones
finder (ck_contour_stones: k_stonefind.hip, ck_stonegeom.cpp).  Grey, Otsu, the medians and Canny come from
tests/filter_ref.py, the outer-border pixel sets from tests/board_ref.py; what is added here is written the slow, obvious
way.

* hough_lines_p: cv2.HoughLinesP(zone, 1, pi / 180, threshold, minLineLength, maxLineGap = 0) as OpenCV 3.1 runs it:
  the points in raster order; cv::RNG((uint64)-1) (multiply-with-carry, factor 4164903690) draws an index below the
  number left, the drawn point is overwritten by the last; a point that a found line has already taken is a dead draw;
  a live point votes in all 180 rows at cvRound(f32(j * cos) + f32(i * sin)) + (numrho - 1) / 2 with
  cos = (float)cos((double)n * (float)(pi / 180)); the first row that reaches the largest count wins if that count
  reaches the threshold; the walk from the point goes both ways in 16.16 fixed point (the long axis moves by one pixel,
  the other by cvRound(f32(f32(short * 65536) / |long|))) and ends at the zone border or at the first empty pixel; a
  line whose extent in x or in y reaches minLineLength is kept and the votes of its pixels are taken back -- whether or
  not they had voted --, a shorter one only loses its pixels.  It also returns the PATH RECORD the cases are chosen by.
* update_grid, find_intersections: stonesfinder.py:516-552, 888-947 in Python floats, over any (19, 19, 4) zone table.
* follow_contours: cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) by Suzuki's border follower, one contour per
  top-level component (board_ref.external_contours names them), started at the component's first pixel in raster order;
  a vertex is stored wherever the step direction differs from the one before.  Handed back last found first.
* find_stones: sf_contours.py:48-330 over any zone table.  open_rows: the opening the reference really asks for (a 4 x 1
  element anchored at its last row: minimum, then maximum, over rows y-3 .. y of the VIEW, rows outside it ignored) as two
  explicit loops.  hull: the strictly convex vertices.  min_rect: the smallest enclosing rectangle over the hull's edge
  directions in float64 -> (short side, long side, angle of the winning edge); only min, max and max(|cos|, |sin|) of it
  are used, which no angle convention changes.  fill_hull: cv2.drawContours(thickness=-1) of a convex polygon -- every
  side drawn by the 8-connected line iterator from its left end, then scanlines ymin .. ymax - 1 filled between the two
  active edges held in 16.16 fixed point (slope = (dx << 16) / dy by C division, span = ceil(left) .. floor(right)).
  chamfer: the 5 x 5 chamfer distance (65536, 91750, 143976) as a shortest-path search inside the box.  Every decision of
  the filters is reported with its margin (|value - threshold| / threshold), every zone with its sums, every find_color
  call with the branches it took.
"""
import heapq
import math
import sys

import numpy as np

from . import board_ref, filter_ref

GS = 19
NANG = 180
ZONE_LINES = 32                      # CK_ZONE_LINES


# ------------------------------------------------------------------------------------------------ HoughLinesP
class Rng:
    """cv::RNG: state = (uint32)state * 4164903690 + (state >> 32); uniform(0, n) = (uint32)state % n"""

    def __init__(self, state=(1 << 64) - 1):
        self.state = state

    def below(self, n):
        lo, hi = self.state & 0xFFFFFFFF, self.state >> 32
        self.state = (lo * 4164903690 + hi) & ((1 << 64) - 1)
        return (self.state & 0xFFFFFFFF) % n


def _trig():
    theta = float(np.float32(math.pi / 180))
    cos = np.array([np.float32(math.cos(n * theta)) for n in range(NANG)], np.float32)
    sin = np.array([np.float32(math.sin(n * theta)) for n in range(NANG)], np.float32)
    return cos, sin


COS, SIN = _trig()
_RHO = {}


def rho_table(height, width):
    """[n][i][j] -> accumulator column of pixel (row i, column j) in angle row n, float32 products and float32 sum"""
    key = (height, width)
    if key not in _RHO:
        j = np.arange(width, dtype=np.float32)[None, None, :]
        i = np.arange(height, dtype=np.float32)[None, :, None]
        a = (j * COS[:, None, None]).astype(np.float32)
        b = (i * SIN[:, None, None]).astype(np.float32)
        s = (a + b).astype(np.float32)
        _RHO[key] = np.rint(s).astype(np.int64) + (width + height)          # (numrho - 1) / 2 = width + height
    return _RHO[key]


def _round_f32(x):
    return int(np.rint(np.float32(x)))


def hough_lines_p(zone, threshold, min_len, xflag_on_equal=False):
    """-> (lines [(x0, y0, x1, y1)] in the order found, path record).  `xflag_on_equal` is a mutant of the walk's choice
    (x-major also where |a| = |b|, at 45 and 135 degrees) for tests/test_stone_ref_cpu.py."""
    zone = np.asarray(zone)
    height, width = zone.shape
    numrho = 2 * (width + height) + 1
    rho = rho_table(height, width)
    rows = np.arange(NANG)
    acc = np.zeros((NANG, numrho), np.int64)
    left = zone != 0                                    # the points no line has taken yet
    pts = [(int(j), int(i)) for i, j in zip(*np.nonzero(left))]
    rng = Rng()
    rec = dict(points=len(pts), drawn=0, dead=0, weak=0, kept=0, short=0, cmin=0, cmax=0, revote_negative=0,
               short_before_first_kept=0, lines=[], shorts=[], threshold=threshold, min_len=min_len)
    lines = []
    for count in range(len(pts), 0, -1):
        k = rng.below(count)
        j, i = pts[k]
        pts[k] = pts[count - 1]
        if not left[i, j]:
            rec["dead"] += 1
            continue
        rec["drawn"] += 1
        cols = rho[:, i, j]
        if (acc[rows, cols] < 0).any():
            rec["revote_negative"] += 1
        acc[rows, cols] += 1
        vals = acc[rows, cols]
        top = int(vals.max())
        rec["cmax"] = max(rec["cmax"], top)
        if top < threshold:
            rec["weak"] += 1
            continue
        winners = np.nonzero(vals == top)[0]
        n = int(winners[0])
        a, b = np.float32(-SIN[n]), np.float32(COS[n])
        xflag = bool(abs(a) >= abs(b)) if xflag_on_equal else bool(abs(a) > abs(b))
        one = np.float32(65536.0)
        if xflag:
            dx = 1 if a > 0 else -1
            dy = _round_f32(np.float32(b * one) / np.float32(abs(a)))
            x, y = j, (i << 16) + (1 << 15)
        else:
            dy = 1 if b > 0 else -1
            dx = _round_f32(np.float32(a * one) / np.float32(abs(b)))
            x, y = (j << 16) + (1 << 15), i
        walked, ends, why = [], [], []
        for sx, sy in ((dx, dy), (-dx, -dy)):
            px, py, path = x, y, []
            while True:
                jj, ii = (px, py >> 16) if xflag else (px >> 16, py)
                if jj < 0 or jj >= width or ii < 0 or ii >= height:
                    why.append("border")
                    break
                if not left[ii, jj]:
                    why.append("gap")
                    break
                path.append((jj, ii))
                px, py = px + sx, py + sy
            walked.append(path)
            ends.append(path[-1])
        (ax, ay), (bx, by) = ends
        extent = max(abs(bx - ax), abs(by - ay))
        good = abs(bx - ax) >= min_len or abs(by - ay) >= min_len
        info = dict(angle=n, tied=[int(v) for v in winners[1:]], xflag=xflag, unit=dx if xflag else dy,
                    frac=dy if xflag else dx, ends=tuple(why), extent=extent, steps=(len(walked[0]) - 1, len(walked[1]) - 1))
        for q in set(walked[0]) | set(walked[1]):
            left[q[1], q[0]] = False
            if good:
                acc[rows, rho[:, q[1], q[0]]] -= 1
        if good:
            rec["cmin"] = min(rec["cmin"], int(acc.min()))
            lines.append((ax, ay, bx, by))
            rec["kept"] += 1
            rec["lines"].append(info)
        else:
            rec["short"] += 1
            rec["shorts"].append(info)
            if not rec["kept"]:
                rec["short_before_first_kept"] += 1
    return lines, rec


# ------------------------------------------------------------------------------------------------ update_grid
def _inside(p, box, margin):
    return box[0] + margin < p[0] < box[2] - margin and box[1] + margin < p[1] < box[3] - margin


def _crossing(s, o):
    """where the lines through the two segments meet, truncated to integers; None for parallels"""
    d1x, d1y = s[2] - s[0], s[3] - s[1]
    d2x, d2y = o[2] - o[0], o[3] - o[1]
    det = float(d1x * d2y - d1y * d2x)
    if abs(det) < sys.float_info.epsilon:
        return None
    t = ((o[0] - s[0]) * d2y - (o[1] - s[1]) * d2x) / det
    return int(s[0] + t * d1x), int(s[1] + t * d1y)


def update_grid(lines, box, slot):
    """-> the new (x, y) of the intersection.  A line counts when it is level or upright (|cos| or |sin| of its angle over
    0.995) and its middle -- measured ACROSS the zone, with the reference's swapped axes -- lies inside the zone shrunk by
    a seventh of its smaller side.  One such line negates the position; two to four of them also move it to the mean of
    their pairwise crossings (every ordered pair) that lie inside the shrunk zone, truncated toward zero."""
    x0, y0, x1, y1 = (int(v) for v in box)
    margin = min(x1 - x0, y1 - y0) / 7
    good = []
    for ln in lines:
        ln = tuple(int(v) for v in ln)
        length = math.sqrt((ln[0] - ln[2]) ** 2 + (ln[1] - ln[3]) ** 2)
        theta = math.acos((ln[2] - ln[0]) / length)
        if abs(math.cos(theta)) > 0.995:
            mid = ((x0 + x1) / 2, (ln[0] + ln[2]) / 2 + y0)
        elif abs(math.sin(theta)) > 0.995:
            mid = ((ln[1] + ln[3]) / 2 + x0, (y1 + y0) / 2)
        else:
            continue
        if _inside(mid, (x0, y0, x1, y1), margin):
            good.append(ln)
    sx, sy = int(slot[0]), int(slot[1])
    if not good:
        return sx, sy
    sx, sy = -sx, -sy
    if 1 < len(good) < 5:
        tx = ty = n = 0
        for a in range(len(good)):
            for b in range(len(good)):
                if a == b:
                    continue
                c = _crossing(good[a], good[b])
                if c is None:
                    continue
                p = (c[1] + x0, c[0] + y0)
                if _inside(p, (x0, y0, x1, y1), margin):
                    tx, ty, n = tx + p[0], ty + p[1], n + 1
        if n:
            sx, sy = int(-tx / n), int(-ty / n)
    return sx, sy


def grid_edges(img):
    """the Canny map of find_intersections: grey, Otsu level, Canny(level / 2, level), thresholds floored"""
    gray = filter_ref.bgr2gray(img)
    level = filter_ref.otsu_level(gray)
    return filter_ref.canny(gray, int(math.floor(level / 2)), int(math.floor(level)))["edges"], level


def zone_params(x0, y0, x1, y1):
    side = min(x1 - x0, y1 - y0)
    return int(side * 3 / 4), int(side * 2 / 3)


def find_intersections(img, mtx, rects):
    """-> dict(grid int16 (19, 19, 2), found {(r, c): lines}, edges, level, records {(r, c): path record})"""
    edges, level = grid_edges(img)
    mtx = np.asarray(mtx, np.int16)
    grid = mtx.copy()
    found, records = {}, {}
    for r in range(GS):
        for c in range(GS):
            x0, y0, x1, y1 = (int(v) for v in rects[r][c])
            thr, min_len = zone_params(x0, y0, x1, y1)
            lines, rec = hough_lines_p(edges[x0:x1, y0:y1], thr, min_len)
            records[(r, c)] = rec
            if lines:
                found[(r, c)] = lines
                grid[r, c] = update_grid(lines, (x0, y0, x1, y1), mtx[r, c])
    return dict(grid=grid, found=found, edges=edges, level=level, records=records, mtx=mtx)


# ------------------------------------------------------------------------------------------------ contours
# direction d: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE as (dx, dy), y grows downwards
STEP = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))


def follow_border(e, x0, y0, resume=4):
    """the outer border that starts at (x0, y0), whose west neighbour is background: -> (nvert, set of (x, y) visited).
    `resume` = 5 is a mutant for tests/test_stone_ref_cpu.py: the search after a step starts one neighbour later."""
    d = 4
    first = None
    for _ in range(8):                                  # clockwise from west
        d = (d - 1) & 7
        if d == 4:
            break
        if e[y0 + STEP[d][1], x0 + STEP[d][0]]:
            first = (x0 + STEP[d][0], y0 + STEP[d][1])
            break
    if first is None:
        return 1, {(x0, y0)}
    x, y, prev = x0, y0, d ^ 4
    nvert, seen = 0, set()
    while True:
        seen.add((x, y))
        while True:                                     # counter-clockwise from the pixel we came from
            d = (d + 1) & 7
            nx, ny = x + STEP[d][0], y + STEP[d][1]
            if e[ny, nx]:
                break
        if d != prev:
            nvert += 1
            prev = d
        if (nx, ny) == (x0, y0) and (x, y) == first:
            return nvert, seen
        x, y = nx, ny
        d = (d + resume) & 7


def follow_contours(edges, resume=4):
    """-> [dict(start (x, y), nvert, pix: set of (x, y))] in cv2's order (last found first)"""
    e = np.asarray(edges) != 0
    e = e.copy()
    e[0, :] = e[-1, :] = e[:, 0] = e[:, -1] = False
    w = e.shape[1]
    out = []
    for c in board_ref.external_contours(edges):
        y0, x0 = divmod(int(c["key"]), w)
        nvert, pix = follow_border(e, x0, y0, resume)
        out.append(dict(start=(x0, y0), nvert=nvert, pix=pix, set_def=set(zip(c["xs"].tolist(), c["ys"].tolist()))))
    return out[::-1]


def follower_in_lds(h, w):
    """which follower k_contour_survey takes: the bit-packed map of one workgroup must fit 64 KB of LDS"""
    return h * ((w + 31) // 32) * 4 + 4 <= 64 * 1024


# ------------------------------------------------------------------------------------------------ which paths a case took
def grid_paths(out, rects):
    """the path records of one find_intersections run, folded into the set of path names tests/stone_cases.py asks for,
    plus the largest line count of a zone and the counter range -> (set, max_lines, cmin, cmax)"""
    took = set()
    max_lines = cmin = cmax = 0
    if out["level"] == 0 and not out["edges"].any():
        took.add("no_edges")
    for (r, c), rec in out["records"].items():
        x0, y0, x1, y1 = (int(v) for v in rects[r][c])
        max_lines, cmin, cmax = max(max_lines, rec["kept"]), min(cmin, rec["cmin"]), max(cmax, rec["cmax"])
        if rec["kept"]:
            took.add("kept_%dx%d" % (x1 - x0, y1 - y0))
        if rec["kept"] >= 2:
            took.add("two_lines")
        if rec["kept"] and rec["short_before_first_kept"] >= 3:
            took.add("shorts_before_kept")
        if rec["cmin"] < 0 and rec["revote_negative"]:
            took.add("negative_revoted")
        if rec["dead"]:
            took.add("dead_draw")
        if rec["weak"]:
            took.add("weak_vote")
        if rec["points"] > 64:
            took.add("points_over_64")
        for ln in rec["lines"]:
            n = ln["angle"]
            took.add("slot%d" % (n >> 6))
            if n in (0, 45, 90, 135):
                took.add("theta%d" % n)
            if n >= 176:
                took.add("angle_176_up")
            if any((t >> 6) != (n >> 6) for t in ln["tied"]):
                took.add("tie_across_slots")
            took.add("%s_unit%+d" % ("xflag" if ln["xflag"] else "yflag", ln["unit"]))
            if ln["frac"]:
                took.add("%s_frac%s" % ("xflag" if ln["xflag"] else "yflag", "+" if ln["frac"] > 0 else "-"))
            if min(ln["steps"]) > 0:
                took.add("%s_both_ways" % ("xflag" if ln["xflag"] else "yflag"))
            if ln["ends"] == ("border", "border") and ln["extent"] == 39 and max(ln["steps"]) >= 20:
                took.add("span39_border_to_border")
            if "gap" in ln["ends"]:
                took.add("end_at_gap")
            if ln["extent"] == rec["min_len"]:
                took.add("exactly_min_len")
        if any(ln["extent"] == rec["min_len"] - 1 for ln in rec["shorts"]):
            took.add("one_short_of_min_len")
    mtx, grid = out["mtx"], out["grid"]
    if ((grid == -mtx) & (mtx != 0)).all(-1).any():
        took.add("slot_negated")
    if (np.abs(grid) != np.abs(mtx)).any(-1).any():
        took.add("slot_moved")
    return took, max_lines, cmin, cmax


# ------------------------------------------------------------------------------------------------ contour stones
E, B, W = 0, 1, 2
OPEN_ROWS = 3                        # the opening looks at rows y - 3 .. y


def open_rows(fg, back=OPEN_ROWS):
    """`back` = 4 is a mutant for tests/test_stone_ref_cpu.py (a fifth row read)"""
    fg = np.asarray(fg, np.uint8)
    h = fg.shape[0]
    eroded = np.empty_like(fg)
    for y in range(h):
        eroded[y] = fg[max(0, y - back):y + 1].min(axis=0)
    out = np.empty_like(fg)
    for y in range(h):
        out[y] = eroded[max(0, y - back):y + 1].max(axis=0)
    return out


def hull(points):
    """strictly convex vertices of a set of integer (x, y), as a closed walk (monotone chain)"""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) < 3:
        return pts
    turn = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    halves = []
    for seq in (pts, pts[::-1]):
        chain = []
        for p in seq:
            while len(chain) >= 2 and turn(chain[-2], chain[-1], p) <= 0:
                chain.pop()
            chain.append(p)
        halves.append(chain[:-1])
    return halves[0] + halves[1]


def min_rect(hull_pts, want_rival=False):
    """-> (short side, long side, angle in degrees of the edge the rectangle lies along), float64; with want_rival also the
    list of (short, long, angle) of every rectangle whose area is within 1e-3 of the smallest, the smallest first: where
    there are several of different sides (a triangle: every side gives the same area), which one a float32 search hands
    back is a matter of rounding, so a decision must come out the same for all of them"""
    if len(hull_pts) < 3:
        (ax, ay), (bx, by) = hull_pts[0], hull_pts[-1]
        out = (0.0, math.hypot(bx - ax, by - ay), math.degrees(math.atan2(by - ay, bx - ax)) if len(hull_pts) == 2 else 0.0)
        return out + ([out],) if want_rival else out
    best = None
    every = []
    n = len(hull_pts)
    for k in range(n):
        (ax, ay), (bx, by) = hull_pts[k], hull_pts[(k + 1) % n]
        length = math.hypot(bx - ax, by - ay)
        ux, uy = (bx - ax) / length, (by - ay) / length
        along = [x * ux + y * uy for x, y in hull_pts]
        across = [-x * uy + y * ux for x, y in hull_pts]
        a, b = max(along) - min(along), max(across) - min(across)
        every.append((a * b, min(a, b), max(a, b), math.degrees(math.atan2(uy, ux))))
        if best is None or a * b < best[0]:
            best = (a * b, min(a, b), max(a, b), math.degrees(math.atan2(uy, ux)))
    if not want_rival:
        return best[1:]
    return best[1:] + ([best[1:]] + [e[1:] for e in every if e[0] <= best[0] * (1 + 1e-3)],)


def line_walk(p, q):
    """the pixels of the 8-connected line iterator between two points, walked from the left one"""
    if q[0] < p[0]:
        p, q = q, p
    (x, y), dx, dy = p, q[0] - p[0], abs(q[1] - p[1])
    sy = 1 if q[1] >= p[1] else -1
    out = []
    if dy > dx:                                          # one row per step; the column moves when the error says so
        err = dy - 2 * dx
        for _ in range(dy + 1):
            out.append((x, y))
            if err < 0:
                x, err = x + 1, err + 2 * dy
            err -= 2 * dx
            y += sy
    else:
        err = dx - 2 * dy
        for _ in range(dx + 1):
            out.append((x, y))
            if err < 0:
                y, err = y + sy, err + 2 * dx
            err -= 2 * dy
            x += 1
    return out


def fill_hull(img, poly, value=1):
    """paint the filled convex polygon `poly` (a closed walk of integer vertices inside the image) into img"""
    n = len(poly)
    edges = []
    for k in range(n):
        p, q = poly[k], poly[(k + 1) % n]
        for x, y in line_walk(p, q):
            img[y, x] = value
        if p[1] == q[1]:
            continue
        num, den = (q[0] - p[0]) << 16, q[1] - p[1]
        slope = abs(num) // abs(den)
        if (num < 0) != (den < 0):
            slope = -slope
        top, low = (p, q) if p[1] < q[1] else (q, p)
        edges.append((top[1], low[1], top[0] << 16, slope))
    if len(edges) < 2:
        return
    for y in range(min(e[0] for e in edges), max(e[1] for e in edges)):
        xs = sorted(x + (y - y0) * slope for y0, y1, x, slope in edges if y0 <= y < y1)
        for left, right in zip(xs[0::2], xs[1::2]):
            a, b = (left + 65535) >> 16, right >> 16
            if a <= b:
                img[y, max(a, 0):min(b, img.shape[1] - 1) + 1] = value


_CHAMFER = [(0, 1, 65536), (1, 0, 65536), (0, -1, 65536), (-1, 0, 65536), (1, 1, 91750), (1, -1, 91750), (-1, 1, 91750), (-1, -1, 91750)]
_CHAMFER += [(dy, dx, 143976) for dy in (-2, -1, 1, 2) for dx in (-2, -1, 1, 2) if abs(dy) != abs(dx)]


def chamfer(img):
    """16.16 distance of every pixel to the nearest zero pixel in steps (1, 1.4, 2.1969), paths kept inside the box"""
    img = np.asarray(img)
    h, w = img.shape
    dist = np.full((h, w), 1 << 40, np.int64)
    heap = [(0, int(y), int(x)) for y, x in np.argwhere(img == 0)]
    for _, y, x in heap:
        dist[y, x] = 0
    heapq.heapify(heap)
    while heap:
        d, y, x = heapq.heappop(heap)
        if d > dist[y, x]:
            continue
        for dy, dx, cost in _CHAMFER:
            yy, xx = y + dy, x + dx
            if 0 <= yy < h and 0 <= xx < w and d + cost < dist[yy, xx]:
                dist[yy, xx] = d + cost
                heapq.heappush(heap, (d + cost, yy, xx))
    return dist


def find_centers(dist, radius):
    """-> (centres [(x, y)], smallest margin of the centre test).  Raises ZeroDivisionError for a box no taller or no wider
    than a radius, as the reference does."""
    rows, cols = dist.shape
    nb_rows = int(round(rows / 2 / radius))
    row_width = int(rows / nb_rows)
    nb_cols = int(round(cols / 2 / radius))
    col_width = int(cols / nb_cols)
    reach = min(row_width, col_width) / 3
    out, margin = [], math.inf
    for row in range(nb_rows):
        for col in range(nb_cols):
            cell = dist[row * row_width:(row + 1) * row_width + 1, col * col_width:(col + 1) * col_width + 1]
            best, at = -1, None
            for y in range(cell.shape[0]):                   # the first maximum in raster order
                for x in range(cell.shape[1]):
                    if cell[y, x] > best:
                        best, at = cell[y, x], (x, y)
            off = math.sqrt((at[0] - col_width / 2) ** 2 + (at[1] - row_width / 2) ** 2)
            margin = min(margin, abs(off - reach) / reach)
            if reach < off:
                continue
            out.append((col * col_width + at[0], row * row_width + at[1]))
    return out, margin


def _decide(log, name, values, threshold, test, exact=True):
    """one entry per decision: (filter, side, margin, whether both sides of the comparison are exact in float32 too).
    `values`: the value decided on first, then its rivals (see min_rect); the margin is the smallest of them all, 0 where
    they do not agree"""
    values = values if isinstance(values, list) else [values]
    rejected = test(values[0])
    margin = 0.0 if any(test(v) != rejected for v in values) else min(abs(v - threshold) / threshold for v in values)
    log.append((name, "reject" if rejected else "pass", margin, exact))
    return rejected


def _trig(angle):
    a = math.radians(angle)
    return max(abs(math.cos(a)), abs(math.sin(a)))


def fg_contours(sub_fg, radius, log, back=OPEN_ROWS, min_vert=10):
    """analyse_fg + extract_contours_fg -> the contours kept (dicts of follow_contours); `log` takes one list of
    (filter, side, margin) per contour.  `back` and `min_vert` are mutants."""
    opened = open_rows(sub_fg, back)
    edges = filter_ref.canny(opened, 25, 75)["edges"]
    cands = []
    for c in follow_contours(edges):
        mine = []
        log.append(mine)
        if _decide(mine, "nvert", c["nvert"], 10, lambda v: v < min_vert):
            continue
        c["hull"] = hull(c["pix"])
        lo, hi, angle, rivals = min_rect(c["hull"], want_rival=True)
        upright = all(r[2] % 90 == 0 for r in rivals)        # an upright box of integers: its sides are exact in any float
        if _decide(mine, "short_side", [r[0] for r in rivals], 1.5 * radius, lambda v: v < 3 / 2 * radius, upright):
            continue
        if _decide(mine, "long_side", [r[1] for r in rivals], 5 * radius, lambda v: 5 * radius < v, upright):
            continue
        if _decide(mine, "big", [r[1] for r in rivals], 2.5 * radius, lambda v: 2.5 * radius < v, upright):
            if _decide(mine, "turned", [_trig(r[2]) for r in rivals], 0.97, lambda v: v < 0.97, False):
                continue
        xs, ys = [p[0] for p in c["hull"]], [p[1] for p in c["hull"]]
        x0, y0, bw, bh = min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1
        inside = np.zeros((bh, bw), np.uint8)
        fill_hull(inside, [(x - x0, y - y0) for x, y in c["hull"]])
        ratio = int(sub_fg[y0:y0 + bh, x0:x0 + bw].astype(np.int64)[inside == 1].sum()) / bh / bw / 255
        if _decide(mine, "fill", ratio, 0.3, lambda v: v < 0.3):
            continue
        cands.append((c, mine))
    kept = []
    ghost = np.zeros(sub_fg.shape, np.uint8)
    for c, mine in cands:
        xs, ys = [p[0] for p in c["pix"]], [p[1] for p in c["pix"]]
        ghost[ys, xs] = 255                                  # outlines stay from one candidate to the next
        box = ghost[min(ys):max(ys) + 1, min(xs):max(xs) + 1]
        centres, margin = find_centers(chamfer(255 - box), radius)
        mine.append(("centre", "pass" if centres else "reject", margin, True))
        if centres:
            kept.append(c)
    return kept


def find_color(r, c, zones, stones, took):
    """-> nothing; stones[r, c] is set where the neighbours agree.  `took` collects the branches"""
    colors, added = set(), 0
    me = [int(v) for v in zones[r, c, 1:4]]
    for i in (-1, 0, 1):
        if not 0 <= r + i < zones.shape[0]:
            continue
        for j in (-1, 0, 1):
            if (i == 0 and j == 0) or not 0 <= c + j < zones.shape[1]:
                continue
            other = [int(v) for v in zones[r + i, c + j, 1:4]]
            raw = [a - b for a, b in zip(me, other)]
            gap = sum(abs(v) for v in raw)
            if not zones[r + i, c + j, 0]:
                if 100 < gap:
                    colors.add(B if sum(raw) < 0 else W)
                    added += 1
                    took.add("bare_darker" if sum(raw) < 0 else "bare_brighter")
                elif gap < 70:
                    colors.add(E)
                    added = 3
                    took.add("bare_alike")
                else:
                    took.add("bare_between")
            else:
                if not (i < 1 and j < 1):
                    took.add("hull_later")
                else:
                    theirs = int(stones[r + i, c + j])
                    if theirs not in (B, W):
                        took.add("hull_undecided")
                        continue                             # skips the test of `added` below, as the reference
                    floor_ = min(sum(me), sum(other))
                    if gap < floor_ * 0.1:
                        colors.add(theirs)
                        added += 1
                        took.add("ally")
                    elif floor_ < gap:
                        colors.add(B if theirs == W else W)
                        added += 1
                        took.add("enemy")
                    else:
                        took.add("hull_between")
            if added == 3:
                break
        if added == 3:
            if len(colors) == 1:
                stones[r, c] = colors.pop()
                took.add("agreed")
            else:
                took.add("disagreed")
            return
    took.add("too_few_votes")


def find_stones(img, fg, rects, rs=0, re=GS, cs=0, ce=GS, back=OPEN_ROWS, min_vert=10, masked_on_equal=False, round_mean=False):
    """-> dict(stones (19, 19) uint8, zones int16 (re-rs, ce-cs, 4), mask uint8 (hs, ws), record).  The keyword switches
    after `ce` are mutants for tests/test_stone_ref_cpu.py."""
    side = img.shape[0]
    radius = side / GS / 2
    rects = np.asarray(rects).reshape(GS, GS, 4)
    x0, y0 = int(rects[rs, cs, 0]), int(rects[rs, cs, 1])
    x1, y1 = int(rects[re - 1, ce - 1, 2]), int(rects[re - 1, ce - 1, 3])
    sub_fg = np.ascontiguousarray(fg[x0:x1, y0:y1])
    sub = np.ascontiguousarray(img[x0:x1, y0:y1])
    rec = dict(fg=[], img=[], spans=set(), columns=set(), overlap=0, zones=[], colour=set(), view=(x1 - x0, y1 - y0))
    hulls = [c["hull"] for c in fg_contours(sub_fg, radius, rec["fg"], back, min_vert)]
    rec["fg_kept"] = len(hulls)
    for c in follow_contours(filter_ref.goban_canny(sub)["edges"]):
        mine = []
        rec["img"].append(mine)
        if _decide(mine, "nvert", c["nvert"], 10, lambda v: v < min_vert):
            continue
        hl = hull(c["pix"])
        rivals = min_rect(hl, want_rival=True)[3]
        if _decide(mine, "huge", [r[1] for r in rivals], 10 * radius, lambda v: 10 * radius < v, all(r[2] % 90 == 0 for r in rivals)):
            continue
        hulls.append(hl)
    mask = np.zeros(sub.shape[:2], np.uint8)
    for hl in hulls:
        one = np.zeros_like(mask)
        fill_hull(one, hl)
        rec["overlap"] += int((mask & one).sum())
        mask |= one
        for row in one:
            xs = np.nonzero(row)[0]
            if len(xs):
                rec["spans"].add(int(xs[-1] - xs[0] + 1))       # a convex shape: one run per row
                rec["columns"].update((int(xs[0]), int(xs[-1])))
    zones = np.zeros((re - rs, ce - cs, 4), np.int16)
    for r in range(re - rs):
        for c in range(ce - cs):
            a0, b0, a1, b1 = (int(v) for v in rects[r + rs, c + cs])
            a0, b0, a1, b1 = a0 - x0, b0 - y0, a1 - x0, b1 - y0
            area = (a1 - a0) * (b1 - b0)
            m = mask[a0:a1, b0:b1]
            px = sub[a0:a1, b0:b1].astype(np.int64)
            visible = int(m.sum())
            under = 0.4 * area <= visible if masked_on_equal else 0.4 * area < visible
            norm = visible if under else area - visible
            zones[r, c, 0] = 1 if under else 0
            means = []
            for k in range(3):
                total = int(px[:, :, k][m == (1 if under else 0)].sum())
                means.append(total / norm)
                zones[r, c, 1 + k] = int(round(total / norm)) if round_mean else int(total / norm)
            rec["zones"].append(dict(area=area, visible=visible, under=under, means=means))
    stones = np.zeros((GS, GS), np.uint8)
    view = stones[rs:re, cs:ce]
    for r in range(re - rs):
        for c in range(ce - cs):
            if zones[r, c, 0]:
                find_color(r, c, zones, view, rec["colour"])
    return dict(stones=stones, zones=zones, mask=mask, record=rec)


def stone_paths(out):
    """the record of one find_stones run folded into path names -> set"""
    rec = out["record"]
    took = set("colour_" + b for b in rec["colour"])
    for side_, logs in (("fg", rec["fg"]), ("img", rec["img"])):
        for log in logs:
            for name, what, _, _ in log:
                took.add("%s_%s_%s" % (side_, name, what))
            if log[0][2] == 0 and log[-1][:2] in (("centre", "pass"), ("huge", "pass")):
                took.add("%s_kept_with_10_vertices" % side_)
    for n in rec["spans"]:
        took.add("span_%d" % n if n in (1, 16, 17) else "span_over_32" if n > 32 else "span_other")
    if 1 in rec["columns"]:
        took.add("hull_at_column_1")
    if rec["view"][1] - 2 in rec["columns"]:
        took.add("hull_at_last_column")
    if rec["overlap"]:
        took.add("hulls_overlap")
    if not rec["spans"]:
        took.add("no_hull")
    for z in rec["zones"]:
        ratio = z["visible"] / (0.4 * z["area"])
        if 0.95 <= ratio <= 1.0:
            took.add("visible_just_under")
        if 1.0 < ratio <= 1.05:
            took.add("visible_just_over")
        if z["visible"] == 0.4 * z["area"]:
            took.add("visible_is_two_fifths")
        if z["area"] == 361:
            took.add("zone_361" + ("_under_hull" if z["under"] else "_bare"))
        if any(v - math.floor(v) >= 0.5 for v in z["means"]):
            took.add("truncation_is_not_rounding")
    return took


def stone_margins(out):
    """the smallest margin of a decision that float32 and float64 could take differently: those on the sides and the angle
    of a rectangle that is not upright (vertex counts, the fill sums and the chamfer distances are integers), taken over
    every rectangle that is the smallest to within 1e-3 of its area"""
    rec = out["record"]
    return min([m for logs in (rec["fg"], rec["img"]) for log in logs for _, _, m, exact in log if not exact], default=math.inf)

"""Inputs for tests/test_stone_ref_cpu.py and tests/test_gpu_stone_paths.py, built per path: every case is named after the
path of k_gridlines.hip, k_contours.hip or k_stonefind.hip it is for, and tests/test_stone_ref_cpu.py asserts from the path
record of tests/stone_ref.py (or from the shape) that the case takes it.  Builders only, deterministic; nothing here runs
the library.  One builder does run the reference: goban_learnt needs PosGrid.zones after one learn(), and what the grid
learns from is the answer of find_intersections on goban_default -- so that case's zone table depends on
stone_ref.find_intersections, the very function it is later compared with (a wrong reference would still give a valid,
merely different, displaced table).

Two things the contour-stones cases cannot be made to do, with the reason:
  * a foreground candidate thinner than one radius that reaches _find_centers (where the reference divides by zero, and the
    library answers CK_ERR_STATE).  _find_centers divides by round(rows / 2 / radius), which is 0 only for a box of at most
    `radius` rows, i.e. a contour that fits a strip r - 1 pixels wide; the axis-aligned rectangle around it is then an
    enclosing rectangle of area <= (r - 1) W, W its extent along the strip.  The smallest rectangle (lo <= hi) must also
    span W, so hi^2 + lo^2 >= W^2 >= (lo hi / (r - 1))^2, and with lo >= 1.5 r (the short-side filter, passed earlier)
    this gives hi^2 (2.25 r^2 / (r - 1)^2 - 1) <= 2.25 r^2, hi < 1.2 r < lo: no such contour at any image side.  The same
    holds for columns.  The branch is unreachable through ck_contour_stones; tests/test_stone_ref_cpu.py holds the
    reference's own ZeroDivisionError and this bound.
  * a hull that touches column 0 or column ws - 1 of the view: the contour survey clears the one-pixel frame of its map, as
    cv2.findContours does, so hulls reach column 1 and column ws - 2 at most.  The cases reach both.
"""
import math

import numpy as np

from . import stone_ref

GS = 19
SIDE = 380
GROUND = 90


# ------------------------------------------------------------------------------------------------ zone tables
def posgrid(size=SIDE):
    """PosGrid.mtx of the reference at its default: cell centres, truncated into int16"""
    start = size / GS / 2
    end = size - start
    mtx = np.zeros((GS, GS, 2), np.int16)
    for i in range(GS):
        for j in range(GS):
            mtx[i, j, 0] = (start * (GS - 1 - i) + end * i) / (GS - 1)
            mtx[i, j, 1] = (start * (GS - 1 - j) + end * j) / (GS - 1)
    return mtx


def zones_of(mtx, size=SIDE):
    """StonesFinder.getrect(r, c, cursor=1.0) for every intersection: halfway to the diagonal neighbours, mirrored at the
    first line, two pixels short of the mirror at the last, index -1 wrapping as in Python"""
    out = np.zeros((GS, GS, 4), np.int32)
    for r in range(GS):
        for c in range(GS):
            p = [int(v) for v in mtx[r, c]]
            before = [int(v) for v in mtx[r - 1, c - 1]]
            after = [int(v) for v in mtx[min(r + 1, GS - 1), min(c + 1, GS - 1)]]
            if r == 0:
                before[0] = -p[0]
            elif r == GS - 1:
                after[0] = 2 * size - p[0] - 2
            if c == 0:
                before[1] = -p[1]
            elif c == GS - 1:
                after[1] = 2 * size - p[1] - 2
            out[r, c] = (max(0, int(0.5 * before[0] + 0.5 * p[0])), max(0, int(0.5 * before[1] + 0.5 * p[1])),
                         min(size, int(0.5 * p[0] + 0.5 * after[0])), min(size, int(0.5 * p[1] + 0.5 * after[1])))
    return out


def learnt(mtx, grid, rate=0.2):
    """PosGrid.learn from a fresh grid: the mean move of the intersections that moved, scaled by `rate`, truncated, applied
    once more than 20 of them contributed -> the new mtx"""
    shift = np.abs(np.asarray(grid, np.int16)) - mtx
    movers = int(np.count_nonzero(np.abs(shift[:, :, 0]) + np.abs(shift[:, :, 1])))
    if movers <= 20:
        return mtx.copy()
    vect = shift.sum(axis=(0, 1), dtype=np.float32) / np.float32(movers)
    vect = (np.zeros(2, np.float32) * np.float32(1.0 - rate) + vect * np.float32(rate)).astype(np.float32)
    return (mtx + vect.astype(np.int16)).astype(np.int16)


SIZES = ((40, 40), (4, 40), (40, 4), (4, 4), (19, 20), (7, 33), (8, 8), (5, 13), (33, 7), (13, 5), (20, 19), (9, 7))
CELL = 40
NCELL = (SIDE // CELL) ** 2                                  # 81 cells of 40 x 40; the last 20 pixels stay ground


def cell_origin(k):
    return CELL * (k // 9), CELL * (k % 9)


def mixed_table(phase=0):
    """361 rectangles of the sizes in SIZES (rows x columns), each centred on one of the 81 cells (where the cell's own
    stroke passes), pushed back inside it: zones overlap and do not tile"""
    out = np.zeros((GS * GS, 4), np.int32)
    for z in range(GS * GS):
        hh, ww = SIZES[(z + phase) % len(SIZES)]
        cx, cy = cell_origin((z * 7 + phase) % NCELL)
        x0 = cx + min(max(0, 20 - hh // 2 + (z // 81) % 3 - 1), CELL - hh)
        y0 = cy + min(max(0, 20 - ww // 2 + (z // 27) % 3 - 1), CELL - ww)
        out[z] = (x0, y0, x0 + hh, y0 + ww)
    return out.reshape(GS, GS, 4)


def tiled_table(side, zone, stride):
    """19 x 19 rectangles of zone x zone pixels every `stride`, cut at the image"""
    out = np.zeros((GS, GS, 4), np.int32)
    for r in range(GS):
        for c in range(GS):
            out[r, c] = (r * stride, c * stride, min(side, r * stride + zone), min(side, c * stride + zone))
    return out


# ------------------------------------------------------------------------------------------------ goban images
def _flat(side=SIDE, level=GROUND):
    return np.full((side, side, 3), level, np.uint8)


def fan_image(seed, jitter):
    """one straight step edge per cell through (about) the cell's middle, the 81 cells sweeping the half turn; even cells
    are filled to their rim (the edge runs into the border of a zone), odd cells only inside a disc (it ends at a gap)"""
    rng = np.random.default_rng(seed)
    img = _flat()
    yy, xx = np.mgrid[0:CELL, 0:CELL]
    for k in range(NCELL):
        cx, cy = cell_origin(k)
        ang = math.radians((k * 180.0 / NCELL + jitter) % 180.0)
        off = rng.uniform(-1.5, 1.5)
        side_of = (xx - 19.5) * math.cos(ang) + (yy - 19.5) * math.sin(ang) > off
        if k % 2:
            side_of &= (xx - 19.5) ** 2 + (yy - 19.5) ** 2 < rng.uniform(8, 19) ** 2
        img[cx:cx + CELL, cy:cy + CELL][side_of] = int(rng.integers(170, 240))
    return img


def axes_image():
    """level and upright edges and both diagonals, exact: bars, and squares standing on a corner"""
    img = _flat()
    for k in range(NCELL):
        cx, cy = cell_origin(k)
        z = img[cx:cx + CELL, cy:cy + CELL]
        kind = k % 4
        if kind == 0:
            z[:, 18:] = 200                              # upright edge through the whole cell
        elif kind == 1:
            z[21:, :] = 30                               # level edge
        else:
            yy, xx = np.mgrid[0:CELL, 0:CELL]
            z[(xx + yy > 39) if kind == 2 else (xx - yy > 0)] = 220
    return img


def goban_image(dx=6, dy=-5):
    """dark lines on a bright board, displaced from the default intersections: crosses that move their intersection,
    far enough for PosGrid.learn to shift the whole grid"""
    img = _flat(level=170)
    for k in range(GS):
        img[10 + dx + 20 * k, :] = 40
        img[:, 10 + dy + 20 * k] = 40
    return img


def boxes_image(seed):
    """turned rectangles of many lengths: lines that end at gaps, some just under and some just over minLineLength"""
    rng = np.random.default_rng(seed)
    img = _flat()
    yy, xx = np.mgrid[0:CELL, 0:CELL]
    for k in range(NCELL):
        cx, cy = cell_origin(k)
        ang = rng.uniform(0, math.pi)
        half_l, half_w = rng.uniform(3, 19), rng.uniform(2, 9)
        u = (xx - 19.5) * math.cos(ang) + (yy - 19.5) * math.sin(ang)
        v = -(xx - 19.5) * math.sin(ang) + (yy - 19.5) * math.cos(ang)
        img[cx:cx + CELL, cy:cy + CELL][(np.abs(u) < half_l) & (np.abs(v) < half_w)] = int(rng.integers(150, 250))
    return img


def noise_image(seed, density):
    """salt on flat ground: dense, tangled edges -- many short lines, counters driven below zero and voted on again"""
    rng = np.random.default_rng(seed)
    img = _flat()
    img[rng.random((SIDE, SIDE)) < density] = 240
    return img


def hatch_image():
    """bars three pixels wide every six pixels, level in the even cells and upright in the odd ones: a zone full of
    parallel lines, each kept line taking votes back from the points of the others"""
    img = _flat()
    for k in range(NCELL):
        cx, cy = cell_origin(k)
        z = img[cx:cx + CELL, cy:cy + CELL]
        if k % 2:
            z[:, 1::6] = z[:, 2::6] = z[:, 3::6] = 230
        else:
            z[1::6, :] = z[2::6, :] = z[3::6, :] = 230
    return img


def two_level_image(side=SIDE):
    img = _flat(side, 50)
    img[:, side // 2:] = 200
    return img


def small_image(side, seed):
    rng = np.random.default_rng(seed)
    img = _flat(side)
    for _ in range(12):
        x, y = rng.integers(2, side - 12, 2)
        img[x:x + rng.integers(4, 12), y:y + rng.integers(4, 12)] = int(rng.integers(150, 250))
    return img


def grid_cases():
    """-> {name: dict(img, mtx, rects)}; goban_learnt is PosGrid.zones after one learn() from the reference's answer on
    goban_default"""
    mtx = posgrid()
    default = zones_of(mtx)
    shifted = (mtx + np.array([3, -2], np.int16)).astype(np.int16)
    cases = {
        "sizes_fan_a": dict(img=fan_image(1, 0.0), mtx=mtx, rects=mixed_table(0)),
        "sizes_fan_b": dict(img=fan_image(2, 1.1), mtx=mtx, rects=mixed_table(5)),
        "angles_axes": dict(img=axes_image(), mtx=mtx, rects=mixed_table(3)),
        "walks_boxes": dict(img=boxes_image(3), mtx=mtx, rects=mixed_table(1)),
        "short_lines_noise": dict(img=noise_image(4, 0.12), mtx=mtx, rects=mixed_table(2)),
        "negative_counters_hatch": dict(img=hatch_image(), mtx=mtx, rects=mixed_table(0)),
        "otsu_flat": dict(img=_flat(), mtx=mtx, rects=default),
        "otsu_two_level": dict(img=two_level_image(), mtx=mtx, rects=default),
        "side_76": dict(img=small_image(76, 5), mtx=posgrid(76), rects=tiled_table(76, 4, 4)),
        "side_127": dict(img=small_image(127, 6), mtx=posgrid(127), rects=tiled_table(127, 13, 6)),
        "goban_default": dict(img=goban_image(), mtx=mtx, rects=default),
        "goban_shifted": dict(img=goban_image(), mtx=shifted, rects=zones_of(shifted)),
    }
    first = stone_ref.find_intersections(cases["goban_default"]["img"], mtx, default)["grid"]
    moved = learnt(mtx, first)
    assert (moved != mtx).any()                              # the grid did learn
    cases["goban_learnt"] = dict(img=goban_image(), mtx=moved, rects=zones_of(moved))
    return cases


SIZE_PATHS = ("kept_4x4", "kept_4x40", "kept_40x4", "kept_40x40", "kept_19x20", "kept_7x33", "kept_8x8", "kept_5x13")
WALK_PATHS = ("xflag_unit-1", "xflag_frac+", "xflag_frac-", "yflag_unit+1", "yflag_unit-1", "yflag_frac-",
              "xflag_both_ways", "yflag_both_ways")
# the paths every case must take, as stone_ref.grid_paths names them.  (The long axis of an x-major walk always steps
# by -1 first: a = -sin is never positive on 0 .. 179 degrees; the short axis of a y-major walk never by a positive
# amount for the same reason.  The other sign of every step is taken by the second walk, from the same point the other
# way: xflag_both_ways / yflag_both_ways ask for a kept line of that branch whose two walks both moved.)
GRID_PATHS = {
    "sizes_fan_a": SIZE_PATHS + WALK_PATHS + ("slot0", "slot1", "slot2", "angle_176_up", "tie_across_slots", "end_at_gap",
                                              "span39_border_to_border", "exactly_min_len", "one_short_of_min_len",
                                              "points_over_64", "dead_draw", "weak_vote"),
    "sizes_fan_b": SIZE_PATHS + WALK_PATHS + ("slot0", "slot1", "slot2", "angle_176_up", "tie_across_slots"),
    "angles_axes": ("theta0", "theta45", "theta90", "theta135", "two_lines"),
    "walks_boxes": WALK_PATHS + ("end_at_gap", "exactly_min_len", "one_short_of_min_len", "shorts_before_kept"),
    "short_lines_noise": ("shorts_before_kept", "points_over_64", "dead_draw", "angle_176_up", "two_lines"),
    "negative_counters_hatch": ("negative_revoted", "two_lines", "span39_border_to_border", "kept_40x40", "kept_4x40"),
    "otsu_flat": ("no_edges",),
    "otsu_two_level": ("theta0", "slot_negated"),
    "side_76": ("kept_4x4", "two_lines"),
    "side_127": ("kept_13x13", "two_lines"),
    "goban_default": ("slot_negated", "slot_moved", "two_lines"),
    "goban_shifted": ("slot_negated", "slot_moved", "two_lines"),
    "goban_learnt": ("slot_negated", "slot_moved", "two_lines"),
}


def refused_table():
    """a 41 x 20 zone: one more than the LDS layout of hough_zones_kernel is sized for"""
    t = zones_of(posgrid()).copy()
    t[9, 9] = (100, 100, 141, 120)
    return t


# ------------------------------------------------------------------------------------------------ edge maps
def ring(e, y0, x0, y1, x1):
    e[y0, x0:x1 + 1] = e[y1, x0:x1 + 1] = 255
    e[y0:y1 + 1, x0] = e[y0:y1 + 1, x1] = 255


def spiral(h, w, pitch=4):
    """one 1-px stroke winding inwards from the rim"""
    e = np.zeros((h, w), np.uint8)
    y0, x0, y1, x1 = 1, 1, h - 2, w - 2
    start = x0                                           # the top stroke of a turn starts where the last turn came up
    while y1 - y0 > pitch and x1 - x0 > pitch:
        e[y0, start:x1 + 1] = 255
        e[y0:y1 + 1, x1] = 255
        e[y1, x0:x1 + 1] = 255
        e[y0 + pitch:y1 + 1, x0] = 255
        start = x0
        y0, x0, y1, x1 = y0 + pitch, x0 + pitch, y1 - pitch, x1 - pitch
    return e


def shapes_map(h=24, w=40):
    """an isolated pixel, a 2-pixel contour, a figure eight (two rings sharing a corner pixel), two blobs joined by a
    one-pixel bridge (the follower passes the bridge twice), a stroke, a caret whose tip is the start pixel (the
    follower passes its start between the two arms)"""
    e = np.zeros((h, w), np.uint8)
    e[3, 3] = 255
    e[3, 7] = e[4, 8] = 255
    ring(e, 8, 3, 12, 7)
    ring(e, 12, 7, 16, 11)
    e[3:7, 14:18] = 255
    e[5, 18:22] = 255
    e[3:7, 22:26] = 255
    e[10:20, 30] = 255                                   # a stroke: every pixel but the ends is passed twice
    e[3, 35] = e[4, 34] = e[5, 33] = e[4, 36] = e[5, 37] = 255
    return e


def seam_map(w, h=12):
    """a ring hugging rows 1 and h - 2 and columns 1 and w - 2, and inside it, blobs and strokes on the bit-word seams:
    pixels at x with (x - 1) & 31 in {29, 30, 31} and on both sides of x = 32 k"""
    e = np.zeros((h, w), np.uint8)
    ring(e, 1, 1, h - 2, w - 2)
    for k in range(1, (w - 4) // 32 + 1):
        x = 32 * k
        if x + 3 < w - 3:
            e[3, x - 2:x + 3] = 255                      # level stroke over the seam
            e[5:8, x - 2] = 255                          # (x - 1) & 31 = 29
            e[5:8, x] = 255                              # 31
            e[9, x - 1] = 255                            # 30, an isolated pixel
    if w - 4 > 3:
        e[5:8, w - 4] = 255                              # one background column from the ring
    return e


def switch_map(h, w=1024):
    """a map on one side of the LDS / global follower switch: a spiral that dominates it, and small shapes"""
    e = spiral(h, w, pitch=32)
    s = shapes_map()
    e[40:40 + s.shape[0], 40:40 + s.shape[1]] = s
    e[h - 40:h - 36, w - 60:w - 40] = 255
    return e


def contour_cases():
    """-> {name: (n, h, w) uint8 batch}"""
    rng = np.random.default_rng(11)
    noise = lambda h, w, d: ((rng.random((h, w)) < d) * 255).astype(np.uint8)
    cases = {
        "follower_lds_511x1024": switch_map(511)[None],
        "follower_global_512x1024": switch_map(512)[None],
        "shapes": np.stack([shapes_map(), shapes_map()[::-1].copy(), shapes_map()[:, ::-1].copy()]),
        "spiral_dominates": spiral(61, 83)[None],
        "one_map_empty": np.stack([shapes_map(), np.zeros((24, 40), np.uint8), noise(24, 40, 0.3)]),
        "all_maps_empty": np.zeros((2, 24, 40), np.uint8),
        "noise_odd_width": np.stack([noise(37, 53, 0.2), noise(37, 53, 0.5)]),
        "full_frame": np.full((2, 9, 11), 255, np.uint8),
    }
    for w in (64, 65, 66, 63, 96, 100):                      # 0, 1, 2, 31 (mod 32); multiples of 4 and not
        cases["seams_w%d" % w] = np.stack([seam_map(w), noise(12, w, 0.35)])
    return cases


# ------------------------------------------------------------------------------------------------ contour stones
REGIONS = tuple((rs, rs + 7, cs, cs + 7) for rs in (0, 6, 12) for cs in (0, 6, 12)) + ((0, GS, 0, GS),)


def stone_board(seed, levels=(20, 240, 75, 120, 185)):
    """a goban image: textured ground of about 150 (so zone means have fractions), discs of radius 8 on random
    intersections in runs along rows and columns -- black, white, and three greys whose distance to the ground falls on
    each side of find_color's 70 and 100"""
    rng = np.random.default_rng(seed)
    img = (150 + rng.integers(-4, 5, (SIDE, SIDE, 1)) + rng.integers(-1, 2, (SIDE, SIDE, 3))).astype(np.uint8)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    for _ in range(46):
        r, c = rng.integers(0, GS, 2)
        dr, dc = ((0, 1), (1, 0), (1, 1))[int(rng.integers(0, 3))]
        for k in range(int(rng.integers(1, 4))):
            rr, cc = r + k * dr, c + k * dc
            if rr < GS and cc < GS:
                level = levels[int(rng.integers(0, len(levels)))] if rng.random() < 0.5 else levels[int(rng.integers(0, 2))]
                img[(yy - (10 + 20 * rr)) ** 2 + (xx - (10 + 20 * cc)) ** 2 <= 64] = level
    return img


def box_blob(fg, y, x, h, w):
    """an upright box whose rim carries two-pixel teeth: its outline has far more than ten vertices, its hull is the box"""
    fg[y:y + h, x:x + w] = 255
    fg[y + 4:y + h - 4:4, x:x + 2] = 0
    fg[y + 4:y + h - 4:4, x + w - 2:x + w] = 0
    fg[y + h - 2:y + h, x + 4:x + w - 4:4] = 0


def turned_blob(fg, cy, cx, half_l, half_w, deg, hollow=0.0):
    yy, xx = np.mgrid[0:fg.shape[0], 0:fg.shape[1]]
    a = math.radians(deg)
    u = (xx - cx) * math.cos(a) + (yy - cy) * math.sin(a)
    v = -(xx - cx) * math.sin(a) + (yy - cy) * math.cos(a)
    inside = (np.abs(u) <= half_l) & (np.abs(v) <= half_w)
    if hollow:
        inside &= ~((np.abs(u) <= half_l * hollow) & (np.abs(v) <= half_w * hollow))
    fg[inside] = 255


def frame_blob(fg, y, x, side, post):
    """a hollow square: lintels four rows high (what the opening lets through), posts `post` pixels wide"""
    fg[y:y + 4, x:x + side] = fg[y + side - 4:y + side, x:x + side] = 255
    fg[y:y + side, x:x + post] = fg[y:y + side, x + side - post:x + side] = 255


def disc_blob(fg, cy, cx, r):
    yy, xx = np.mgrid[0:fg.shape[0], 0:fg.shape[1]]
    fg[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255


def filter_mask():
    """foreground blobs, one per 60-pixel cell and more, that put every filter of extract_contours_fg / analyse_fg on both
    sides of its threshold"""
    fg = np.zeros((SIDE, SIDE), np.uint8)
    disc_blob(fg, 30, 30, 9)                             # a stone: kept
    disc_blob(fg, 30, 90, 6.6)                           # short side just under 15
    disc_blob(fg, 30, 150, 8.2)                          # and just over
    fg[27:33, 205:215] = 255                             # a bar of 6 x 10: fewer than ten vertices
    box_blob(fg, 20, 260, 20, 47)                        # long side under 50, upright: kept
    box_blob(fg, 20, 320, 20, 54)                        # long side over 50
    turned_blob(fg, 95, 40, 17, 9, 30)                   # long side over 25 and turned: rejected
    turned_blob(fg, 95, 110, 11, 9, 30)                  # turned but small: kept
    turned_blob(fg, 95, 170, 17, 9, 12)                  # big, turned a little: |cos| = 0.978, kept
    turned_blob(fg, 95, 240, 17, 9, 16)                  # |cos| = 0.961, rejected
    frame_blob(fg, 80, 300, 40, 2)                       # a frame: fill ratio 0.28
    frame_blob(fg, 140, 20, 40, 3)                       # thicker posts: 0.32
    box_blob(fg, 140, 90, 22, 22)
    fg[150:153, 90:112] = 0                              # a box cut in two lying halves, ten rows each: no cell centre
    fg[142:160, 140:143] = 255                           # an L: the farthest point of its box hugs a wall
    fg[157:160, 140:162] = 255
    for k in range(6):                                   # a comb: many vertices, open to one side
        fg[200:222, 30 + 4 * k:32 + 4 * k] = 255
    fg[220:223, 30:54] = 255
    disc_blob(fg, 215, 100, 9)
    disc_blob(fg, 215, 118, 9)                           # two stones touching: one contour, two cells
    fg[260:280, 20:40] = 255                             # a plain box: its outline has fewer than ten vertices;
    fg[260:280, 60:80] = 255
    fg[260, 60] = 0                                      # with one corner pixel gone: exactly ten, and kept
    return fg


def span_mask():
    """hulls with row spans of 1 (a diamond's tip), 16, 17 and more than 32 pixels, hulls that overlap, and hulls that reach
    column 1 and column ws - 2 (the outermost a contour can: the survey clears the frame of its map, as findContours does)"""
    fg = np.zeros((SIDE, SIDE), np.uint8)
    turned_blob(fg, 40, 40.5, 8, 8, 55)                  # turned squares whose hull ends in a single pixel
    turned_blob(fg, 40, 90, 10, 10, 50)
    box_blob(fg, 30, 130, 18, 16)
    box_blob(fg, 30, 170, 18, 17)
    box_blob(fg, 30, 210, 18, 15)
    box_blob(fg, 30, 250, 20, 40)
    box_blob(fg, 30, 310, 20, 36)
    disc_blob(fg, 100, 40, 10)                           # two discs whose hulls overlap although the blobs do not touch
    turned_blob(fg, 104, 62, 10, 10, 45)
    box_blob(fg, 90, 0, 20, 20)                          # into the left frame
    box_blob(fg, 90, SIDE - 21, 20, 21)                  # into the right one
    box_blob(fg, 140, 0, 22, 18)
    box_blob(fg, 140, SIDE - 19, 22, 19)
    return fg


def sweep_mask(step=1):
    """boxes of 22 x 22 sliding across the zones a pixel further in each cell: the hull covers a zone by every amount around
    two fifths, the corner zones of 19 x 19 and the rim zones of 19 x 20 included"""
    fg = np.zeros((SIDE, SIDE), np.uint8)
    k = 0
    for r in range(0, GS - 1, 2):
        for c in range(0, GS - 1, 2):
            y, x = 20 * r + 2 + (k * step) % 17, 20 * c + 2 + (k * step * 5) % 17
            box_blob(fg, y, x, 22, 22)
            k += 1
    box_blob(fg, SIDE - 22, SIDE - 22, 20, 20)           # over the last corner zone
    box_blob(fg, SIDE - 30, 2, 22, 22)
    return fg


def stone_cases():
    """-> {name: dict(img, fg, region)}: single images; stone_batches() groups them"""
    board = stone_board(7)
    empty = np.zeros((SIDE, SIDE), np.uint8)
    rng = np.random.default_rng(8)
    moves = empty.copy()                                  # fresh stones and a hand over the board of every region
    for r, c in rng.integers(0, GS, (40, 2)):
        disc_blob(moves, 10 + 20 * r + int(rng.integers(-2, 3)), 10 + 20 * c + int(rng.integers(-2, 3)), 9)
    turned_blob(moves, 190, 300, 60, 12, 20)
    cases = {}
    for region in REGIONS:
        name = "whole_board" if region == (0, GS, 0, GS) else "region_r%d_c%d" % (region[0], region[2])
        cases[name] = dict(img=board, fg=moves, region=region)
    rects = zones_of(posgrid())
    for name, above in (("above_view_0", 0), ("above_view_255", 255)):
        fg = empty.copy()
        x0, y0 = int(rects[6, 6, 0]), int(rects[6, 6, 1])
        for k in range(6):                               # blobs that start in rows 0 .. 5 of the view
            disc_blob(fg, x0 + k + 9, y0 + 12 + 22 * k, 9)
        fg[:x0] = 0
        fg[x0 - 4:x0] = above
        cases[name] = dict(img=board, fg=fg, region=(6, 13, 6, 13))
    cases["filters"] = dict(img=stone_board(9), fg=filter_mask(), region=(0, GS, 0, GS))
    cases["hull_spans"] = dict(img=stone_board(10), fg=span_mask(), region=(0, GS, 0, GS))
    cases["two_fifths"] = dict(img=stone_board(11), fg=sweep_mask(), region=(0, GS, 0, GS))
    huge = _flat(level=150)
    disc_blob(huge[:, :, 0], 80, 80, 52)                 # image contours of more than and of just under 100 pixels
    huge[:, :, 1:][huge[:, :, 0] == 255] = 255
    for ch in range(3):
        turned_blob(huge[:, :, ch], 250, 250, 47, 47, 0)
        huge[:, :, ch][huge[:, :, ch] == 255] = 30 if ch else 30
    cases["image_contours"] = dict(img=huge, fg=empty, region=(0, GS, 0, GS))
    cases["flat"] = dict(img=_flat(level=150), fg=empty, region=(0, GS, 0, GS))
    return cases


STONE_BATCHES = {
    "batch_1_and_3_without_hull": ("filters", "flat", "hull_spans", "flat"),
    "batch_without_any_span": ("flat", "flat"),
    "batch_of_boards": ("whole_board", "two_fifths", "image_contours"),
}


ALL_COLOURS = tuple("colour_" + b for b in ("agreed", "disagreed", "too_few_votes", "bare_darker", "bare_brighter", "bare_alike",
                                            "bare_between", "ally", "enemy", "hull_between", "hull_later", "hull_undecided"))
FG_FILTERS = tuple("fg_%s_%s" % (f, side) for f in ("nvert", "short_side", "long_side", "big", "turned", "fill") for side in ("pass", "reject"))
# the paths every case must take, as stone_ref.stone_paths names them
STONE_PATHS = {
    "whole_board": ALL_COLOURS + ("span_1", "span_16", "span_17", "span_over_32", "hulls_overlap", "hull_at_column_1",
                                  "hull_at_last_column", "visible_just_under", "visible_just_over", "zone_361_under_hull",
                                  "truncation_is_not_rounding", "img_nvert_reject", "img_huge_pass", "visible_is_two_fifths"),
    "above_view_0": ("fg_centre_pass", "colour_agreed"),
    "above_view_255": ("fg_centre_pass", "colour_agreed"),
    "filters": FG_FILTERS + ("fg_centre_pass", "fg_kept_with_10_vertices", "visible_is_two_fifths") + ALL_COLOURS,
    "hull_spans": ("span_1", "span_16", "span_17", "span_over_32", "hulls_overlap", "hull_at_last_column", "fg_centre_reject",
                   "fg_centre_pass"),
    "two_fifths": ("visible_just_under", "visible_just_over", "zone_361_bare", "truncation_is_not_rounding", "hull_at_column_1",
                   "hull_at_last_column", "fg_centre_reject"),
    "image_contours": ("img_huge_pass", "img_huge_reject", "span_over_32"),
    "flat": ("no_hull",),
}
STONE_PATHS.update({"region_r%d_c%d" % (rs, cs): ("fg_centre_pass", "img_nvert_pass", "colour_agreed") for rs in (0, 6, 12) for cs in (0, 6, 12)})

"""What the finders concluded, as display lists for the frames of a film (tools/transcode.py --annotate): the grid, the
stones of the game position after each frame, the agitated zones, the corners and hull of the board, and two lines of
text.  Everything here builds lists (core/overlay.py); the caller draws a whole batch with one Context.overlay_draw."""
import numpy as np

from ..golib_shim import B, E, Move, NP_TYPE, W, gsize
from . import overlay

AGITATION_RATIO = 0.7            # SfNeural.is_agitated's default (reference stone/sf_neural.py:178-180)
BLACK, WHITE, RED, GRID = (0, 0, 0), (255, 255, 255), (0, 0, 255), (255, 255, 0)


def moves_text(requests):
    """the requests one frame emitted, [(kind, [(colour, r, c), ..]), ..] -> 'B[D4] W[Q16]', removals as 'E[..]'"""
    return " ".join(repr(Move(NP_TYPE, (color if color in (B, W) else "E", r, c))) for _kind, moves in requests for color, r, c in moves)


def _stones(dl, codes, points, radius):
    """a disc per stone with a ring in the opposite colour; points[r, c] = (x, y)"""
    black, white = overlay.colour_code(BLACK), overlay.colour_code(WHITE)
    codes = np.asarray(codes)
    rows, cols = np.nonzero(codes > 0)
    for (x, y), code in zip(np.asarray(points)[rows, cols].tolist(), codes[rows, cols].tolist()):
        mine, other = (black, white) if code == 1 else (white, black)
        dl.prims.append((overlay.DISC, x, y, 0, 0, radius, mine, 0))
        dl.prims.append((overlay.CIRCLE, x, y, 1, 0, radius, other, 0))
    return dl


_grid_rows = {}


def _grid(dl, points, radius):
    """a circle per intersection; the rows are built once per set of points (the same 361 on every frame of a film)"""
    key = (points.tobytes(), radius)
    rows = _grid_rows.get(key)
    if rows is None:
        one = overlay.DisplayList()
        for x, y in points.reshape(-1, 2):
            one.circle(int(x), int(y), radius, GRID)
        _grid_rows.clear()
        rows = _grid_rows[key] = one.prims
    dl.prims.extend(rows)
    return dl


def goban_list(codes, fgcount, posgrid, frame_no, total, moves="", into=None):
    """the annotation of one 380 x 380 goban image: the grid's circles (as StonesFinder._drawgrid), the stones of the
    position `codes` (19, 19; 0 E / 1 B / 2 W) as discs of radius 6 ringed in the opposite colour, the zones whose
    foreground count `fgcount` (19, 19, or None) exceeds AGITATION_RATIO of their area as filled red rectangles at alpha
    96, 'Frame i/N' at the top and the frame's moves at the bottom"""
    dl = into if into is not None else overlay.DisplayList()
    mtx = posgrid.mtx
    _grid(dl, np.ascontiguousarray(mtx[..., ::-1]), 5)
    _stones(dl, codes, mtx[..., ::-1], 6)
    if fgcount is not None:
        zones = posgrid.zones()
        area = (zones[..., 2] - zones[..., 0]) * (zones[..., 3] - zones[..., 1])
        for r, c in np.argwhere(area * AGITATION_RATIO < np.asarray(fgcount).reshape(gsize, gsize)):
            x0, y0, x1, y1 = (int(v) for v in zones[r, c])                 # rows x0 .. x1 - 1, columns y0 .. y1 - 1
            dl.rect(y0, x0, y1 - 1, x1 - 1, RED, thickness=0, alpha=96)
    return _captions(dl, posgrid.size, frame_no, total, moves, 1)


def _captions(dl, height, frame_no, total, moves, scale):
    top, left = 4 * scale, 4 * scale
    for x, y, s in ((left, top, "Frame %d/%d" % (frame_no, total)), (left, height - top - overlay.CELL_H * scale, moves)):
        if s:
            dl.text(x + scale, y + scale, s, BLACK, scale=scale).text(x, y, s, WHITE, scale=scale)
    return dl


def project(mtx_inv, points):
    """goban-image points (.., 2) as (x, y) through the inverse board transform -> frame pixels (.., 2), rounded"""
    p = np.asarray(points, np.float64)
    q = np.concatenate([p, np.ones(p.shape[:-1] + (1,))], -1) @ np.asarray(mtx_inv, np.float64).T
    return np.rint(q[..., :2] / q[..., 2:]).astype(np.int64)


def frame_list(shape, corners, mtx, codes, posgrid, frame_no, total, moves="", into=None):
    """the annotation of one full-size frame of `shape` (h, w): the corners and hull as GobanCorners.paint paints them,
    the 361 intersections projected through the inverse of the board transform `mtx` as radius-3 circles, the stones on
    top as discs at the projected positions, and the two text lines at scale 2.  Before the first detection (mtx None)
    only the text."""
    dl = into if into is not None else overlay.DisplayList()
    if mtx is not None:
        if hasattr(corners, "display_list"):                    # (the host application's GobanCorners only paints with cv2)
            corners.display_list(dl)
        points = project(np.linalg.inv(np.asarray(mtx, np.float64)), posgrid.mtx[..., ::-1])
        # a degenerate transform can throw points anywhere: the rasteriser takes |coordinate| <= 32767
        points = np.clip(points, -32767, 32767)
        _grid(dl, np.ascontiguousarray(points), 3)
        cell = np.abs(points[9, 10] - points[9, 9]).max()
        _stones(dl, codes, points, int(min(4095, max(2, cell * 2 // 5))))
    return _captions(dl, shape[0], frame_no, total, moves, 2)

"""A plain painter for display lists: the reference the overlay kernel is compared with, byte for byte.  It shares no code
with the library: it paints primitive after primitive (the library tests pixel after pixel), steps a segment by
Bresenham's error recurrence (the library uses the closed form), loops discs, rings and rectangles over their boxes,
and renders text from glyph rows handed in as data.

    paint(images, prims, frame_start, text, glyphs) -> a painted copy, and the mask of the pixels any primitive covered
    pixels_of(prim, h, w, text, glyphs)             -> the set of (x, y) one primitive covers inside an h x w image

prims (P, 8) = kind, x0, y0, x1, y1, size, colour, aux as include/camkifu_amd.h has them; glyphs: (95, 7) row bytes
of bytes 32 .. 126, bit 4 = the leftmost column."""
import numpy as np

SEGMENT, CIRCLE, DISC, RECT, TEXT = 1, 2, 3, 4, 5


def bresenham(x0, y0, x1, y1):
    """the path of a thin segment as a list of (x, y), from the lexicographically smaller endpoint: err = D - 2d, a minor
    step whenever err < 0 (then err += 2D - 2d), else err -= 2d -- OpenCV's LineIterator"""
    if (x1, y1) < (x0, y0):
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, y1 - y0
    sx, sy = 1, (1 if dy >= 0 else -1)
    dx, dy = abs(dx), abs(dy)
    steep = dy > dx
    big, small = (dy, dx) if steep else (dx, dy)
    err = big - 2 * small
    x, y, out = x0, y0, []
    for _ in range(big + 1):
        out.append((x, y))
        minor = err < 0
        err += (2 * big - 2 * small) if minor else (-2 * small)
        if steep:
            y += sy
            x += sx if minor else 0
        else:
            x += sx
            y += sy if minor else 0
    return out


def _clip_path_range(x0, y0, x1, y1, h, w, margin):
    """True when the box of the segment, grown by margin, misses the image (nothing to paint: skip the long walk)"""
    return max(x0, x1) + margin < 0 or min(x0, x1) - margin >= w or max(y0, y1) + margin < 0 or min(y0, y1) - margin >= h


def _in_disc(dx, dy, r):
    return r >= 0 and dx * dx + dy * dy <= r * r + r


def pixels_of(prim, h, w, text=b"", glyphs=None):
    kind, x0, y0, x1, y1, size, _colour, aux = (int(v) for v in prim)
    out = set()
    if kind == SEGMENT:
        half = (size - 1) // 2
        if _clip_path_range(x0, y0, x1, y1, h, w, half):
            return out
        for px, py in bresenham(x0, y0, x1, y1):
            if px + half < 0 or px - half >= w or py + half < 0 or py - half >= h:
                continue
            for yy in range(max(0, py - half), min(h, py + half + 1)):
                for xx in range(max(0, px - half), min(w, px + half + 1)):
                    out.add((xx, yy))
    elif kind in (DISC, CIRCLE):
        outer = size if kind == DISC else size + (x1 - 1) // 2
        inner = -1 if kind == DISC else size - (x1 + 1) // 2
        for yy in range(max(0, y0 - outer), min(h, y0 + outer + 1)):
            for xx in range(max(0, x0 - outer), min(w, x0 + outer + 1)):
                if _in_disc(xx - x0, yy - y0, outer) and not _in_disc(xx - x0, yy - y0, inner):
                    out.add((xx, yy))
    elif kind == RECT:
        xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        for yy in range(max(0, ya), min(h, yb + 1)):
            for xx in range(max(0, xa), min(w, xb + 1)):
                if size == 0 or min(xx - xa, xb - xx, yy - ya, yb - yy) < size:
                    out.add((xx, yy))
    elif kind == TEXT:
        for k, byte in enumerate(text[aux:aux + x1]):
            rows = glyphs[(byte if 32 <= byte <= 126 else ord("?")) - 32]
            cx = x0 + k * 6 * size
            if cx >= w or cx + 5 * size <= 0:
                continue
            for gy in range(7):
                for gx in range(5):
                    if not (int(rows[gy]) >> (4 - gx)) & 1:
                        continue
                    for yy in range(max(0, y0 + gy * size), min(h, y0 + (gy + 1) * size)):
                        for xx in range(max(0, cx + gx * size), min(w, cx + (gx + 1) * size)):
                            out.add((xx, yy))
    else:
        raise ValueError("unknown kind %d" % kind)
    return out


def blend(colour, pixel, alpha):
    """one channel: alpha 255 replaces, else (c alpha + p (255 - alpha) + 127) // 255"""
    return colour if alpha == 255 else (colour * alpha + pixel * (255 - alpha) + 127) // 255


def paint(images, prims, frame_start, text=b"", glyphs=None):
    """images (n, h, w, c) or (n, h, w) uint8 -> (painted copy, covered (n, h, w) bool)"""
    out = np.array(images, np.uint8, copy=True)
    view = out.reshape(out.shape[:3] + (-1,))
    n, h, w, c = view.shape
    covered = np.zeros((n, h, w), bool)
    prims = np.asarray(prims).reshape(-1, 8)
    for f in range(n):
        for prim in prims[frame_start[f]:frame_start[f + 1]]:
            colour = int(prim[6]) & 0xffffffff
            alpha = colour >> 24
            for x, y in pixels_of(prim, h, w, text, glyphs):
                covered[f, y, x] = True
                for ch in range(c):
                    view[f, y, x, ch] = blend(colour >> (8 * ch) & 255, int(view[f, y, x, ch]), alpha)
    return out, covered

"""The overlay reference (tests/overlay_ref.py) against answers written by hand: what every other overlay test trusts."""
import numpy as np

from . import overlay_ref as ref


def _covered(prim, h=16, w=16):
    return sorted(ref.pixels_of(prim, h, w))


def test_segments_by_hand():
    assert ref.bresenham(0, 0, 4, 2) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)]        # the half-way tie: the smaller offset
    assert ref.bresenham(0, 0, 2, 1) == [(0, 0), (1, 0), (2, 1)]
    assert ref.bresenham(4, 2, 0, 0) == ref.bresenham(0, 0, 4, 2)                        # from the smaller endpoint, always
    assert ref.bresenham(0, 2, 4, 0) == [(0, 2), (1, 2), (2, 1), (3, 1), (4, 0)]
    assert ref.bresenham(0, 0, 2, 4) == [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4)]
    assert ref.bresenham(3, 3, 3, 3) == [(3, 3)]
    assert ref.bresenham(1, 5, 1, 2) == [(1, 2), (1, 3), (1, 4), (1, 5)]
    assert _covered((ref.SEGMENT, 5, 5, 5, 5, 3, -1, 0)) == sorted((x, y) for x in (4, 5, 6) for y in (4, 5, 6))


def test_the_closed_form_is_the_recurrence():
    """m(i) = floor((2 d i + D - 1) / (2 D)) for every segment with coordinates in -4 .. 4"""
    r = range(-4, 5)
    for x0 in r:
        for y0 in r:
            for x1 in r:
                for y1 in r:
                    path = ref.bresenham(x0, y0, x1, y1)
                    (ax, ay), (bx, by) = sorted([(x0, y0), (x1, y1)])
                    dx, dy = bx - ax, abs(by - ay)
                    D, d = max(dx, dy), min(dx, dy)
                    sy = 1 if by >= ay else -1
                    for i, (x, y) in enumerate(path):
                        m = (2 * d * i + D - 1) // (2 * D) if D else 0
                        assert (x, y) == ((ax + i, ay + sy * m) if dx >= dy else (ax + m, ay + sy * i))


def test_discs_and_rings_by_hand():
    disc2 = [(x, y) for y in range(-2, 3) for x in range(-2, 3) if (abs(x), abs(y)) != (2, 2)]
    assert len(disc2) == 21
    assert _covered((ref.DISC, 8, 8, 0, 0, 2, -1, 0)) == sorted((8 + x, 8 + y) for x, y in disc2)
    assert _covered((ref.CIRCLE, 8, 8, 1, 0, 1, -1, 0)) == sorted((8 + x, 8 + y) for x in (-1, 0, 1) for y in (-1, 0, 1) if (x, y) != (0, 0))
    assert _covered((ref.CIRCLE, 8, 8, 1, 0, 0, -1, 0)) == [(8, 8)]
    assert _covered((ref.DISC, 8, 8, 0, 0, 0, -1, 0)) == [(8, 8)]
    assert _covered((ref.CIRCLE, 0, 0, 1, 0, 1, -1, 0)) == [(0, 1), (1, 0), (1, 1)]      # clipped per pixel
    assert _covered((ref.CIRCLE, 8, 8, 3, 0, 1, -1, 0)) == _covered((ref.DISC, 8, 8, 0, 0, 2, -1, 0))   # inner radius -1: the empty set


def test_rectangles_by_hand():
    assert _covered((ref.RECT, 4, 3, 2, 2, 0, -1, 0)) == [(2, 2), (2, 3), (3, 2), (3, 3), (4, 2), (4, 3)]
    ring = _covered((ref.RECT, 2, 2, 6, 5, 1, -1, 0))
    assert len(ring) == 5 * 4 - 3 * 2 and (3, 3) not in ring and (2, 5) in ring
    assert _covered((ref.RECT, 2, 2, 6, 5, 2, -1, 0)) == _covered((ref.RECT, 2, 2, 6, 5, 0, -1, 0))


def test_text_from_glyph_rows():
    glyphs = np.zeros((95, 7), np.uint8)
    glyphs[ord("A") - 32] = [0x10, 0, 0, 0, 0, 0, 0x01]            # top-left and bottom-right pixel of the 5 x 7
    glyphs[ord("?") - 32] = [0x1F, 0, 0, 0, 0, 0, 0]
    prim = (ref.TEXT, 1, 2, 2, 0, 2, -1, 0)
    got = sorted(ref.pixels_of(prim, 32, 32, b"A\xc8", glyphs))
    a = [(1 + x, 2 + y) for x in (0, 1) for y in (0, 1)] + [(1 + 8 + x, 2 + 12 + y) for x in (0, 1) for y in (0, 1)]
    q = [(1 + 12 + x, 2 + y) for x in range(10) for y in (0, 1)]
    assert got == sorted(a + q)


def test_blend_by_hand():
    want = {1: (0, 254, 1, 255), 127: (0, 128, 127, 255), 128: (0, 127, 128, 255), 254: (0, 1, 254, 255)}
    for alpha, (c0p0, c0p255, c255p0, c255p255) in want.items():
        assert ref.blend(0, 0, alpha) == c0p0 and ref.blend(0, 255, alpha) == c0p255
        assert ref.blend(255, 0, alpha) == c255p0 and ref.blend(255, 255, alpha) == c255p255
    assert ref.blend(7, 200, 255) == 7
    img = np.full((1, 2, 2, 3), 255, np.uint8)
    prims = np.array([(ref.RECT, 0, 0, 0, 0, 0, 0x00FF00 | 128 << 24, 0), (ref.RECT, 0, 0, 0, 0, 0, 0x0000FF | 127 << 24, 0)], np.int64)
    out, covered = ref.paint(img, prims, [0, 2])
    # b: 255 -> (0*128 + 255*127 + 127)/255 = 127 -> (255*127 + 127*128 + 127)/255 = 191;  g: 255 -> 255 -> 128;  r: 127 -> 64
    assert out[0, 0, 0].tolist() == [191, 128, 64] and covered.sum() == 1 and (out[0, 1] == 255).all()

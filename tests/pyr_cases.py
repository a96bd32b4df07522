"""The images the pyramid kernels are checked on (tests/test_pyr_ref_cpu.py on the CPU, tests/test_gpu_pyr.py on the GPU).

Each case exists for one branch of camkifu_amd/csrc/k_pyramid.hip and carries the property that makes it reach that
branch, asserted on the CPU (`prop`).  The sizes below follow the kernels' tiling, restated here so that a change of
the tile sizes shows as a failing property and not as a silently weaker suite:

  one workgroup writes TILE_W x TILE_H = 64 x 16 output pixels and stages source columns 2*x0 - 4 .. 2*x0 + 131 and rows
  2*y0 - 2 .. 2*y0 + 33.  A tile is INTERIOR when that window lies inside the frame; the dword form runs when w % 8 == 0
  (and the pointers are dword aligned), the narrow form otherwise.  The first tile that can be interior is tile (1, 1):
  columns 124 .. 263 and rows 30 .. 65, so the smallest frame with an interior tile is 66 x 264 (h x w).

Every case: dict(name, make() -> uint8 (h, w, 3) or (n, h, w, 3), levels, prop(img) -> None (asserts), why)."""
import numpy as np

from . import pyr_ref

TILE_W, TILE_H = 64, 16
STAGE_W, STAGE_H = 2 * TILE_W + 8, 2 * TILE_H + 4
SMALLEST_INTERIOR = (66, 264)
ROUNDING_SHARE = 0.10


def interior_tiles(h, w):
    """tiles (ty, tx) of an h x w source that take the interior path of the dword form"""
    if w % 8:
        return []
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = []
    for ty in range((oh + TILE_H - 1) // TILE_H):
        for tx in range((ow + TILE_W - 1) // TILE_W):
            sx, sy = 2 * tx * TILE_W - 4, 2 * ty * TILE_H - 2
            if sx >= 0 and sy >= 0 and sx + STAGE_W <= w and sy + STAGE_H <= h:
                out.append((ty, tx))
    return out


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def rounding_edge(h, w, seed):
    """noise in which every third output pixel (both ways, interior windows only: the 5x5 windows do not overlap) has its
    weighted sum moved to residue 127 or 128 mod 256, alternately, through the window's corner tap of weight 1"""
    img = noise((h, w, 3), seed)
    k = 0
    for y in range(1, (h - 3) // 2 + 1, 3):
        for x in range(1, (w - 3) // 2 + 1, 3):
            img[2 * y + 2, 2 * x + 2] = 0
            s = pyr_ref.weighted_sums(img[2 * y - 2:2 * y + 3, 2 * x - 2:2 * x + 3])[1, 1]
            img[2 * y + 2, 2 * x + 2] = ((127 + (k & 1)) - s) % 256
            k += 1
    return img


def _shape_is(*shape):
    def prop(img):
        assert img.shape == shape, (img.shape, shape)
    return prop


def _all(*props):
    def prop(img):
        for p in props:
            p(img)
    return prop


def _constant(v):
    def prop(img):
        assert (img == v).all()
    return prop


def _binary(img):
    assert set(np.unique(img)) == {0, 255}


def _rounding(img):
    r = pyr_ref.weighted_sums(img) & 255
    for res in (127, 128):
        share = (r == res).mean()
        assert share >= ROUNDING_SHARE / 2, (res, share)        # stated share: a tenth of the pixels, half at each residue
    q = pyr_ref.weighted_sums(img) >> 8
    assert ((r == 128) & (q & 1 == 0)).any() and ((r == 128) & (q & 1 == 1)).any()    # both sides of a tie


def _interior(count):
    def prop(img):
        h, w = img.shape[-3:-1]
        got = len(interior_tiles(h, w))
        assert got == count if count >= 0 else got > 0, (h, w, got)          # count < 0: some
    return prop


def _narrow(img):
    assert img.shape[-2] % 8 != 0


def _dword(img):
    assert img.shape[-2] % 8 == 0


def _frames_off_a_dword(img):
    n, h, w, _ = img.shape
    assert (h * w * 3) % 4 != 0 and n >= 3


def _odd_intermediates(levels):
    def prop(img):
        h, w = img.shape[-3:-1]
        odd = 0
        for _ in range(levels - 1):
            h, w = (h + 1) // 2, (w + 1) // 2
            odd += (h & 1) + (w & 1)
            assert h >= 2 and w >= 2
        assert odd >= 1
    return prop


def _case(name, make, prop, why, levels=1, big=False):
    return dict(name=name, make=make, levels=levels, prop=prop, why=why, big=big)


H0, W0 = SMALLEST_INTERIOR
CASES = [
    _case("noise 66x264", lambda: noise((H0, W0, 3), 1), _all(_dword, _interior(1)),
          "the smallest frame with an interior tile: dword staging without reflect, next to rim tiles on all four sides"),
    _case("noise 65x264", lambda: noise((H0 - 1, W0, 3), 2), _all(_dword, _interior(0)),
          "one row less: the same tile is a rim tile of the dword form (window one row past the frame)"),
    _case("noise 66x263", lambda: noise((H0, W0 - 1, 3), 3), _all(_narrow, _interior(0)), "one column less: narrow form"),
    _case("noise 66x256", lambda: noise((H0, W0 - 8, 3), 4), _all(_dword, _interior(0)),
          "the nearest narrower dword width: rim tiles only, the window reflects on the right"),
    _case("noise 130x520", lambda: noise((130, 520, 3), 5), _all(_dword, _interior(9)), "several interior tiles, partial tiles right and below"),
    _case("constant 0", lambda: np.zeros((66, 264, 3), np.uint8), _constant(0), "smallest sums"),
    _case("constant 255", lambda: np.full((66, 264, 3), 255, np.uint8), _constant(255), "largest sums (255 * 256): no clamp needed"),
    _case("constant 255 narrow", lambda: np.full((21, 37, 3), 255, np.uint8), _all(_constant(255), _narrow), "largest sums through the reflecting rim"),
    _case("rounding edge 66x264", lambda: rounding_edge(66, 264, 6), _all(_rounding, _interior(1)), "sums at residues 127 and 128: + 128 >> 8"),
    _case("rounding edge 40x53", lambda: rounding_edge(40, 53, 7), _all(_rounding, _narrow), "the same in the narrow form"),
    _case("binary texture", lambda: (noise((66, 264, 3), 8) >> 7) * np.uint8(255), _binary, "hard 0 / 255 texture"),
    _case("checkerboard", lambda: np.broadcast_to((((np.add.outer(np.arange(67), np.arange(91))) & 1) * 255).astype(np.uint8)[..., None], (67, 91, 3)).copy(),
          _binary, "the texture a decimating filter must not alias: every output 127 or 128"),
    _case("even h odd w", lambda: noise((20, 35, 3), 9), _shape_is(20, 35, 3), "odd width: the last output column reflects"),
    _case("odd h even w", lambda: noise((21, 40, 3), 10), _shape_is(21, 40, 3), "odd height, dword width"),
    _case("odd h odd w", lambda: noise((33, 47, 3), 11), _shape_is(33, 47, 3), "both odd"),
] + [
    _case("w mod 8 = %d" % (wd % 8), (lambda wd=wd: noise((20, wd, 3), 20 + wd)), _shape_is(20, wd, 3),
          "every residue of the width: dword form at 0, narrow form elsewhere; two tile columns")
    for wd in range(136, 144)
] + [
    _case("2x2", lambda: noise((2, 2, 3), 30), _shape_is(2, 2, 3), "index -2 folds twice"),
    _case("3x3", lambda: noise((3, 3, 3), 31), _shape_is(3, 3, 3), "index n + 1 folds to n - 3 = 0"),
    _case("2x9", lambda: noise((2, 9, 3), 32), _shape_is(2, 9, 3), "the smallest height under a wider row"),
    _case("batch of 3, frames off a dword", lambda: noise((3, 5, 7, 3), 33), _frames_off_a_dword, "105-byte frames"),
    _case("batch of 4, frames off a dword", lambda: noise((4, 33, 47, 3), 34), _frames_off_a_dword, "4653-byte frames"),
    _case("batch of 3, dword form", lambda: noise((3, 66, 264, 3), 35), _all(_dword, _interior(1)), "frame stride of the dword form"),
    _case("levels 2, odd intermediates", lambda: noise((67, 101, 3), 36), _odd_intermediates(2), "67x101 -> 34x51 -> 17x26", levels=2),
    _case("levels 3, odd intermediates", lambda: noise((2, 67, 101, 3), 37), _odd_intermediates(3), "-> 9x13, ping-pong scratch, a batch", levels=3),
    _case("levels 3 of 264x528", lambda: noise((264, 528, 3), 38), _all(_dword, _interior(-1)), "dword form, then 132x264, then the narrow 66x132", levels=3),
    _case("levels 2 down to 1x1", lambda: noise((3, 4, 3), 39), _shape_is(3, 4, 3), "3x4 -> 2x2 -> 1x1: the smallest legal chain", levels=2),
    _case("1080p", lambda: noise((1080, 1920, 3), 40), _all(_dword, _interior(-1)), "a full frame", big=True),
    _case("3840x2160", lambda: noise((2160, 3840, 3), 41), _all(_dword, _interior(-1)), "a 4K frame", big=True),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)

"""Inputs of the k-means stones finder's tests, shared by the CPU file (which checks that they tell the listed mutants apart)
and the GPU file (which holds the kernel to the plain reference on them).  A case is (name, images (n, side, side, 3), zone
table (19, 19, 4), jobs (m, 5) rows of (image, rs, re, cs, ce), int_sums)."""
import numpy as np

from tests import cluster_ref as cr

SIDE = 380
CORNERS = np.array([(0, 0), (SIDE, 0), (SIDE, SIDE), (0, SIDE)], np.float32)
NINE = [(a, b, c, d) for a, b in ((0, 6), (6, 12), (12, 19)) for c, d in ((0, 6), (6, 12), (12, 19))]


def board(density, seed, hand=None):
    """a rendered goban image (the board fills the picture: intersection i at pixel 10 + 20 i) and its stones"""
    from camkifu_amd import synth
    stones = synth.random_stones(np.random.default_rng(seed), density)
    return synth.render(SIDE, SIDE, stones, CORNERS, seed=seed, hand=hand).numpy(), stones


def nine_jobs(n):
    return np.array([(f,) + reg for f in range(n) for reg in NINE], np.int32)


def noise_image(seed):
    return np.random.default_rng(seed).integers(0, 256, (SIDE, SIDE, 3)).astype(np.uint8)


def texture_image(seed, contrast=110.0):
    """a smooth random texture: three independent 1/f fields around mid-grey (contrast 200: up to 23 passes per attempt)"""
    from camkifu_amd import synth
    planes = [synth.natural_texture(SIDE, SIDE, seed=seed + k, contrast=contrast).numpy() for k in range(3)]
    return np.clip(np.stack(planes, -1) + 128.0, 0, 255).round().astype(np.uint8)


def ramp_image():
    """a slow diagonal ramp: a continuum, on which Lloyd's passes creep (many passes per attempt)"""
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    g = (x * 0.45 + y * 0.2)
    return np.clip(np.stack([g, g * 0.9 + 10, 255 - g], -1), 0, 255).round().astype(np.uint8)


def flat_image(colours):
    """vertical bands of the given BGR colours, equally wide inside every 20-pixel cell"""
    img = np.zeros((SIDE, SIDE, 3), np.uint8)
    for x in range(SIDE):
        img[:, x] = colours[(x * len(colours) // 20) % len(colours)] if len(colours) > 1 else colours[0]
    return img


def square_rects(size):
    """a made-up zone table of size x size squares from the image's corner: pixel counts to order"""
    out = np.zeros((19, 19, 4), np.int32)
    for r in range(19):
        for c in range(19):
            out[r, c] = (r * size, c * size, (r + 1) * size, (c + 1) * size)
    return out


def learned_rects(shift=(3, -2)):
    """the zone table of a grid that has learned a drift: shifted positions, rects clamped at the image's edges"""
    from camkifu_amd.stone.stonesfinder import PosGrid
    grid = PosGrid(SIDE)
    grid.mtx += np.array(shift, np.int16)
    return np.ascontiguousarray(grid.zones(1.0), np.int32)


def cases():
    rects = cr.default_rects(SIDE)
    out = []
    boards = np.stack([board(d, 40 + k)[0] for k, d in enumerate((0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7))])
    out.append(("boards", boards, rects, nine_jobs(len(boards)), False))
    out.append(("hand", board(0.4, 7, hand=(9, 9))[0][None], rects, nine_jobs(1), False))
    out.append(("noise", noise_image(3)[None], rects, nine_jobs(1), False))
    out.append(("texture", texture_image(11)[None], rects, nine_jobs(1), False))
    out.append(("creep", texture_image(21, 200.0)[None], rects, nine_jobs(1)[[0, 4, 8]], False))
    out.append(("ramp", ramp_image()[None], rects, nine_jobs(1)[[0, 4, 8]], False))
    flats = np.stack([flat_image([(20, 30, 40), (120, 130, 140), (220, 230, 240)]),
                      flat_image([(20, 30, 40), (220, 230, 240)]), flat_image([(90, 100, 110)])])
    out.append(("flat", flats, rects, np.array([(f, 6, 12, 6, 12) for f in range(3)] + [(1, 0, 6, 12, 19)], np.int32), False))
    out.append(("learned", boards[[2, 5]], learned_rects(), nine_jobs(2), False))
    sized = [(0, 0, 2, 0, 2), (0, 0, 4, 0, 4), (0, 3, 4, 3, 7), (0, 5, 6, 5, 6), (0, 2, 11, 1, 10), (0, 0, 8, 0, 10)]
    out.append(("sized16", boards[[4]], square_rects(16), np.array(sized, np.int32), False))        # 1024, 4096, 1024, 256, 20736 (streaming), 20480
    out.append(("sized20", boards[[4]], square_rects(19), np.array([(0, 0, 1, 0, 1), (0, 1, 4, 2, 7), (0, 10, 17, 3, 4)], np.int32), False))
    out.append(("one_zone", boards[[3]], rects, np.array([(0, 9, 10, 9, 10), (0, 0, 1, 18, 19)], np.int32), False))
    out.append(("columns", boards[[2, 6]], rects, np.array([(0, 0, 19, 6, 13), (1, 0, 19, 6, 13)], np.int32), False))
    out.append(("whole", boards[[5]], rects, np.array([(0, 0, 19, 0, 19)], np.int32), True))
    return out


def reference(images, rects, mask, jobs, state=0xffffffff, int_sums=False, draws=21, **rules):
    """the plain reference on every job of a call: job j starts `draws` * j numbers into the generator's sequence
    -> (list of results, state after the call)"""
    res = []
    for j, (f, a, b, c, d) in enumerate(np.asarray(jobs).reshape(-1, 5)):
        rng = cr.RNG(cr.RNG(state).advanced(draws * j))
        res.append(cr.find_stones(images[f], rects, mask, a, b, c, d, rng=rng, int_sums=int_sums, **rules))
    return res, cr.RNG(state).advanced(draws * len(res))

"""Inputs of the K1 / K2 tests (median and Canny), shared by tests/test_filter_ref_cpu.py, which asserts of every case the
property it was built for, and tests/test_gpu_filters.py, which holds the kernels to tests/filter_ref.py on them; and a model
of the path the median kernel takes through a tile, written from k_median.hip, with which those properties are asserted.

The model (median_paths): a tile is 48 x 48 medians from 64 x 64 replicate-clamped input pixels at (oy - K/2, ox - K/2).
From the 256 samples (input row r, columns 16 g + {1, 6, 9, 14}[r / 16], g = 0..3) the kernel takes the radix descent when
they span more than 28 levels.  Otherwise it scans thresholds g0, g0 + 1, .. (g0 = the rounded sample mean, at most 254)
while a block of 16 output columns still holds a median above the threshold, then g0 - 1, g0 - 2, .. while one holds a
median at or below it -- ALL 48 x 48 medians of the tile count, also those beyond the frame -- and gives up (radix descent
from scratch, bounds (0, 255)) when a direction needs a 13th threshold.  A finished scan leaves the bounds (lo, hi) of the
tile's medians that the NMS kernel uses to skip tiles: hi = the last threshold of the upward scan (255 if it ran into
254), lo = two above the last of the downward scan (0 if it ran into 0, g0 + 1 if it never started).

The K1 cases and what the model says of them, in (tile, channel) pairs per call.  A library built with -DMED_DBG=1, run
once on an MI355X over these 41 calls, printed the same tiles / scanned / given up in every one of them:

    case                      frames  tiles  scanned  given up   there for
    hidden_up                      1     90       90        90   all give up going up (samples 45, medians ~130)
    hidden_down                    1     90       90        90   all give up going down (samples 215)
    hidden_inside                  1     90       90        74   61 up, 13 down, 16 finish (samples 128 inside the medians' range)
    cap                            6    540      515        38   scans of exactly 12 that finish: 19 up, 48 down; a 13th needed:
                                                                 15 up, 23 down (two levels 13 / 14 apart, ramps of 0.40 / 0.45)
    ends                          10    900      720       109   into 254: 33 interior + 93 rim; into 0: 32 + 101; 180 radix
                                                                 tiles with medians 0 and 255
    k<K>_<big size>, K 3 .. 17     3    180       60         0   interior loads of every window: noise, smooth (radix), flat (scan)
    k<K>_<size at the condition>   3     81       27         0   tile (1, 1) interior; the two sizes one pixel less: none
                                                                 (k11_107x109: 28 scanned, 1 given up; k11_107x108: 28, 0)
    batch3 / batch4            3 / 4  180 / 240  120 / 180  60   frames off a dword; plain / remapped tile order; mixed paths
    batch3_k5 / batch4_k7      3 / 4  180 / 240   60 / 120   0   the same for the windows SfContours uses next to 13
"""
import numpy as np
from scipy import ndimage

from tests import filter_ref as fr

MT = 48                      # medians per tile edge (= the range tile of the bounds)
SAMPLE_COLS = (1, 6, 9, 14)
SCAN_RANGE, SCAN_CAP = 28, 12
NTW, NTH = 64, 28            # tile of the NMS kernel


# ------------------------------------------------------------------------------------------------ the model of K1
def sample_positions(h, w, k, by, bx):
    """-> (ys, xs): the 256 frame pixels the kernel samples for tile (by, bx), replicate-clamped"""
    r = np.repeat(np.arange(64), 4)
    cc = (16 * np.tile(np.arange(4), 64) + np.array(SAMPLE_COLS)[r // 16])
    ys = np.clip(by * MT - k // 2 + r, 0, h - 1)
    xs = np.clip(bx * MT - k // 2 + cc, 0, w - 1)
    return ys, xs


def is_interior(h, w, k, by, bx):
    ox, oy, hk = bx * MT, by * MT, k // 2
    return ox >= hk and ox - hk + 65 < w and oy >= hk and oy - hk + 63 < h


def median_paths(img, k, lo_plus=2, hi_minus=0, keep_bounds_on_give_up=False, top_at_254=False):
    """img (h, w, cn) -> list over channels of dicts keyed (by, bx): path 'radix' / 'scan' / 'gave_up', up and down (the
    thresholds evaluated each way), need_up and need_down (the thresholds a scan without a cap would take), min and max (of the
    tile's medians), gave_up_dir, hit254, hit0, lo, hi (the bounds written), g0, interior.
    The keyword arguments are mutants of the bounds for tests/test_filter_ref_cpu.py; keep_bounds_on_give_up writes what the
    kernel's own expressions give when a scan is abandoned, instead of (0, 255)."""
    img = np.asarray(img, np.uint8)
    h, w, cn = img.shape
    ty, tx = -(-h // MT), -(-w // MT)
    ext = np.pad(img, ((0, ty * MT - h), (0, tx * MT - w), (0, 0)), mode="edge")
    med = fr.median(ext, k).astype(np.int64)
    out = []
    for c in range(cn):
        tiles = {}
        for by in range(ty):
            for bx in range(tx):
                ys, xs = sample_positions(h, w, k, by, bx)
                s = img[ys, xs, c].astype(np.int64)
                t = dict(path="radix", up=0, down=0, gave_up_dir=None, hit254=False, hit0=False, lo=0, hi=255, g0=None,
                         interior=is_interior(h, w, k, by, bx))
                tiles[(by, bx)] = t
                if s.max() - s.min() > SCAN_RANGE:
                    continue
                inv = int((255 - s).sum())
                g0 = min(max(255 - ((inv + 128) >> 8), 0), 254)
                t["g0"] = g0
                m = med[by * MT:(by + 1) * MT, bx * MT:(bx + 1) * MT, c]
                blocks = [m[:, 16 * j:16 * j + 16] for j in range(3)]
                t["need_up"], t["need_down"] = int(m.max()) - g0 + 1, (g0 - int(m.min()) + 1 if m.min() <= g0 else 0)
                t["min"], t["max"] = int(m.min()), int(m.max())
                up, down = {0, 1, 2}, set()
                thr, steps, gave_up = g0, 0, None
                while up and thr <= 254:
                    if steps == SCAN_CAP:
                        gave_up = "up"
                        break
                    if thr == g0:
                        down = {j for j in up if (blocks[j] <= thr).any()}
                    up = {j for j in up if (blocks[j] > thr).any()}
                    thr += 1
                    steps += 1
                t["up"] = steps
                t["hit254"] = bool(up) and gave_up is None
                top = 255 if (up and not top_at_254) else thr - 1
                steps, thr = 0, g0 - 1
                while gave_up is None and down and thr >= 0:
                    if steps == SCAN_CAP:
                        gave_up = "down"
                        break
                    down = {j for j in down if (blocks[j] <= thr).any()}
                    thr -= 1
                    steps += 1
                t["down"] = steps
                t["hit0"] = bool(down) and gave_up is None
                if gave_up is None or keep_bounds_on_give_up:
                    t["hi"] = min(max(top - hi_minus, 0), 255)
                    t["lo"] = 0 if down else min(thr + lo_plus, 255)
                if gave_up is None:
                    t["path"] = "scan"
                else:
                    t["path"], t["gave_up_dir"] = "gave_up", gave_up
        out.append(tiles)
    return out


def count_paths(paths):
    """-> dict of how many (tile, channel) pairs took each path class"""
    n = dict(tiles=0, radix=0, scan=0, gave_up=0, gave_up_up=0, gave_up_down=0, up12=0, down12=0, up13=0, down13=0, hit254_interior=0, hit254_rim=0,
             hit0_interior=0, hit0_rim=0, interior=0)
    for tiles in paths:
        for t in tiles.values():
            n["tiles"] += 1
            n[t["path"]] += 1
            n["interior"] += t["interior"]
            if t["path"] == "gave_up":
                n["gave_up_" + t["gave_up_dir"]] += 1
                n["up13"] += t["gave_up_dir"] == "up" and t["need_up"] == SCAN_CAP + 1
                n["down13"] += t["gave_up_dir"] == "down" and t["need_down"] == SCAN_CAP + 1
            if t["path"] == "scan":
                n["up12"] += t["up"] == SCAN_CAP
                n["down12"] += t["down"] == SCAN_CAP
                for key in ("hit254", "hit0"):
                    n[key + ("_interior" if t["interior"] else "_rim")] += t[key]
    return n


def flat_nms_tiles(paths, h, w, low, first_only=False, slack=0):
    """the NMS kernel's flat test on the model's bounds -> bool array over NMS tiles: the tile is skipped (map 1 everywhere)
    when, in every channel, the largest hi minus the smallest lo of the range tiles under its pixel region (2-px halo, clamped
    to the frame) is at most low / 6.  first_only, slack: mutants."""
    gy, gx = -(-h // NTH), -(-w // NTW)
    out = np.zeros((gy, gx), bool)
    for by in range(gy):
        for bx in range(gx):
            ox, oy = bx * NTW, by * NTH
            xa, xb = max(ox - 2, 0) // MT, min(ox + NTW + 1, w - 1) // MT
            ya, yb = max(oy - 2, 0) // MT, min(oy + NTH + 1, h - 1) // MT
            flat = low >= 0
            for tiles in paths:
                under = [tiles[(y, x)] for y in range(ya, yb + 1) for x in range(xa, xb + 1)]
                if first_only:
                    under = under[:1]
                flat = flat and 6 * (max(t["hi"] for t in under) - min(t["lo"] for t in under)) <= low + slack
            out[by, bx] = flat
    return out


def canny_with_skips(planes, low, high, flat):
    """filter_ref.canny with the candidates of the NMS tiles in `flat` removed: what the kernel computes if those tiles are
    skipped.  Equal to filter_ref.canny when the bounds are right."""
    res = fr.canny(planes, low, high)
    m = res["map"].copy()
    for by, bx in zip(*np.nonzero(flat)):
        m[by * NTH:(by + 1) * NTH, bx * NTW:(bx + 1) * NTW] = 1
    return dict(map=m, edges=fr.hysteresis(m))


# ------------------------------------------------------------------------------------------------ K1 inputs
def noise(seed, h, w, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, 3)).astype(np.uint8)


def smooth(seed, h, w):
    img = ndimage.uniform_filter(noise(seed, h, w).astype(np.float32), (7, 7, 1)).astype(np.uint8)
    img[h // 4: h // 2, w // 3: 2 * w // 3] //= 3
    return img


def hidden(seed, h, w, k, sample_value, lo=60, hi=200):
    """noise everywhere except the pixels the kernel samples, in every tile, which all hold one value: the tile looks flat,
    the guess g0 is the sample value, and the medians are wherever the noise puts them"""
    img = noise(seed, h, w, lo, hi)
    for by in range(-(-h // MT)):
        for bx in range(-(-w // MT)):
            ys, xs = sample_positions(h, w, k, by, bx)
            img[ys, xs] = sample_value
    return img


def ramp(seed, h, w, slope, base=60, vertical=False):
    """a ramp of `slope` levels per pixel plus 1-level noise, the same in the three channels but for the noise"""
    y, x = np.mgrid[0:h, 0:w]
    g = base + slope * (y if vertical else x)
    return np.clip(np.floor(g)[..., None] + np.random.default_rng(seed).integers(0, 2, (h, w, 3)), 0, 255).astype(np.uint8)


def two_level(h, w, base, step, offset, period=MT, down=False):
    """columns x with (x - offset) mod period < period / 2 hold base, the others base + step (base - step if `down`): every
    tile column sees the same mix of two levels, `offset` moves the sampled columns' share of each"""
    x = np.arange(w)
    hi = ((x - offset) % period) >= period // 2
    row = np.where(hi, base - step if down else base + step, base)
    return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (h, w, 3))).astype(np.uint8)


def minority(seed, h, w, major, minor, share):
    """`major` with a random `share` of the pixels at `minor`"""
    img = np.full((h, w, 3), major, np.uint8)
    img[np.random.default_rng(seed).random((h, w, 3)) < share] = minor
    return img


def flat_noise(seed, h, w, level, span):
    return noise(seed, h, w, level, level + span + 1)


def window_sizes(k):
    """for window k: a size with interior tiles both ways and w % 4 != 0, the smallest size whose tile (1, 1) is interior, and
    one pixel less in w and in h"""
    hk = k // 2
    big = {0: (170, 203), 1: (166, 202), 2: (163, 201)}[(k // 2) % 3]
    return [big, (112 - hk, 114 - hk), (112 - hk, 113 - hk), (111 - hk, 114 - hk)]


# ------------------------------------------------------------------------------------------------ the model of K2's hysteresis
def links(m):
    """the links the kernels make between candidates (map != 1): every candidate with its W neighbour, with its N neighbour,
    and with NW and NE only where N is no candidate -> (p, q, kind) arrays, p and q flat pixel indices"""
    c = np.asarray(m) != 1
    h, w = c.shape
    z = np.zeros_like(c)
    W, N, NW, NE = z.copy(), z.copy(), z.copy(), z.copy()
    W[:, 1:] = c[:, 1:] & c[:, :-1]
    N[1:] = c[1:] & c[:-1]
    NW[1:, 1:] = c[1:, 1:] & ~c[:-1, 1:] & c[:-1, :-1]
    NE[1:, :-1] = c[1:, :-1] & ~c[:-1, :-1] & c[:-1, 1:]
    ps, qs, kinds = [], [], []
    for kind, mask, off in (("W", W, -1), ("N", N, -w), ("NW", NW, -w - 1), ("NE", NE, -w + 1)):
        p = np.flatnonzero(mask)
        ps.append(p), qs.append(p + off), kinds.append(np.full(len(p), kind))
    return np.concatenate(ps), np.concatenate(qs), np.concatenate(kinds), w


def crossings(m):
    """-> dict: how many links join two NMS tiles, by the link and by the border it crosses (side: x 63 -> 64 only; top:
    y 27 -> 28 only; corner: both)"""
    p, q, kind, w = links(m)
    out = {}
    for a, b, k in zip(p, q, kind):
        sx, sy = (a % w) // NTW != (b % w) // NTW, (a // w) // NTH != (b // w) // NTH
        if sx or sy:
            key = k + "_" + ("corner" if sx and sy else "side" if sx else "top")
            out[key] = out.get(key, 0) + 1
    return out


def tiled_hysteresis(m, skip_last_column=False, skip_top_row=False, local_ne=True):
    """the edges as the kernels find them: links inside an NMS tile are made by the tile itself (all of them; NE is left out
    with local_ne=False), a link to another tile only by a candidate in a tile's first or last column or first row, which
    then makes all its links.  The other two switches remove the last column / the first row from that rule: the mutants of
    the link kernel.  Without mutants this is filter_ref.hysteresis."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    m = np.asarray(m)
    p, q, kind, w = links(m)
    x, y = p % w, p // w
    local = ((x // NTW) == ((q % w) // NTW)) & ((y // NTH) == ((q // w) // NTH))
    visited = (x % NTW == 0) | ((x % NTW == NTW - 1) & (not skip_last_column)) | ((y % NTH == 0) & (not skip_top_row))
    made = (local & (local_ne | (kind != "NE"))) | visited
    n = m.size
    g = coo_matrix((np.ones(made.sum(), np.int8), (p[made], q[made])), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    lab = lab.reshape(m.shape)
    strong = np.unique(lab[m == 2])
    return (np.isin(lab, strong) & (m != 1)).astype(np.uint8) * 255


# ------------------------------------------------------------------------------------------------ K2 inputs
def texture(seed, h, w):
    """hard 0 / 255 texture (the largest magnitudes), the right part with three identical channels (ties: the first channel
    wins), a patch of noise"""
    rng = np.random.default_rng(seed)
    img = (rng.random((h, w, 3)) < 0.5).astype(np.uint8) * 255
    img[:, w // 2:] = img[:, w // 2:, :1]
    img[h // 4: h // 2, w // 8: 3 * w // 8] = rng.integers(0, 256, (h // 2 - h // 4, 3 * w // 8 - w // 8, 3), dtype=np.uint8)
    return img


def grey_smooth(seed, h, w):
    """a smooth image with three identical channels: every pixel is a tie between the channels"""
    return np.ascontiguousarray(np.repeat(smooth(seed, h, w)[..., :1], 3, axis=2))


def step_image(h, w, x0, y0, run_x, run_y, strong=None, step=10, base=100):
    """grey `base`, and base + step on one side of the line through (x0, y0) with direction (run_x, run_y): the side where
    run_x (y - y0) - run_y (x - x0) >= 0; three equal channels.  A step of 10 gives a chain of candidates of magnitude 40 (60 on
    a slant): weak for the thresholds (25, 75).  strong = (axis, start, sign): the raised side rises further, by 2 levels per
    pixel and 30 at most, from coordinate `start` of that axis ('x' or 'y') on in direction `sign` -- a taper towards the frame's
    edge, without a border of its own, that lifts the end of the chain above `high`."""
    y, x = np.mgrid[0:h, 0:w]
    side = run_x * (y - y0) - run_y * (x - x0) >= 0
    img = np.full((h, w), base, np.int64)
    img[side] = base + step
    if strong is not None:
        axis, start, sign = strong
        img[side] += np.clip(sign * ((x if axis == "x" else y) - start) * 2, 0, 30)[side]
    return np.ascontiguousarray(np.repeat(img.astype(np.uint8)[..., None], 3, axis=2))


# (name, x0, y0, run_x, run_y, the taper that makes one end strong, the crossings between NMS tiles the case is there for)
CHAINS = [
    ("horizontal", 0, 60, 1, 0, ("x", 270, 1), ("W_side",)),
    ("vertical", 150, 0, 0, 1, ("y", 18, -1), ("N_top",)),
    ("down_right", 192, 56, 2, 1, ("y", 12, -1), ("NW_corner", "NW_side", "NW_top")),
    ("up_right", 191, 56, 2, -1, ("y", 125, 1), ("NE_corner", "NE_side", "NE_top")),
    ("steep_down_right", 100, 56, 1, 2, ("y", 18, -1), ("N_top", "NW_side")),
    ("steep_up_right", 110, 56, 1, -2, ("y", 125, 1), ("N_top", "NE_side")),
]
CHAIN_SHAPE = (140, 300)


def chain_image(name, strong=True):
    _, x0, y0, rx, ry, taper, _ = next(c for c in CHAINS if c[0] == name)
    return step_image(CHAIN_SHAPE[0], CHAIN_SHAPE[1], x0, y0, rx, ry, taper if strong else None)


def blobs(seed, left, right, side=380, sigma=25.0):
    """two dark plateaus (`left` in the left half, `right` in the right), each with large blobs one level higher where a
    Gaussian-filtered random field is positive: the Otsu level lands between the plateaus, Canny's thresholds are a few
    levels, and the blobs' outlines (magnitude 4 at most) are weak chains that hang on the plateaus' border -- inside range
    tiles whose medians span exactly one level"""
    field = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal((side, side)), sigma)
    img = np.where(np.arange(side)[None, :] < side // 2, left, right) + (field > 0)
    return np.ascontiguousarray(np.repeat(img.astype(np.uint8)[..., None], 3, axis=2))


def span5(h=330, w=520):
    """for the board thresholds (25, 75): a diagonal step of 5 levels -- magnitude 30: weak, and its range tiles span exactly 5
    levels, one more than the NMS kernel may skip -- whose raised side tapers up to 35 levels towards the top of the frame:
    the weak chain hangs on strong pixels many NMS tiles away.  (Found by drawing it: a step that ends in a block of another
    level loses its connection at the junction; the taper has no border of its own and passes the median.)"""
    return step_image(h, w, 60, 0, 1, 1, ("y", 40, -1), step=5)


def span5_top(h=330, w=520):
    """the same drawing at the top of the range: 255 with a side at 250 that tapers down to 220 -- the scan of its tiles runs
    into threshold 254, whose bound has to be 255"""
    return 255 - step_image(h, w, 60, 0, 1, 1, ("y", 40, -1), step=5, base=0)


def striped(h=200, w=250, high=230, low=205, dark=140, dark_rows=60):
    """a scan that gives up in the SECOND median of goban_canny, whose input the first median has filtered: stripes 8 wide
    of `low` on `high`, 25 levels apart, shifted from one band of 16 rows to the next so that they miss every pixel the
    median-7 pass samples (columns = -3 + {1, 6, 9, 14} mod 16 by band; the band of a tile's last 16 rows is the next tile's
    first, and misses both sets) and are wide enough to pass the median-13 pass in front of it: the samples say 230, the scan
    finds no median above that and gives up 12 levels below.  A dark top of `dark` puts the Otsu level there: thresholds
    (70, 140), under which the stripes' outlines (magnitude 100 and more) are candidates, some of them strong."""
    y, x = np.mgrid[0:h, 0:w]
    start = np.choose(((y + 3) // 16) % 3, [1, 7, 10])
    img = np.where((x - start) % 16 < 8, low, high)
    img[:dark_rows] = dark
    return np.ascontiguousarray(np.repeat(img.astype(np.uint8)[..., None], 3, axis=2))


# ------------------------------------------------------------------------------------------------ the cases
K1_SHAPE = (200, 250)        # 5 x 6 tiles, 2 x 3 of them interior for K = 15: 90 (tile, channel) pairs per frame
BATCH_SHAPE = (163, 201)     # 163 * 201 * 3 % 4 == 1: every frame but the first starts off a dword; 4 x 5 tiles, (1..2, 1..2) interior


def median_cases():
    """-> list of (name, k, frames (n, h, w, 3), wants): wants = the least number of (tile, channel) pairs, over the frames, that
    the model must put in each path class named (count_paths), which tests/test_filter_ref_cpu.py asserts"""
    h, w = K1_SHAPE
    out = [
        ("hidden_up", 15, hidden(1, h, w, 15, 45)[None], dict(gave_up_up=80)),
        ("hidden_down", 15, hidden(2, h, w, 15, 215)[None], dict(gave_up_down=80)),
        ("hidden_inside", 15, hidden(3, h, w, 15, 128, 0, 256)[None], dict(gave_up_up=8, gave_up_down=8, scan=8)),
        ("cap", 15, np.stack([two_level(h, w, 100, 13, 4), two_level(h, w, 100, 13, 28), two_level(h, w, 100, 14, 2),
                              two_level(h, w, 100, 14, 26), ramp(4, h, w, 0.40), ramp(4, h, w, 0.45)]),
         dict(up12=8, down12=8, up13=8, down13=8, scan=300)),
        ("ends", 15, np.stack([np.full((h, w, 3), v, np.uint8) for v in (0, 1, 254, 255)]
                              + [minority(5, h, w, 255, 230, 0.4), minority(6, h, w, 0, 25, 0.4), minority(7, h, w, 255, 0, 0.2),
                                 minority(8, h, w, 0, 255, 0.2), flat_noise(9, h, w, 250, 5), flat_noise(10, h, w, 0, 5)]),
         dict(hit254_interior=8, hit254_rim=8, hit0_interior=8, hit0_rim=8, radix=100)),
    ]
    for k in range(3, 19, 2):
        for j, (hh, ww) in enumerate(window_sizes(k)):
            frames = np.stack([noise(100 * k + j, hh, ww), smooth(100 * k + j, hh, ww),
                               np.minimum(flat_noise(100 * k + j, hh, ww, 98, 3) + ramp(k, hh, ww, 0.1, 0), 255).astype(np.uint8)])
            out.append(("k%d_%dx%d" % (k, hh, ww), k, frames, dict(radix=8, scan=8) if j == 0 else dict()))
    hh, ww = BATCH_SHAPE
    mix = np.stack([noise(21, hh, ww), flat_noise(22, hh, ww, 120, 4), hidden(23, hh, ww, 15, 215), np.full((hh, ww, 3), 255, np.uint8)])
    out.append(("batch3", 15, mix[:3], dict(radix=8, scan=8, gave_up=8)))       # 20 tiles x 9 planes: no multiple of 8
    out.append(("batch4", 15, mix, dict(radix=8, scan=8, gave_up=8)))           # 20 x 12: the remapped tile order
    out.append(("batch3_k5", 5, mix[:3], dict()))
    out.append(("batch4_k7", 7, mix, dict()))
    return out


def canny_cases():
    """-> list of (name, frames, low, high) for the Canny call alone (the map is compared)"""
    out = [
        ("noise", noise(31, 200, 300)[None], 25, 75),
        ("noise_dense", noise(32, 200, 300)[None], 0, 100),
        ("texture", texture(33, 200, 300)[None], 100, 1000),
        ("texture_swapped", texture(34, 200, 300)[None], 2039, 1),
        ("equal_channels", grey_smooth(35, 200, 300)[None], 25, 75),
    ]
    for hh, ww in ((57, 135), (57, 136), (58, 135), (58, 136)):                   # tile (1, 1) of the NMS kernel is interior from 58 x 136 on
        out.append(("edge_%dx%d" % (hh, ww), np.stack([noise(hh + ww, hh, ww), smooth(hh * ww, hh, ww)]), 25, 75))
    odd = np.stack([noise(36, 135, 201), texture(37, 135, 201), smooth(38, 135, 201), grey_smooth(39, 135, 201)])
    out.append(("odd_batch3", odd[:3], 25, 75))                                   # 3 x 5 x 4 tiles x 3: no multiple of 8
    out.append(("odd_batch4", odd, 25, 75))                                       # x 4: the remapped tile order
    for name, *_ in CHAINS:                                                       # frame 0 is noise: the chain is a frame >= 1
        for strong in (True, False):
            out.append(("chain_%s_%s" % (name, "strong" if strong else "weak"),
                        np.stack([noise(40, *CHAIN_SHAPE), chain_image(name, strong)]), 25, 75))
    return out


def goban_chain_image(name, strong=True):
    """the chain drawings for Otsu thresholds: grey 100 with a step of 15 has its Otsu level at 100, thresholds (50, 100), and
    chains of magnitude 60 (90 on a slant); straight steps pass the two medians unchanged"""
    _, x0, y0, rx, ry, taper, _ = next(c for c in CHAINS if c[0] == name)
    return step_image(CHAIN_SHAPE[0], CHAIN_SHAPE[1], x0, y0, rx, ry, taper if strong else None, step=15)


def goban_cases():
    """-> list of (name, frames) for goban_canny: median 13, median 7, per-frame Otsu thresholds"""
    out = [("blobs", np.stack([blobs(5, 3, 7), blobs(6, 2, 6), blobs(7, 1, 4)]))]
    chains = [goban_chain_image(name, strong) for name, *_ in CHAINS for strong in (True, False)]
    out.append(("chains", np.stack([noise(41, *CHAIN_SHAPE)] + chains)))           # 13 frames x 15 tiles: per-frame thresholds, no remap
    out.append(("chains_remap", np.stack(chains + [noise(42, *CHAIN_SHAPE)] * 4)))   # 16 frames: the remapped order permutes the frames
    hh, ww = BATCH_SHAPE
    out.append(("mix", np.stack([noise(43, hh, ww), smooth(44, hh, ww), hidden(45, hh, ww, 7, 215), two_level(hh, ww, 100, 14, 26),
                                 np.full((hh, ww, 3), 90, np.uint8)])))
    out.append(("striped", np.stack([striped(), striped(dark_rows=40)])))
    return out


def board_cases(big=True):
    """-> list of (name, frames) for board_edges: median 15, Canny (25, 75)"""
    h, w = K1_SHAPE
    out = [("span5", np.stack([span5(), span5_top(), np.full((330, 520, 3), 7, np.uint8)])),
           ("chains", np.stack([chain_image(name, strong) for name, *_ in CHAINS for strong in (True, False)])),
           ("ends", np.stack([minority(5, h, w, 255, 230, 0.4), minority(6, h, w, 0, 25, 0.4), two_level(h, w, 100, 40, 4),
                              hidden(2, h, w, 15, 215), smooth(46, h, w)]))]
    if big:
        out.append(("scene_1080p", scene(1080, 1920, 9)[None]))
    return out


def scene(h, w, seed):
    """a rendered camera frame of a board on a table (the library's own synthetic scenes)"""
    from camkifu_amd import synth
    return synth.scene(h, w, seed=seed)["frame"].numpy()

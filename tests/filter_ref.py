"""Plain references of the two byte filters in front of the board path and of SfContours.get_canny -- cv2.medianBlur (K1,
k_median.hip) and cv2.Canny with the L1 gradient and aperture 3 on a 3-channel image (K2, k_canny.hip), cvtColor BGR2GRAY and
the Otsu level -- written from the definitions (OpenCV 3.1) with numpy and scipy, vectorised so that a 1080p frame is
affordable.  They share no code with the CPU restatement in C or with the library: tests/test_filter_ref_cpu.py holds the two
against each other, tests/test_gpu_filters.py holds the kernels to these.

median: replicate border, the element of rank (k k) / 2 (0-based) of the k x k window, per channel.  Three forms that check each
other: scipy's rank filter, threshold counting with integral images, np.partition over sliding windows.
canny: Sobel 3 x 3 on the replicated image, |dx| + |dy|, the first channel of largest magnitude, non-maximum suppression with
the fixed-point tangent test (TG22 = 13573 = round(tan 22.5 * 2^15); `>` towards the first neighbour, `>=` towards the second
in the horizontal and vertical sectors, `>` both ways on the diagonals; magnitudes beyond the image count as 0), map 1 = not a
candidate, 0 = candidate, 2 = candidate above `high`; an edge is a candidate whose 8-connected component of candidates holds
a 2."""
import numpy as np
from scipy import ndimage

TG22 = 13573


# ------------------------------------------------------------------------------------------------ median
def _planes(img):
    img = np.asarray(img, np.uint8)
    return img[..., None] if img.ndim == 2 else img


def median_rank(img, k):
    """scipy's rank filter, one window per pixel and channel"""
    p = _planes(img)
    return ndimage.median_filter(p, size=(k, k, 1), mode="nearest").reshape(np.shape(img))


def median_counting(img, k):
    """median = number of levels t in 0 .. 254 for which fewer than (k k + 1) / 2 pixels of the window are <= t; the window
    counts of one level are a box sum, taken from an integral image"""
    p = _planes(img)
    h, w, cn = p.shape
    r, need = k // 2, (k * k + 1) // 2
    out = np.zeros((h, w, cn), np.uint8)
    for c in range(cn):
        e = np.pad(p[..., c], r, mode="edge")
        for t in range(int(e.min()), int(e.max())):            # below the minimum every count is 0, from the maximum on k k
            s = np.zeros((h + 2 * r + 1, w + 2 * r + 1), np.int32)
            s[1:, 1:] = np.cumsum(np.cumsum(e <= t, axis=0, dtype=np.int32), axis=1, dtype=np.int32)
            count = s[k:, k:] - s[:-k, k:] - s[k:, :-k] + s[:-k, :-k]
            out[..., c] += count < need
        out[..., c] += e.min()
    return out.reshape(np.shape(img))


def median_partition(img, k):
    """the k k values of every window side by side, np.partition picks rank (k k) / 2: for small images"""
    p = _planes(img)
    r = k // 2
    e = np.pad(p, ((r, r), (r, r), (0, 0)), mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(e, (k, k), axis=(0, 1)).reshape(p.shape + (k * k,))
    return np.partition(win, (k * k) // 2, axis=-1)[..., (k * k) // 2].reshape(np.shape(img))


def median(img, k):
    return median_rank(img, k)


# ------------------------------------------------------------------------------------------------ canny
def sobel(img):
    """-> dx, dy (h, w, cn) int32 of the edge-replicated image"""
    p = np.pad(_planes(img).astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    left, right = p[:, :-2], p[:, 2:]
    dx = (right[:-2] + 2 * right[1:-1] + right[2:]) - (left[:-2] + 2 * left[1:-1] + left[2:])
    top, bottom = p[:-2], p[2:]
    dy = (bottom[:, :-2] + 2 * bottom[:, 1:-1] + bottom[:, 2:]) - (top[:, :-2] + 2 * top[:, 1:-1] + top[:, 2:])
    return dx, dy


def canny(img, low, high, first_channel=True, sector0_strict=False):
    """-> dict(edges 0 / 255, map {0, 1, 2}, mag, dx, dy, channel).  The two switches are mutants of the tie rules (the last
    maximal channel; `>` on both sides of the horizontal sector) for tests/test_filter_ref_cpu.py."""
    low, high = int(low), int(high)
    if low > high:
        low, high = high, low
    dx3, dy3 = sobel(img)
    mag3 = np.abs(dx3) + np.abs(dy3)
    cn = mag3.shape[2]
    ch = np.argmax(mag3, axis=2) if first_channel else cn - 1 - np.argmax(mag3[..., ::-1], axis=2)
    pick = lambda a: np.take_along_axis(a, ch[..., None], axis=2)[..., 0]
    dx, dy, mag = pick(dx3), pick(dy3), pick(mag3)
    h, w = mag.shape
    mp = np.pad(mag, 1)                                      # beyond the image: 0
    at = lambda oy, ox: mp[1 + oy: 1 + oy + h, 1 + ox: 1 + ox + w]
    ax, ay = np.abs(dx).astype(np.int64), np.abs(dy).astype(np.int64) << 15
    t = ax * TG22
    horizontal, vertical = ay < t, ay > t + (ax << 16)
    if sector0_strict:
        keep_h = (mag > at(0, -1)) & (mag > at(0, 1))
    else:
        keep_h = (mag > at(0, -1)) & (mag >= at(0, 1))
    keep_v = (mag > at(-1, 0)) & (mag >= at(1, 0))
    anti = (dx ^ dy) < 0                                     # signs differ: the neighbours are NE and SW
    keep_d = np.where(anti, (mag > at(-1, 1)) & (mag > at(1, -1)), (mag > at(-1, -1)) & (mag > at(1, 1)))
    keep = np.where(horizontal, keep_h, np.where(vertical, keep_v, keep_d)) & (mag > low)
    m = np.where(keep, np.where(mag > high, 2, 0), 1).astype(np.uint8)
    return dict(edges=hysteresis(m), map=m, mag=mag, dx=dx, dy=dy, channel=ch)


def hysteresis(m):
    lab, _ = ndimage.label(m != 1, structure=np.ones((3, 3), int))
    strong = np.unique(lab[m == 2])
    return (np.isin(lab, strong[strong > 0]) * 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ grey, Otsu, the two chains
def bgr2gray(img):
    """8-bit BGR -> grey: weights 0.114, 0.587, 0.299 as 14-bit fixed point (1868, 9617, 4899), rounded"""
    a = np.asarray(img, np.uint8).astype(np.int64)
    return ((a @ np.array([1868, 9617, 4899], np.int64) + 8192) >> 14).astype(np.uint8)


def otsu_level(gray):
    """the level of largest between-class variance, in doubles: a level is passed over while either class holds less than
    FLT_EPSILON of the pixels; the first maximum wins"""
    n = np.bincount(np.asarray(gray, np.uint8).ravel(), minlength=256)
    scale = 1.0 / float(n.sum())
    mu = float(np.dot(np.arange(256, dtype=np.float64), n.astype(np.float64))) * scale
    eps = float(np.float32(2.0) ** -23)
    best, level = 0.0, 0
    q1 = mu1 = 0.0
    for i in range(256):
        p = float(n[i]) * scale
        mu1 *= q1
        q1 += p
        q2 = 1.0 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1.0 - eps:
            continue
        mu1 = (mu1 + i * p) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > best:
            best, level = sigma, i
    return float(level)


def goban_canny(img, **rules):
    """median 13, median 7, Otsu level of the grey image, canny(floor(otsu / 2), floor(otsu))
    -> dict of canny plus otsu, median (the image Canny saw), low, high"""
    m = median(median(img, 13), 7)
    otsu = otsu_level(bgr2gray(m))
    low, high = int(np.floor(otsu / 2)), int(np.floor(otsu))
    out = canny(m, low, high, **rules)
    out.update(otsu=otsu, median=m, low=low, high=high)
    return out


def board_edges(img, **rules):
    m = median(img, 15)
    out = canny(m, 25, 75, **rules)
    out.update(median=m, low=25, high=75)
    return out

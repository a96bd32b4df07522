"""Plain references for cv2.pyrDown of 8-bit images (OpenCV 3.1.0, BORDER_DEFAULT), test-only.

    dst[y, x] = (sum_{i,j in -2..2} k[i] k[j] src[r(2y+i), r(2x+j)] + 128) >> 8,  k = 1 4 6 4 1,  r = BORDER_REFLECT_101

Two forms that share no code with the library or with each other:

  pyr_down        separable integer passes over an np.pad(mode="reflect") image
  pyr_down_scipy  scipy.ndimage.correlate of the 5x5 outer-product kernel with mode="mirror", then [::2, ::2]

and MUTANTS of the first form, each one plausible mistake (tests/test_pyr_ref_cpu.py shows that the cases of
tests/pyr_cases.py tell every one of them from the reference).  Images are (h, w) or (h, w, c); batches (n, h, w, c)
go through `pyr_down_batch`."""
import numpy as np

K = np.array([1, 4, 6, 4, 1], np.int64)
PAD = 3          # two for the filter, one more so that a mutant may shift it


def weighted_sums(img, mode="reflect", dx=0, dy=0):
    """the sums before rounding, int64 ((h+1)//2, (w+1)//2[, c]): taps centred at (2y + dy, 2x + dx) on an image
    padded with np.pad(mode)"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim in (2, 3) and min(a.shape[:2]) >= 2, (a.dtype, a.shape)
    h, w = a.shape[:2]
    oh, ow = (h + 1) // 2, (w + 1) // 2
    p = np.pad(a.astype(np.int64), ((PAD, PAD), (PAD, PAD)) + ((0, 0),) * (a.ndim - 2), mode=mode)
    x0, y0 = PAD - 2 + dx, PAD - 2 + dy
    rows = sum(K[j] * p[:, x0 + j:x0 + j + 2 * ow:2] for j in range(5))              # (h + 2 PAD, ow)
    return sum(K[i] * rows[y0 + i:y0 + i + 2 * oh:2] for i in range(5))              # (oh, ow)


def pyr_down(img):
    return ((weighted_sums(img) + 128) >> 8).astype(np.uint8)


def pyr_down_scipy(img):
    from scipy import ndimage
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    k2 = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]).astype(np.int32)
    planes = a[..., None] if a.ndim == 2 else a
    out = [ndimage.correlate(planes[..., c].astype(np.int32), k2, mode="mirror")[::2, ::2] for c in range(planes.shape[-1])]
    out = ((np.stack(out, -1) + 128) // 256).astype(np.uint8)
    return out[..., 0] if a.ndim == 2 else out


def pyr_down_levels(img, levels):
    for _ in range(levels):
        img = pyr_down(img)
    return img


def pyr_down_batch(frames, levels=1):
    """(n, h, w, c) or one image -> the same rank, `levels` times smaller"""
    a = np.asarray(frames)
    if a.ndim == 4:
        return np.stack([pyr_down_levels(f, levels) for f in a])
    return pyr_down_levels(a, levels)


def pyr_shape(h, w, levels):
    for _ in range(levels):
        assert h >= 2 and w >= 2
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


def _round(s):
    return ((s + 128) >> 8).astype(np.uint8)


def _half_even(s):
    q, r = s >> 8, s & 255
    return (q + ((r > 128) | ((r == 128) & (q & 1 == 1)))).astype(np.uint8)


MUTANTS = {
    "replicate border": lambda img: _round(weighted_sums(img, mode="edge")),
    "reflect without the 101": lambda img: _round(weighted_sums(img, mode="symmetric")),
    "truncation instead of +128": lambda img: (weighted_sums(img) >> 8).astype(np.uint8),
    "round half to even": lambda img: _half_even(weighted_sums(img)),
    "kernel shifted by one pixel": lambda img: _round(weighted_sums(img, dx=-1)),
    "centre at 2x+1": lambda img: _round(weighted_sums(img, dx=1, dy=1)),
}

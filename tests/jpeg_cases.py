"""The cases of the JPEG tests: the committed fixtures (tools/make_jpeg_fixtures.py) and synthetic coefficient sets for
the GPU half alone.  References are computed once per process and shared (treat them as read-only)."""
import functools
import glob
import os

import numpy as np

from . import jpeg_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AVI = os.path.join(GOLDEN, "tiny.avi")


@functools.lru_cache(maxsize=None)
def file_cases():
    """{name: (jpeg bytes, expected BGR)} of every committed case"""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "jpeg_cases*.npz"))):
        with np.load(path) as z:
            for k in z.files:
                if k.startswith("j_"):
                    out[k[2:]] = (z[k].tobytes(), z["e_" + k[2:]])
    return out


@functools.lru_cache(maxsize=None)
def batch_case():
    """([jpeg bytes] * 5, expected (5, 136, 200, 3))"""
    with np.load(os.path.join(GOLDEN, "jpeg_batch.npz")) as z:
        return [z["j_%d" % k].tobytes() for k in range(5)], np.stack([z["e_%d" % k] for k in range(5)])


@functools.lru_cache(maxsize=None)
def ref_coefficients(name):
    return jpeg_ref.coefficients(file_cases()[name][0])


def names(stride=1, offset=0):
    return sorted(file_cases())[offset::stride]


# ---- synthetic coefficients for ck_jpeg_reconstruct ------------------------------------------------------------------------
SAMPLINGS = (jpeg_ref.GREY, jpeg_ref.S444, jpeg_ref.S422, jpeg_ref.S420)
KINDS = ("dc_only", "one_ac", "sparse", "range_ends")


def _quant(rng, flat=False):
    q = np.ones((3, 64), np.uint16) if flat else rng.integers(1, 40, (3, 64)).astype(np.uint16)
    return q


def one_ac_starts(nb):
    """the frames of the "one_ac" set: frame k drives AC position (b + start_k) % 63 + 1 alone in block b, and together the
    frames drive every position 1..63 alone -- a frame of nb blocks covers nb of them"""
    return list(range(0, 63, min(nb, 63)))


def synthetic(kind, h, w, sampling, start=0):
    """-> (coef (blocks * 64,) int16, quant (3, 64) uint16): one frame of one of KINDS for a frame of h x w.  Magnitudes
    stay where every intermediate of the inverse DCT fits int32 (jpeg_ref asserts it when the reference is computed)."""
    nb = jpeg_ref.n_blocks(h, w, sampling)
    rng = np.random.default_rng(KINDS.index(kind) * 1000 + h * 37 + w * 5 + sampling + 100000 * start)
    coef = np.zeros((nb, 64), np.int64)
    quant = _quant(rng)
    if kind == "dc_only":
        coef[:, 0] = rng.integers(-60, 61, nb)
    elif kind == "one_ac":
        coef[:, 0] = rng.integers(-20, 21, nb)
        pos = (np.arange(nb) + start) % 63 + 1                       # one AC position per block, consecutive ones
        coef[np.arange(nb), pos] = rng.integers(-30, 31, nb) | 1
    elif kind == "sparse":
        for b in range(nb):
            k = rng.integers(1, 9)
            coef[b, rng.integers(0, 64, k)] = rng.integers(-25, 26, k)
    elif kind == "range_ends":
        # samples far past both ends of the range table's ramp (DC alone: -128 - 255 .. 127 + 255) and, with the AC terms,
        # beyond the table's 1024 entries, where it wraps
        quant = _quant(rng, flat=True)
        coef[:, 0] = np.where(np.arange(nb) & 1, 2040, -2040)
        coef[::3, 1] = 3000
        coef[1::3, 8] = -3000
        coef[2::3, 63] = 1023
    else:
        raise ValueError(kind)
    return coef.reshape(-1).astype(np.int16), quant


@functools.lru_cache(maxsize=None)
def synthetic_case(kind, h, w, sampling):
    """-> (coef (frames, blocks * 64), quant (frames, 3, 64), expected (frames, h, w, 3)): one frame, except "one_ac", which
    has as many as it takes to drive each of the 63 AC positions alone in some block"""
    nb = jpeg_ref.n_blocks(h, w, sampling)
    starts = one_ac_starts(nb) if kind == "one_ac" else [0]
    frames = [synthetic(kind, h, w, sampling, start) for start in starts]
    coef, quant = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    if kind == "one_ac":
        blocks = coef.reshape(-1, 64)
        ac = blocks[:, 1:] != 0
        assert (ac.sum(axis=1) == 1).all(), "a block with other than one AC coefficient"
        assert set(np.nonzero(ac)[1] + 1) == set(range(1, 64)), "an AC position that no block drives alone"
    exp = np.stack([jpeg_ref.reconstruct(c, q, h, w, sampling) for c, q in zip(coef, quant)])
    return coef, quant, exp


def synthetic_shapes():
    """(h, w, sampling): 17 x 33 for all four samplings and grey at 8 x 8"""
    return [(17, 33, s) for s in SAMPLINGS] + [(8, 8, jpeg_ref.GREY)]


def strip_dht(data):
    """the stream without its DHT segments (a Motion-JPEG frame as AVI files hold them)"""
    segs, scan_at = jpeg_ref.segments(data)
    out, p = bytearray(data[:2]), 2
    for m, o, ln in segs:
        if m != 0xC4:
            out += data[o - 4:o + ln]
    return bytes(out) + data[scan_at:]


@functools.lru_cache(maxsize=None)
def avi_reference():
    """(index dict of tiny.avi, [BGR frame or None per chunk] with the repeat rule applied)"""
    with open(AVI, "rb") as f:
        idx = jpeg_ref.avi_index(f.read())
    frames, last = [], None
    for c in idx["chunks"]:
        if len(c):
            last = jpeg_ref.decode(c)
        frames.append(last)
    return idx, frames

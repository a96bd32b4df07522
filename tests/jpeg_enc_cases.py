"""The cases of the JPEG encoder tests.  Inputs are regenerated here from seeds; the committed fixtures
(tests/golden/jpeg_enc_cases*.npz, written by tools/make_jpeg_enc_fixtures.py) hold Pillow's bytes only.  References are
computed once per process and shared (treat them as read-only).

A case is (content, h, w, sampling, quality, restart interval in MCUs); its name spells the six out."""
import functools
import glob
import os
import zlib

import numpy as np

from . import jpeg_enc_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SNAME = {ref.GREY: "grey", ref.S444: "444", ref.S422: "422", ref.S420: "420"}
SAMPLINGS = (ref.GREY, ref.S444, ref.S422, ref.S420)
CONTENTS = ("noise", "ramp", "checker", "fine")

# (h, w): smallest image; three dummy luma blocks at 4:2:0; exact MCUs; one short of / one over a block both ways; portrait;
# the tile seams of the kernel at 64 across and 32 down; whole tiles
SHAPES = [(1, 1), (8, 8), (16, 32), (15, 31), (17, 33), (33, 17), (65, 33), (33, 70), (48, 64)]
QUALITIES = (1, 50, 90, 100)


def name_of(case):
    content, h, w, s, q, ri = case
    return "%s_%dx%d_%s_q%d_r%d" % (content, h, w, SNAME[s], q, ri)


def image(content, h, w, seed=0):
    """BGR (h, w, 3) uint8"""
    rng = np.random.default_rng(zlib.crc32(("%s %d %d %d" % (content, h, w, seed)).encode()))
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if content == "ramp":
        img = np.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 5 + 40) % 256, 255 - (xx + yy) * 4 % 256], axis=2)
        return (img + rng.integers(0, 3, (h, w, 3))).clip(0, 255).astype(np.uint8)
    if content == "checker":                         # 8-pixel cells on the block grid: solid blocks of 0 and of 255
        return np.repeat(((((xx >> 3) + (yy >> 3)) & 1) * 255)[:, :, None], 3, axis=2).astype(np.uint8)
    if content == "fine":                            # cells of 1, 2 and 3 pixels, one size per channel
        return np.stack([((((xx + k) // c + yy // c) & 1) * 255) for k, c in enumerate((1, 2, 3))], axis=2).astype(np.uint8)
    raise ValueError(content)


@functools.lru_cache(maxsize=None)
def forward_cases():
    """every shape x sampling x quality of the kernel's test, the content rotating"""
    out, k = [], 0
    for h, w in SHAPES:
        for s in SAMPLINGS:
            for q in QUALITIES:
                out.append((CONTENTS[(k + k // 4) % len(CONTENTS)], h, w, s, q, 0))
                k += 1
    return out


def forward_case(h, w, s, q):
    return next(c for c in forward_cases() if c[1:5] == (h, w, s, q))


# restart intervals of 1, 3 and 7 MCUs (12 MCUs at 4:2:0, so RSTn wraps at interval 1) and of one MCU row of an image of
# 10 MCU rows; quant tables at the qualities around the two branches of the scaling; solid 0 / 255 blocks at quality 100
# (DC differences of 11 bits) and fine checkers (AC values of 10 bits, blocks that end on coefficient 63); a smooth image at
# low quality (ZRL runs); noise at quality 100 (stuffed bytes)
EXTRA = [("noise", 48, 64, ref.S420, 90, 1), ("ramp", 48, 64, ref.S420, 90, 3), ("noise", 48, 64, ref.S422, 50, 7),
         ("ramp", 17, 33, ref.S420, 90, 3), ("noise", 17, 33, ref.GREY, 90, 1), ("fine", 33, 70, ref.S444, 100, 7),
         ("noise", 80, 24, ref.S444, 90, 3), ("ramp", 80, 24, ref.GREY, 50, 3)] + \
        [("ramp", 8, 8, ref.S444, q, 0) for q in (2, 49, 51, 99)] + \
        [("checker", 16, 32, ref.S444, 100, 0), ("checker", 32, 32, ref.S420, 100, 0), ("fine", 16, 32, ref.S444, 100, 0),
         ("fine", 24, 24, ref.GREY, 100, 0), ("ramp", 48, 64, ref.S444, 20, 0), ("noise", 48, 64, ref.S444, 100, 0)]
ROW_RESTART = {("noise", 80, 24, ref.S444, 90, 3), ("ramp", 80, 24, ref.GREY, 50, 3)}        # (one MCU row = 3 MCUs, set by rows)

BATCH = [("ramp", 136, 200, ref.S420, 90, 0)] * 5                   # seeds 0..4


@functools.lru_cache(maxsize=None)
def all_cases():
    seen, out = set(), []
    for c in forward_cases() + EXTRA:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def case_image(case, seed=0):
    img = image(case[0], case[1], case[2], seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def goldens():
    """{name: Pillow's bytes}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "jpeg_enc_cases*.npz"))):
        with np.load(path) as z:
            for k in z.files:
                out[k] = z[k].tobytes()
    return out


def golden(case, seed=None):
    return goldens()[name_of(case) + ("" if seed is None else "_s%d" % seed)]


@functools.lru_cache(maxsize=None)
def ref_forward(case, seed=0):
    """the reference's coefficients of a case, int16 flat (read-only)"""
    q = ref.quant_tables(case[4])
    c = ref.forward(case_image(case, seed), q, case[3])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ref_encode(case, seed=0):
    """(the reference's bytes, its path statistics)"""
    stats = ref.new_stats()
    q = ref.quant_tables(case[4])
    return ref.entropy_encode(ref_forward(case, seed), q, case[1], case[2], case[3], case[5], stats), stats


def pillow_encode(bgr, quality, sampling, restart_interval=0, restart_rows=0):
    """what the goldens hold: libjpeg's default compressor through Pillow (grey: mode "L" of the reference's Y plane)"""
    import io

    from PIL import Image
    if sampling == ref.GREY:
        im = Image.fromarray(ref.ycc(np.asarray(bgr))[0].astype(np.uint8), "L")
        kw = {}
    else:
        im = Image.fromarray(np.ascontiguousarray(np.asarray(bgr)[:, :, ::-1]), "RGB")
        kw = dict(subsampling={ref.S444: 0, ref.S422: 1, ref.S420: 2}[sampling])
    if restart_rows:
        kw["restart_marker_rows"] = restart_rows
    elif restart_interval:
        kw["restart_marker_blocks"] = restart_interval
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()

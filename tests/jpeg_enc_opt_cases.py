"""The cases of the optimised-table tests.  Inputs are regenerated here from seeds or built directly; the committed fixture
(tests/golden/jpeg_enc_opt_cases.npz, written by tools/make_jpeg_enc_opt_fixtures.py) holds Pillow's bytes, optimize=True,
only.  References are computed once per process and shared (treat them as read-only).

A case is (content, h, w, sampling, quality, restart interval in MCUs), as in jpeg_enc_cases."""
import functools
import os

import numpy as np

from . import jpeg_enc_cases as base
from . import jpeg_enc_opt_ref as opt
from . import jpeg_enc_ref as ref

GOLDEN = os.path.join(base.GOLDEN, "jpeg_enc_opt_cases.npz")
CONTENTS = ("noise", "flat", "ramp", "checker")            # noise, flat, smooth, two-level
SHAPES = [(8, 8), (17, 23), (48, 64)]                      # one block; dummy edge blocks in every sampling; whole tiles
QUALITIES = (1, 50, 90, 100)
INTERVALS = (0, 2)

name_of = base.name_of


def image(content, h, w, seed=0):
    if content == "flat":
        return np.full((h, w, 3), (31 + 50 * seed, 200 - 60 * seed, 97 + 11 * seed), np.uint8)
    return base.image(content, h, w, seed)


@functools.lru_cache(maxsize=None)
def matrix():
    """every shape x sampling x quality x restart interval, the content rotating"""
    out, k = [], 0
    for h, w in SHAPES:
        for s in base.SAMPLINGS:
            for q in QUALITIES:
                for ri in INTERVALS:
                    out.append((CONTENTS[(k + k // 4 + k // 16) % len(CONTENTS)], h, w, s, q, ri))
                    k += 1
    return out


# one block, flat: a DC table of one symbol and an AC table of EOB alone; flat 16 x 16 in colour: four one-symbol tables;
# 17 x 23 of every content that the rotation above leaves out at quality 90
EXTRA = [("flat", 8, 8, ref.GREY, 90, 0), ("flat", 16, 16, ref.S420, 90, 0), ("flat", 16, 16, ref.S444, 50, 0), ("noise", 8, 8, ref.GREY, 90, 0)] + \
        [(c, 17, 23, s, 90, ri) for c in CONTENTS for s in base.SAMPLINGS for ri in INTERVALS]
# a film of three different pictures: three table sets, three header lengths
BATCH = [("noise", 40, 56, ref.S420, 90, 0), ("flat", 40, 56, ref.S420, 90, 0), ("ramp", 40, 56, ref.S420, 90, 0)]


@functools.lru_cache(maxsize=None)
def all_cases():
    seen, out = set(), []
    for c in matrix() + EXTRA + BATCH:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def case_image(case):
    img = image(case[0], case[1], case[2])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def goldens():
    with np.load(GOLDEN) as z:
        return {k: z[k].tobytes() for k in z.files}


def golden(case):
    return goldens()[name_of(case)]


@functools.lru_cache(maxsize=None)
def ref_forward(case):
    c = ref.forward(case_image(case), ref.quant_tables(case[4]), case[3])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ref_encode(case):
    return opt.entropy_encode(ref_forward(case), ref.quant_tables(case[4]), case[1], case[2], case[3], case[5])


def pillow_encode(bgr, quality, sampling, restart_interval=0):
    """libjpeg's optimize_coding through Pillow (grey: mode "L" of the reference's Y plane)"""
    import io

    from PIL import Image
    if sampling == ref.GREY:
        im = Image.fromarray(ref.ycc(np.asarray(bgr))[0].astype(np.uint8), "L")
        kw = {}
    else:
        im = Image.fromarray(np.ascontiguousarray(np.asarray(bgr)[:, :, ::-1]), "RGB")
        kw = dict(subsampling={ref.S444: 0, ref.S422: 1, ref.S420: 2}[sampling])
    if restart_interval:
        kw["restart_marker_blocks"] = restart_interval
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, optimize=True, **kw)
    return buf.getvalue()


# ---- coefficient arrays built directly (no picture gives them): (coef int16 flat, h, w, sampling, restart interval) ----
def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


@functools.lru_cache(maxsize=None)
def length_limited():
    """grey 280 x 280 (1225 blocks, every AC coefficient non-zero: no block has an EOB).  With the pseudo-symbol's 1 in front,
    the AC counts follow 1, 1, 2, 3, 5, 8 ... 17711 over 21 symbols: each merged sum stays below the next count but one, so the
    tree is one chain, jpeg_gen_optimal_table's code sizes reach 22 and the lengths are limited.  A 22nd symbol fills what
    is left (30198 coefficients; 160 x 160 has 25 200 in all, too few for the sequence).  DC differences of every size
    0 .. 11 with counts 1, 2, 3, 5 ... give the DC table a code of 12 bits, the longest it can have: 12 symbols and the
    pseudo-symbol are 13 leaves, so a DC code of 16 bits cannot arise."""
    h = w = 280
    nb = 35 * 35
    chain = fibonacci(22)[1:]                               # 1, 2, 3, 5 ... 17711
    # the rarest two: run 2, sizes 1 and 2; the next ten: run 1; the frequent nine: run 0, sizes 2 .. 10; the filler: 0x01
    syms = [(2, 1), (2, 2)] + [(1, s) for s in range(1, 11)] + [(0, s) for s in range(2, 11)]
    with_run = [rs for rs, c in zip(syms[:12], chain[:12]) for _ in range(c)]
    without = [rs for rs, c in zip(syms[12:], chain[12:]) for _ in range(c)]
    coef = np.zeros((nb, 64), np.int64)
    sign = 1
    for b in range(nb):
        k = 1
        while k <= 63:
            if with_run and k + with_run[-1][0] <= 63:
                run, size = with_run.pop()
            elif without:
                run, size = without.pop()
            else:
                run, size = 0, 1
            coef[b, ref.ZIGZAG[k + run]] = sign * (1 << (size - 1))
            sign, k = -sign, k + run + 1
    assert not with_run and not without
    sizes = [s for s, c in zip(range(11, -1, -1), fibonacci(13)[1:]) for _ in range(c)]
    sizes = sizes + [0] * (nb - len(sizes))
    dc = 0
    for i, s in enumerate(sizes):
        mag = (1 << (s - 1)) if s else 0
        dc += -mag if dc > 0 else mag
        coef[i, 0] = dc
    out = coef.reshape(-1).astype(np.int16)
    out.setflags(write=False)
    return out, h, w, ref.GREY, 0


@functools.lru_cache(maxsize=None)
def zrl_and_no_eob():
    """grey 8 x 24, three blocks: coefficient 63 alone (three ZRL in front, no EOB); coefficients 17 and 63 (ZRL, a run, no
    EOB); coefficient 40 alone (two ZRL, then EOB)"""
    coef = np.zeros((3, 64), np.int64)
    coef[0, 0], coef[0, ref.ZIGZAG[63]] = 5, -3
    coef[1, 0], coef[1, ref.ZIGZAG[17]], coef[1, ref.ZIGZAG[63]] = -200, 1, 1023
    coef[2, 0], coef[2, ref.ZIGZAG[40]] = 5, 7
    out = coef.reshape(-1).astype(np.int16)
    out.setflags(write=False)
    return out, 8, 24, ref.GREY, 0


def built():
    return {"length_limited": length_limited(), "zrl_and_no_eob": zrl_and_no_eob()}


@functools.lru_cache(maxsize=None)
def built_ref(name):
    coef, h, w, s, ri = built()[name]
    return opt.entropy_encode(coef, ref.quant_tables(90), h, w, s, ri)


# ---- symbol counts for the table tests ----
def table_inputs():
    fib = np.zeros(256, np.int64)
    for i, c in enumerate(fibonacci(25)[1:]):               # 1, 2, 3, 5 ...: with the pseudo-symbol's 1 in front, one chain
        fib[(i * 37 + 5) % 256] = c                         # scattered over the symbols; code sizes up to 24
    ties = np.zeros(256, np.int64)
    ties[[0, 1, 2, 3, 17, 33, 0xF0, 255]] = [4, 4, 2, 2, 1, 1, 1, 1]
    single = np.zeros(256, np.int64)
    single[7] = 1000
    single_one = np.zeros(256, np.int64)
    single_one[0] = 1                                       # equal to the pseudo-symbol's count
    equal = np.full(256, 3, np.int64)
    big = np.zeros(256, np.int64)
    big[:24] = [2 ** 31 >> i for i in range(24)]            # counts of 32 bits: their sums need 64
    return {"fibonacci": fib, "ties": ties, "single": single, "single_one": single_one, "equal": equal, "big": big}

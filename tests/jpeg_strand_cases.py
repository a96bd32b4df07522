"""Streams for the strand decoder's tests, made at test time with the library's own host coder (capi.jpeg_entropy_encode):
random coefficient sets with restart intervals of every kind.  Computed once per process and shared (read-only)."""
import functools

import numpy as np

from . import jpeg_ref

SAMPLINGS = (jpeg_ref.GREY, jpeg_ref.S444, jpeg_ref.S422, jpeg_ref.S420)
ROUND_TRIP_SHAPES = [(h, w, s) for h, w in ((17, 33), (48, 64)) for s in SAMPLINGS]


def mcu_grid(h, w, sampling):
    """(MCUs across, MCUs down)"""
    mw, mh = (16 if sampling >= jpeg_ref.S422 else 8), (16 if sampling == jpeg_ref.S420 else 8)
    return -(-w // mw), -(-h // mh)


@functools.lru_cache(maxsize=None)
def random_coefficients(h, w, sampling, seed=0):
    """(blocks * 64,) int16 the baseline tables can code: about a tenth of the blocks all zero, about a third dense with
    magnitudes up to +-1023 on many positions (long codes, and +1023 is ten 1-bits: many FF bytes), the rest sparse"""
    nb = jpeg_ref.n_blocks(h, w, sampling)
    rng = np.random.default_rng(7000 + 131 * h + 17 * w + sampling + 100003 * seed)
    coef = np.zeros((nb, 64), np.int64)
    kind = rng.random(nb)
    kind[:3] = (0.05, 0.2, 0.9)                                     # (every kind in every set, whatever the draw)
    for b in range(nb):
        if kind[b] < 0.1:
            continue
        coef[b, 0] = rng.integers(-500, 501)
        if kind[b] < 0.45:
            k = rng.integers(20, 64)
            pos = rng.choice(np.arange(1, 64), k, replace=False)
            coef[b, pos] = rng.integers(-1023, 1024, k)
            coef[b, pos[:k // 3]] = rng.choice((-1023, 1023), k // 3)
        else:
            k = rng.integers(0, 7)
            coef[b, rng.integers(1, 64, k)] = rng.integers(-40, 41, k)
    return coef.reshape(-1).astype(np.int16)


@functools.lru_cache(maxsize=None)
def coded(h, w, sampling, ri, seed=0):
    """the coefficients of random_coefficients as a baseline JPEG stream with a restart interval of ri MCUs (0: none)"""
    from camkifu_amd import capi
    return capi.jpeg_entropy_encode(random_coefficients(h, w, sampling, seed), capi.jpeg_quant(90), h, w, sampling, ri)


def restart_intervals(h, w, sampling):
    mcux, mcuy = mcu_grid(h, w, sampling)
    return sorted({1, 2, 3, mcux, mcux * mcuy, mcux * mcuy + 5})


def round_trips(h, w, sampling):
    """[(ri, stream, the coefficients it was coded from, the quant tables)]"""
    from camkifu_amd import capi
    seed = 20
    return [(ri, coded(h, w, sampling, ri, seed + k), random_coefficients(h, w, sampling, seed + k), capi.jpeg_quant(90))
            for k, ri in enumerate(restart_intervals(h, w, sampling))]


def mutations(old, at):
    """the values a damaged byte takes in the tests: one flipped bit, and FF (a marker or a stuffed byte appears)"""
    return [v for v in (old ^ (1 << (at & 7)), 0xFF) if v != old]


@functools.lru_cache(maxsize=None)
def _stuffed(_):
    from camkifu_amd import capi
    for seed in range(100, 1500):
        data = coded(48, 64, jpeg_ref.S420, 1, seed)
        rows = [tuple(int(v) for v in r) for r in capi.jpeg_plan([data])[0]]
        if any(data[r[2] - 2:r[2]] == b"\xff\x00" for r in rows[:-1]):
            return data, rows
    raise AssertionError("no strand ends in a stuffed byte")


def stream_with_stuffed_strand_end(capi):
    """(stream, its plan rows): a 48x64 stream with one MCU per strand in which some strand's last byte is a stuffed FF 00"""
    return _stuffed(0)


def swap_luma_chroma_tables(data):
    """the stream with the ids of its Huffman tables exchanged (0 <-> 1) inside the DHT segments: tables of other content for
    luma and chroma.  For the planner only: the entropy-coded data no longer fits them."""
    out = bytearray(data)
    segs, _ = jpeg_ref.segments(data)
    for m, o, ln in segs:
        if m != 0xC4:
            continue
        q = o
        while q < o + ln:
            out[q] ^= 1
            q += 17 + sum(data[q + 1:q + 17])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def cr_with_luma_dc_table(seed=0):
    """(stream, its coefficients, the same coefficients coded plainly): a 17 x 33 4:4:4 frame, restart interval 2, whose scan
    header names the LUMA DC table for Cr.  Every DC value of Cr is 0, and a DC difference of 0 is the code 00 in both DC
    tables of Annex K.3, so the data is valid under the tables the header names: the host decoder accepts the frame, with
    other tables for Cr than for Cb."""
    from camkifu_amd import capi
    h, w, sampling = 17, 33, jpeg_ref.S444
    coef = random_coefficients(h, w, sampling, 400 + seed).reshape(-1, 64).copy()
    nb = coef.shape[0] // 3
    coef[2 * nb:, 0] = 0
    coef = coef.reshape(-1)
    plain = capi.jpeg_entropy_encode(coef, capi.jpeg_quant(90), h, w, sampling, 2)
    segs, _ = jpeg_ref.segments(plain)
    sos = next(o for m, o, ln in segs if m == 0xDA)
    assert plain[sos + 6] == 0x11
    return plain[:sos + 6] + b"\x01" + plain[sos + 7:], coef, plain


def many_strands():
    """(streams, h, w, sampling): 5 frames of 8 x 536 4:4:4 with one MCU per strand -- 67 strands a frame, 335 in the call:
    more than one wave per frame, a partial last wave, more than 256 strands"""
    return [coded(8, 536, jpeg_ref.S444, 1, 50 + k) for k in range(5)], 8, 536, jpeg_ref.S444

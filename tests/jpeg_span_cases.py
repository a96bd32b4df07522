"""Streams for the span decoder's tests (csrc/ck_jpeg_span.h), on top of jpeg_cases, jpeg_strand_cases and jpeg_enc_ref: the
span sizes the tests run, streams searched for a stuffing 00 at a span's first byte, a noisy picture without restart
intervals, three table sets in one call.  Computed once per process and shared (read-only)."""
import functools

import numpy as np

from . import jpeg_cases, jpeg_enc_ref, jpeg_ref
from . import jpeg_strand_cases as sc

SMALL_SPANS = (8, 16, 64)


def decision(fn, streams, *args):
    """-> (coefficients, None) or (None, (code, bad frame, message))"""
    try:
        return fn(streams, *args)[1], None
    except Exception as e:                                           # noqa: BLE001  (CkError: code, frame and message are compared)
        return None, (e.code, e.bad_frame, str(e))


def strand_bytes(capi, data):
    """[(begin, end)] of the stream's strands"""
    return [(int(r[1]), int(r[2])) for r in capi.jpeg_plan([data])[0]]


@functools.lru_cache(maxsize=None)
def stuffing_at_span_start(span):
    """(stream, offset in its one strand): 48 x 64 4:2:0 without restart intervals in which a stuffing 00 is the FIRST byte of
    a span.  The scan is shifted bit by bit with the first block's leading AC coefficient until the offsets fall that way."""
    from camkifu_amd import capi
    base = sc.random_coefficients(48, 64, jpeg_ref.S420, seed=77)
    for lead in range(1, 1024):
        coef = base.copy()
        coef[1] = lead
        data = capi.jpeg_entropy_encode(coef, capi.jpeg_quant(90), 48, 64, jpeg_ref.S420, 0)
        (begin, end), = strand_bytes(capi, data)
        for off in range(span, end - begin, span):
            if data[begin + off] == 0 and data[begin + off - 1] == 0xFF:
                return data, coef, off
    raise AssertionError("no stream with a stuffing byte at a span's start")


@functools.lru_cache(maxsize=None)
def stuffed_strand_end_on_span_end(span):
    """(stream, strand index): one MCU per strand, and some strand that a marker follows ends in FF 00 with the 00 as the
    first byte of its last span (the FF is the last byte of the span before)"""
    from camkifu_amd import capi
    for seed in range(100, 3000):
        data = sc.coded(48, 64, jpeg_ref.S420, 1, seed)
        rows = strand_bytes(capi, data)
        for k, (b, e) in enumerate(rows[:-1]):
            if data[e - 2:e] == b"\xff\x00" and (e - 1 - b) % span == 0 and e - 1 - b > 0:
                return data, k
    raise AssertionError("no strand ends in a stuffed byte at a span's start")


@functools.lru_cache(maxsize=None)
def noisy_picture():
    """a noisy 48 x 64 4:2:0 picture at quality 90 without restart intervals, coded by the numpy reference coder"""
    rng = np.random.default_rng(4242)
    bgr = rng.integers(0, 256, (48, 64, 3)).astype(np.uint8)
    return jpeg_enc_ref.encode(bgr, 90, jpeg_ref.S420, 0)


@functools.lru_cache(maxsize=None)
def three_table_sets():
    """([streams], coefficients of each): a 17 x 33 4:4:4 call whose frames bring three different table sets: the plain
    Annex K.3 tables, Cr with the luma DC table, and plain again behind a frame without DHT segments (the same set)"""
    other, coef, plain = sc.cr_with_luma_dc_table()
    third, coef3, _ = sc.cr_with_luma_dc_table(1)
    # Cb as well under the luma DC table: every DC value of Cb is made 0, as cr_with_luma_dc_table does for Cr
    from camkifu_amd import capi
    c = coef3.reshape(-1, 64).copy()
    nb = c.shape[0] // 3
    c[nb:2 * nb, 0] = 0
    c = c.reshape(-1)
    both = capi.jpeg_entropy_encode(c, capi.jpeg_quant(90), 17, 33, jpeg_ref.S444, 2)
    segs, _ = jpeg_ref.segments(both)
    sos = next(o for m, o, ln in segs if m == 0xDA)
    assert both[sos + 4] == 0x11 and both[sos + 6] == 0x11
    both = both[:sos + 4] + b"\x01" + both[sos + 5:sos + 6] + b"\x01" + both[sos + 7:]
    return [plain, other, both, jpeg_cases.strip_dht(plain)], [coef, coef, c, coef]

"""The span decoder on the host, no GPU: the steps the "device-spans" kernels run (csrc/ck_jpeg_span.h behind
ck_jpeg_coefficients_spans: speculate, resolve, write, dc, verdict, the one-lane decoder for suspect frames) against the host
decoder (ck_jpeg_coefficients): every committed case, round trips at small span sizes, stuffing at span boundaries, several
table sets, the repair path, damaged streams with frame and message, and the binding."""
import numpy as np
import pytest

from . import jpeg_cases, jpeg_ref
from . import jpeg_span_cases as pc
from . import jpeg_strand_cases as sc
from .test_jpeg_sanitize_cpu import CASES


@pytest.fixture(scope="module")
def capi():
    from camkifu_amd import capi
    capi.build()
    return capi


def _same(capi, streams, span):
    info, coef, quant = capi.jpeg_coefficients(streams)
    sinfo, scoef, squant, stats = capi.jpeg_coefficients_spans(streams, span)
    assert sinfo == info
    assert np.array_equal(scoef, coef) and np.array_equal(squant, quant)
    return coef, stats


# ---- equality with the host decoder ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_every_committed_case_equals_the_host_decoder(capi, part):
    cases = jpeg_cases.file_cases()
    assert len(cases) == 298
    default = capi.jpeg_span_bytes()
    for name in jpeg_cases.names(4, part):
        data = cases[name][0]
        for span in (16, default):
            _, stats = _same(capi, [data], span)
            # a condition, not a measurement: a clean stream never needs the one-lane decoder
            assert stats["suspect_strands"] == 0 and stats["one_lane_frames"] == 0, (name, span, stats)
            assert stats["spans"] >= len(capi.jpeg_plan([data])[0]), (name, span)


@pytest.mark.parametrize("shape", sc.ROUND_TRIP_SHAPES, ids=lambda s: "%dx%d_s%d" % s)
def test_round_trips_decode_to_the_coefficients_they_were_coded_from(capi, shape):
    h, w, sampling = shape
    short, whole = 0, 0
    for ri, data, coef, quant in sc.round_trips(h, w, sampling):
        lens = [e - b for b, e in pc.strand_bytes(capi, data)]
        for span in pc.SMALL_SPANS:
            info, got, gq, stats = capi.jpeg_coefficients_spans([data], span)
            assert info["restart_interval"] == ri
            assert np.array_equal(got[0], coef), (shape, ri, span)
            assert np.array_equal(gq[0], capi.jpeg_coefficients([data])[2][0])
            assert stats["spans"] == sum(max(1, -(-n // span)) for n in lens)
            assert stats["suspect_strands"] == 0, (shape, ri, span, stats)
            short += sum(n < span for n in lens)
        whole += len(data)
    assert whole > 0
    if sampling == jpeg_ref.GREY:
        assert short > 0                                             # strands shorter than one span occur (one block an MCU)


def test_runs_of_stuffed_bytes_and_long_symbols_at_eight_byte_spans(capi):
    """the dense round-trip streams hold runs of FF 00 FF 00 FF 00 (+1023 behind a long code: one symbol with its stuffing
    bytes fills most of an 8-byte span, and where it starts in the span before it covers the whole of it, so that two spans
    enter at the same state and the one between owns no symbol).  A guard on the cases, then the decoder at S = 8."""
    seen = 0
    for seed in range(20, 60):
        d = sc.coded(48, 64, jpeg_ref.S420, 0, seed)
        (b, e), = pc.strand_bytes(capi, d)
        seen += sum(d[b + o:b + o + 6] == b"\xff\x00\xff\x00\xff\x00" for o in range(0, e - b - 6))
        _same(capi, [d], 8)
    assert seen > 0


@pytest.mark.parametrize("span", (8, 16))
def test_stuffing_at_a_span_boundary(capi, span):
    data, coef, off = pc.stuffing_at_span_start(span)
    (b, e), = pc.strand_bytes(capi, data)
    assert off % span == 0 and data[b + off] == 0 and data[b + off - 1] == 0xFF     # the offsets do fall that way
    got, stats = _same(capi, [data], span)
    assert np.array_equal(got[0], coef) and stats["suspect_strands"] == 0
    data, k = pc.stuffed_strand_end_on_span_end(span)
    b, e = pc.strand_bytes(capi, data)[k]
    assert data[e - 2:e] == b"\xff\x00" and (e - 1 - b) % span == 0 and data[e] == 0xFF and data[e + 1] == 0xD0 + k % 8
    _, stats = _same(capi, [data], span)
    assert stats["suspect_strands"] == 0
    # and the strand-end case of the strand tests, at every small span size
    data, _ = sc.stream_with_stuffed_strand_end(capi)
    for s in pc.SMALL_SPANS:
        assert _same(capi, [data], s)[1]["suspect_strands"] == 0


def test_other_tables_for_cr_and_three_table_sets_in_one_call(capi):
    other, coef, plain = sc.cr_with_luma_dc_table()
    for span in pc.SMALL_SPANS + (capi.jpeg_span_bytes(),):
        got, stats = _same(capi, [plain, other], span)
        assert np.array_equal(got[1], coef) and stats["suspect_strands"] == 0
    streams, coefs = pc.three_table_sets()
    assert capi.jpeg_plan(streams)[1] == 3
    for span in pc.SMALL_SPANS:
        got, stats = _same(capi, streams, span)
        assert all(np.array_equal(g, c) for g, c in zip(got, coefs)) and stats["suspect_strands"] == 0


def test_the_repair_path_decodes_spans_no_guess_met(capi):
    data = pc.noisy_picture()
    info = capi.jpeg_probe(data)
    assert (info["h"], info["w"], info["sampling"], info["restart_interval"]) == (48, 64, capi.CK_JPEG_420, 0)
    _, stats = _same(capi, [data], 8)
    assert stats["unresolved"] > 0 and stats["suspect_strands"] == 0, stats
    assert stats["unresolved"] < stats["spans"]                      # ... and most spans a guess did meet
    _, wide = _same(capi, [data], 64)
    assert wide["unresolved"] <= stats["unresolved"]


# ---- damage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_damaged_streams_get_the_host_decoders_decision_frame_and_message(capi, name):
    """the corpus of test_jpeg_strands_cpu: truncated at every offset, single-byte mutations at every offset of the scan.  The
    same accept / refuse decision as the host decoder, the same frame, the same message, the same coefficients when accepted;
    every refused variant whose headers are whole also inside a batch of five, with the same first bad frame.  The span size
    goes round 8, 16, 64 and the default with the variants."""
    data = jpeg_cases.file_cases()[name][0]
    scan = jpeg_ref.segments(data)[1]
    variants = [(data[:cut], cut >= scan) for cut in range(len(data))]
    for at in range(scan, len(data)):
        for v in sc.mutations(data[at], at):
            variants.append((data[:at] + bytes([v]) + data[at + 1:], True))
    spans = pc.SMALL_SPANS + (capi.jpeg_span_bytes(),)
    refused, batches, before = 0, 0, None
    for k, (bad, whole_headers) in enumerate(variants):
        span = spans[k % 4]
        want, werr = pc.decision(capi.jpeg_coefficients, [bad])
        got, gerr = pc.decision(capi.jpeg_coefficients_spans, [bad], span)
        assert werr == gerr, (name, k, span, werr, gerr)
        if werr is None:
            assert np.array_equal(want, got), (name, k, span)
            continue
        refused += 1
        if not whole_headers:
            continue
        at = 1 + batches % 4
        batch = [data] * 5
        batch[at] = bad
        if at < 4 and before is not None:
            batch[4] = before
        _, werr = pc.decision(capi.jpeg_coefficients, batch)
        _, gerr = pc.decision(capi.jpeg_coefficients_spans, batch, span)
        assert werr == gerr and werr[:2] == (capi.CK_ERR_DATA, at), (name, k, span, werr, gerr)
        batches, before = batches + 1, bad
    assert refused > len(data) // 2 and batches > 0


# ---- the ABI and the binding ---------------------------------------------------------------------------------------------------
def test_span_sizes_outside_8_to_4096_are_refused(capi):
    data = jpeg_cases.file_cases()[CASES[0]][0]
    assert 8 <= capi.jpeg_span_bytes() <= 4096
    for span in (8, 4096):
        _same(capi, [data], span)
    for span in (-1, 0, 7, 4097, 1 << 20):
        with pytest.raises(capi.CkError, match="span size") as e:
            capi.jpeg_coefficients_spans([data], span)
        assert e.value.code == capi.CK_ERR_ARG


def test_the_binding_knows_the_mode_by_name():
    """no library call: the constant, the names, and the old wording of the refusal (a context is not needed to refuse)"""
    import inspect
    from camkifu_amd import capi, pipeline
    assert capi.CK_JPEG_ENTROPY_DEVICE_SPANS == 2
    with open(capi.HEADER) as f:
        assert "CK_JPEG_ENTROPY_DEVICE_SPANS = 2" in f.read()
    calls = []

    class Lib:
        def ck_jpeg_set_entropy(self, h, mode):
            calls.append(("mode", mode))
            return 0

        def ck_jpeg_set_span_bytes(self, h, n):
            calls.append(("span", n))
            return 0

    ctx = object.__new__(capi.Context)
    ctx._h = None
    ctx._chk = lambda rc: None
    real = capi.lib
    capi.lib = lambda: Lib()
    try:
        for mode in ("host", "device", "device-spans"):
            ctx.jpeg_set_entropy(mode)
        ctx.jpeg_set_span_bytes(64)
        with pytest.raises(capi.CkError, match="'host' or 'device'"):
            ctx.jpeg_set_entropy("auto")
    finally:
        capi.lib = real
    assert calls == [("mode", 0), ("mode", 1), ("mode", 2), ("span", 64)]
    assert "device-spans" in inspect.getsource(pipeline)
    sigs = capi._SIGNATURES
    for fn in ("ck_jpeg_set_span_bytes", "ck_jpeg_span_bytes", "ck_jpeg_span_stats", "ck_jpeg_coefficients_spans"):
        assert fn in sigs

"""Parallel Huffman decoding inside a restart interval on the GPU (csrc/k_jpeg_span.hip behind ck_jpeg_coefficients_device and
ck_jpeg_decode in the "device-spans" entropy mode) against the host decoder, Pillow's committed decodes and the host's
staged run of the same steps (capi.jpeg_coefficients_spans), bit for bit, at small span sizes and at the default."""
import numpy as np
import pytest

from . import jpeg_cases, jpeg_ref
from . import jpeg_span_cases as pc
from . import jpeg_strand_cases as sc
from .test_jpeg_sanitize_cpu import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture()
def spans(ck):
    from camkifu_amd import capi
    ck.jpeg_set_entropy("device-spans")
    yield ck
    ck.jpeg_set_span_bytes(capi.jpeg_span_bytes())
    ck.jpeg_set_entropy("host")


def _groups():
    """the committed cases by geometry: [(names, streams)]"""
    from camkifu_amd import capi
    by = {}
    for name in jpeg_cases.names():
        info = capi.jpeg_probe(jpeg_cases.file_cases()[name][0])
        by.setdefault((info["h"], info["w"], info["sampling"]), []).append(name)
    return [(names, [jpeg_cases.file_cases()[n][0] for n in names]) for _, names in sorted(by.items())]


@pytest.mark.parametrize("part", range(4))
def test_every_case_through_the_span_kernels_equals_the_host_decoder(spans, part):
    """batched by geometry, at S = 16 and at the default; the default's result in HBM as well"""
    import torch
    from camkifu_amd import capi
    ck = spans
    groups = _groups()
    assert sum(len(g[0]) for g in groups) == 298
    for names, streams in groups[part::4]:
        info, coef, quant = capi.jpeg_coefficients(streams)
        for span in (16, capi.jpeg_span_bytes()):
            ck.jpeg_set_span_bytes(span)
            ginfo, gcoef, gquant = ck.jpeg_coefficients_device(streams)
            assert ginfo == info and np.array_equal(gcoef, coef) and np.array_equal(gquant, quant), (names, span)
            st = ck.jpeg_span_stats()
            assert st["suspect_strands"] == 0 and st["one_lane_frames"] == 0 and st["spans"] >= len(streams), (names, span, st)
        _, dcoef, dquant = ck.jpeg_coefficients_device(streams, to_device=torch.device("cuda:0"))
        assert np.array_equal(dcoef.cpu().numpy(), coef) and np.array_equal(dquant.cpu().numpy().view(np.uint16), quant), names


@pytest.mark.parametrize("part", range(4))
def test_decode_in_span_mode_gives_pillows_bytes(spans, part):
    import torch
    ck = spans
    cases = jpeg_cases.file_cases()
    dev = torch.device("cuda:0")
    for k, name in enumerate(jpeg_cases.names(4, part)):
        data, exp = cases[name]
        if k & 1:
            got = ck.jpeg_decode([data], to_device=dev).cpu().numpy()
        else:
            got = ck.jpeg_decode([data])
        assert got.shape == (1,) + exp.shape and np.array_equal(got[0], exp), name


@pytest.mark.parametrize("shape", sc.ROUND_TRIP_SHAPES, ids=lambda s: "%dx%d_s%d" % s)
def test_round_trips_through_the_span_kernels(spans, shape):
    """every restart interval of the CPU round trips, the streams of one shape in one call, at S = 8 and 64"""
    ck = spans
    h, w, sampling = shape
    trips = sc.round_trips(h, w, sampling)
    for span in (8, 64):
        ck.jpeg_set_span_bytes(span)
        _, coef, _ = ck.jpeg_coefficients_device([t[1] for t in trips])
        for k, (ri, _, want, _) in enumerate(trips):
            assert np.array_equal(coef[k], want), (shape, ri, span)
        assert ck.jpeg_span_stats()["suspect_strands"] == 0


def test_frames_with_no_restarts_and_with_many_in_one_call(spans):
    """8 x 536 4:4:4: five frames of 67 strands each (one MCU per strand, each shorter than a default span) and five without
    restart intervals (one strand of many spans) in ONE call, interleaved"""
    from camkifu_amd import capi
    ck = spans
    streams, h, w, sampling = sc.many_strands()
    whole = [sc.coded(h, w, sampling, 0, 50 + k) for k in range(5)]
    call = [s for pair in zip(streams, whole) for s in pair]
    rows, sets = capi.jpeg_plan(call)
    assert rows.shape[0] == 5 * 67 + 5 and sets == 1
    for span in (16, capi.jpeg_span_bytes()):
        ck.jpeg_set_span_bytes(span)
        _, coef, _ = ck.jpeg_coefficients_device(call)
        for k in range(10):
            assert np.array_equal(coef[k], sc.random_coefficients(h, w, sampling, 50 + k // 2)), (k, span)
        st = ck.jpeg_span_stats()
        assert st["suspect_strands"] == 0 and st["spans"] > rows.shape[0]


def test_the_devices_stats_equal_the_hosts_staged_run(spans):
    """spans, unresolved spans, suspect strands and one-lane frames of the kernels against the same steps on the host: this
    pins the speculation and the resolve decisions, not only the coefficients.  The noisy picture at S = 8 has unresolved
    spans; the three-table call reads tables from global memory; the damaged batch has a suspect strand and a one-lane frame."""
    from camkifu_amd import capi
    ck = spans
    noisy = pc.noisy_picture()
    three, _ = pc.three_table_sets()
    trips = [t[1] for t in sc.round_trips(48, 64, jpeg_ref.S420)]
    for streams, span in (([noisy], 8), ([noisy] * 3, 16), (three, 8), (three, 64), (trips, 8), (trips, 64), (trips, capi.jpeg_span_bytes())):
        ck.jpeg_set_span_bytes(span)
        _, coef, _, want = capi.jpeg_coefficients_spans(streams, span)
        _, got, _ = ck.jpeg_coefficients_device(streams)
        assert np.array_equal(got, coef)
        assert ck.jpeg_span_stats() == want, (span, ck.jpeg_span_stats(), want)
    ck.jpeg_set_span_bytes(8)
    ck.jpeg_coefficients_device([noisy])
    assert ck.jpeg_span_stats()["unresolved"] > 0
    # a frame the host still accepts though a strand of it is suspect: surplus bytes before a restart marker
    data = sc.coded(48, 64, jpeg_ref.S420, 3, seed=3)
    rows, _ = capi.jpeg_plan([data])
    at = int(rows[0][2])
    padded = data[:at] + b"\x00" + data[at:]
    want, werr = pc.decision(capi.jpeg_coefficients, [padded])
    for span in (8, 64):
        ck.jpeg_set_span_bytes(span)
        try:
            shost = capi.jpeg_coefficients_spans([data, padded, data], span)[3]
        except capi.CkError as e:
            shost = e.stats
        got, gerr = pc.decision(ck.jpeg_coefficients_device, [data, padded, data])
        assert (werr is None) == (gerr is None)
        if werr is None:
            assert np.array_equal(got[1], want[0])
        st = ck.jpeg_span_stats()
        assert st == shost and st["suspect_strands"] >= 1 and st["one_lane_frames"] == 1, (span, st, shost)


def test_a_damaged_frame_is_named_as_the_host_names_it_and_the_context_works_on(spans):
    from camkifu_amd import capi
    ck = spans
    data = jpeg_cases.file_cases()[CASES[0]][0]
    exp = jpeg_cases.file_cases()[CASES[0]][1]
    scan = jpeg_ref.segments(data)[1]
    bads = [data[:(scan + len(data)) // 2]]                          # cut inside the scan
    for at in range(scan, len(data)):                                # the first flipped bit the host decoder refuses
        bad = data[:at] + bytes([sc.mutations(data[at], at)[0]]) + data[at + 1:]
        if pc.decision(capi.jpeg_coefficients, [bad])[1] is not None:
            bads.append(bad)
            break
    assert len(bads) == 2
    for span in (8, capi.jpeg_span_bytes()):
        ck.jpeg_set_span_bytes(span)
        for bad in bads:
            batch = [data, data, bad, data, data]
            _, werr = pc.decision(capi.jpeg_coefficients, batch)
            _, gerr = pc.decision(ck.jpeg_coefficients_device, batch)
            assert werr == gerr and werr[:2] == (capi.CK_ERR_DATA, 2), (span, werr, gerr)
            with pytest.raises(capi.CkError) as e:
                ck.jpeg_decode(batch)
            assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 2 and str(e.value) == werr[2]
            good = ck.jpeg_decode([data] * 5)                        # the next call decodes clean
            assert all(np.array_equal(g, exp) for g in good)
    for mode in ("host", "device", "device-spans"):                  # and the other modes still work on this context
        ck.jpeg_set_entropy(mode)
        assert np.array_equal(ck.jpeg_decode([data])[0], exp), mode
    with pytest.raises(capi.CkError, match="'host' or 'device'"):
        ck.jpeg_set_entropy("auto")
    with pytest.raises(capi.CkError, match="span size"):
        ck.jpeg_set_span_bytes(7)
    with pytest.raises(capi.CkError, match="span size"):
        ck.jpeg_set_span_bytes(4097)


def test_several_passes(spans, monkeypatch):
    """CK_JPEG_PASS_BYTES at a few KB: two frames of the mean size per pass (three passes), then one frame per pass; the stats
    add up over the passes"""
    from camkifu_amd import capi
    ck = spans
    streams, exp = jpeg_cases.batch_case()
    ck.jpeg_set_span_bytes(64)
    assert np.array_equal(ck.jpeg_decode(streams), exp)
    one_pass = ck.jpeg_span_stats()
    up = ck.jpeg_uploaded_bytes()
    rows, _ = capi.jpeg_plan(streams)
    segments = sum(len(s) - int(r[1]) for s, r in zip(streams, rows))
    assert segments < up < segments + 5 * 48 + 8520 + 5 * 384 + 6 * 4 + 16 * 10      # compressed bytes, not coefficients
    monkeypatch.setenv("CK_JPEG_PASS_BYTES", str(2 * (sum(len(s) for s in streams) // 5 + 400) + 100))
    assert np.array_equal(ck.jpeg_decode(streams), exp)
    assert ck.jpeg_span_stats() == one_pass
    assert np.array_equal(ck.jpeg_coefficients_device(streams)[1], capi.jpeg_coefficients(streams)[1])
    with pytest.raises(capi.CkError, match=r"frame 4: ") as e:
        ck.jpeg_decode(streams[:4] + [streams[4][:len(streams[4]) // 2]])
    assert e.value.bad_frame == 4
    monkeypatch.setenv("CK_JPEG_PASS_BYTES", "1")
    assert np.array_equal(ck.jpeg_decode(streams), exp)
    assert ck.jpeg_span_stats() == one_pass


def test_a_film_of_two_batches_gives_the_records_of_host_mode(ck):
    from camkifu_amd import pipeline
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture as cap
    from camkifu_amd.stone.nn_manager import NNManager
    ck.cnn_set_weights(NNManager.init_net())
    runs = {}
    for mode in ("host", "device-spans"):
        c = cap.open_capture(jpeg_cases.AVI)
        ctrl = ControllerHeadless()
        ck.timing_enable(True)
        ck.timing_reset()
        try:
            with pipeline.FastFilePipeline(48, 64, ctrl, ctx=ck, bg_init_frames=2) as pipe:
                out = pipe.process_mjpeg(c, batch=2, file_fps=25, entropy=mode)
                runs[mode] = (repr(out), pipe.frames_done, ctrl.kifu.to_sgf())
            launches = ck.timing_get("jpeg_span_write")[1]
        finally:
            ck.timing_enable(False)
            ck.jpeg_set_entropy("host")
        assert (launches > 0) == (mode == "device-spans"), (mode, launches)      # the mode is the one that was asked for
    assert runs["host"][1] == 3 and runs["device-spans"] == runs["host"]

"""The Huffman stage of the JPEG decoder on the GPU (csrc/k_jpeg_huff.hip behind ck_jpeg_coefficients_device and, in the device
entropy mode, behind ck_jpeg_decode) against the host decoder and Pillow's committed decodes, bit for bit.

The kernel has two table paths: the table set of a workgroup's first strand is read from LDS, any other set from global
memory.  test_custom_tables_three_sets_in_one_call drives the GLOBAL path (three sets inside one workgroup); every other test
here drives the LDS path (one set per call)."""
import numpy as np
import pytest

from . import jpeg_cases, jpeg_ref
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
def device_mode(ck):
    ck.jpeg_set_entropy("device")
    yield ck
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
def test_every_case_through_the_device_equals_the_host_decoder(ck, part):
    """batched by geometry; the result in host memory, in HBM, and the first group once more after calls of other sizes"""
    import torch
    from camkifu_amd import capi
    groups = _groups()
    assert sum(len(g[0]) for g in groups) == 298
    mine = groups[part::4]
    dev = torch.device("cuda:0")
    want = []
    for names, streams in mine:
        info, coef, quant = capi.jpeg_coefficients(streams)
        want.append((coef, quant))
        ginfo, gcoef, gquant = ck.jpeg_coefficients_device(streams)
        assert ginfo == info and gcoef.dtype == np.int16 and gquant.dtype == np.uint16, names
        assert np.array_equal(gcoef, coef) and np.array_equal(gquant, quant), names
        _, dcoef, dquant = ck.jpeg_coefficients_device(streams, to_device=dev)
        assert dcoef.is_cuda and dquant.is_cuda
        assert np.array_equal(dcoef.cpu().numpy(), coef) and np.array_equal(dquant.cpu().numpy().view(np.uint16), quant), names
    _, gcoef, gquant = ck.jpeg_coefficients_device(mine[0][1])
    assert np.array_equal(gcoef, want[0][0]) and np.array_equal(gquant, want[0][1])


@pytest.mark.parametrize("part", range(4))
def test_decode_in_device_mode_gives_pillows_bytes(device_mode, part):
    import torch
    ck = device_mode
    cases = jpeg_cases.file_cases()
    dev = torch.device("cuda:0")
    for k, name in enumerate(jpeg_cases.names(4, part)):
        data, exp = cases[name]
        if k & 1:
            got = ck.jpeg_decode([data], to_device=dev).cpu().numpy()
        else:
            got = ck.jpeg_decode([data])
        assert got.shape == (1,) + exp.shape and np.array_equal(got[0], exp), name


def test_the_batch_of_five_in_device_mode_and_back_in_host_mode(ck, monkeypatch):
    import torch
    streams, exp = jpeg_cases.batch_case()
    ck.jpeg_set_entropy("device")
    try:
        assert np.array_equal(ck.jpeg_decode(streams), exp)
        dev = ck.jpeg_decode(streams, to_device=torch.device("cuda:0"))
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), exp)
        ck.timing_enable(True)
        ck.timing_reset()
        ck.jpeg_decode(streams)
        huff, recon = ck.timing_get("jpeg_huff"), ck.timing_get("jpeg")
        ck.timing_enable(False)
        assert huff[1] == 1 and huff[0] > 0 and recon[1] == 1
        # what went up: the entropy-coded segments, 5 plan rows, a table set and the quant tables -- not the coefficients
        from camkifu_amd import capi
        rows, sets = capi.jpeg_plan(streams)
        segments = sum(len(s) - int(r[1]) for s, r in zip(streams, rows))
        up = ck.jpeg_uploaded_bytes()
        assert segments + 5 * 48 + 8520 + 5 * 384 <= up <= segments + 5 * 48 + 8520 + 5 * 384 + 16 * 5 + 16 * 4
        ck.jpeg_set_entropy("host")
        ck.jpeg_decode(streams)
        assert ck.jpeg_uploaded_bytes() == 5 * (capi.jpeg_probe(streams[0])["blocks"] * 128 + 384)
        ck.jpeg_set_entropy("device")
        # large batches go through in passes, under the staging rule of the host mode applied to what this mode stages, the
        # compressed bytes: two frames of the mean size per pass (three passes), then one frame per pass
        from camkifu_amd import capi
        monkeypatch.setenv("CK_JPEG_PASS_BYTES", str(2 * (sum(len(s) for s in streams) // 5 + 400) + 100))
        assert np.array_equal(ck.jpeg_decode(streams), exp)
        assert np.array_equal(ck.jpeg_coefficients_device(streams)[1], capi.jpeg_coefficients(streams)[1])
        with pytest.raises(capi.CkError, match=r"frame 4: ") as e:
            ck.jpeg_decode(streams[:4] + [streams[4][:len(streams[4]) // 2]])
        assert e.value.bad_frame == 4
        monkeypatch.setenv("CK_JPEG_PASS_BYTES", "1")
        assert np.array_equal(ck.jpeg_decode(streams), exp)
        monkeypatch.delenv("CK_JPEG_PASS_BYTES")
    finally:
        ck.jpeg_set_entropy("host")
    assert np.array_equal(ck.jpeg_decode(streams), exp)              # the same context, back in host mode: the same bytes
    from camkifu_amd import capi
    with pytest.raises(capi.CkError, match="'host' or 'device'"):
        ck.jpeg_set_entropy("auto")


@pytest.mark.parametrize("shape", sc.ROUND_TRIP_SHAPES, ids=lambda s: "%dx%d_s%d" % s)
def test_round_trips_through_the_device(ck, shape):
    """every restart interval of the CPU round trips, the streams of one shape in one call"""
    h, w, sampling = shape
    trips = sc.round_trips(h, w, sampling)
    # (the restart interval is no part of the geometry: streams with different ones share a call)
    _, coef, _ = ck.jpeg_coefficients_device([t[1] for t in trips])
    for k, (ri, _, want, _) in enumerate(trips):
        assert np.array_equal(coef[k], want), (shape, ri)


def test_335_strands_in_one_call(ck):
    """67 strands a frame, 5 frames: more than one wave per frame, a partial last wave, more than 256 strands in the call"""
    from camkifu_amd import capi
    streams, h, w, sampling = sc.many_strands()
    rows, sets = capi.jpeg_plan(streams)
    assert rows.shape == (335, 6) and sets == 1 and [(rows[:, 0] == f).sum() for f in range(5)] == [67] * 5
    _, coef, _ = ck.jpeg_coefficients_device(streams)
    for k in range(5):
        assert np.array_equal(coef[k], sc.random_coefficients(h, w, sampling, 50 + k)), k
    assert np.array_equal(coef, capi.jpeg_coefficients(streams)[1])


def test_custom_tables_three_sets_in_one_call(ck):
    """the GLOBAL table path: two frames with Huffman tables optimised for each (tests/golden/jpeg_huff_cases.npz, written by
    tools/make_jpeg_huff_fixtures.py) and a frame without DHT in one call -- three table sets inside one workgroup, whose LDS
    holds the first"""
    import os
    from camkifu_amd import capi
    with np.load(os.path.join(jpeg_cases.GOLDEN, "jpeg_huff_cases.npz")) as z:
        streams = [z["j_0"].tobytes(), z["j_1"].tobytes()]
        exp = [z["e_0"], z["e_1"]]
    name = "ramp_48x64_420_q90_r3"
    streams.append(jpeg_cases.strip_dht(jpeg_cases.file_cases()[name][0]))
    exp.append(jpeg_cases.file_cases()[name][1])
    rows, sets = capi.jpeg_plan(streams)
    assert sets == 3 and sorted(set(rows[:, 5])) == [0, 1, 2] and len(rows) <= 64
    assert capi.jpeg_probe(streams[0])["restart_interval"] == 2
    info, coef, quant = capi.jpeg_coefficients(streams)
    _, gcoef, gquant = ck.jpeg_coefficients_device(streams)
    assert np.array_equal(gcoef, coef) and np.array_equal(gquant, quant)
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):                   # each set in the workgroup's LDS once, the others global
        ck.jpeg_set_entropy("device")
        try:
            got = ck.jpeg_decode([streams[k] for k in order])
        finally:
            ck.jpeg_set_entropy("host")
        for at, k in enumerate(order):
            assert np.array_equal(got[at], exp[k]), (order, k)


def test_a_frame_with_other_tables_for_cr_than_for_cb(ck):
    """accepted by the host decoder, so by the kernel: alone (its set in LDS) and behind a plain frame (its set global)"""
    from camkifu_amd import capi
    other, coef, plain = sc.cr_with_luma_dc_table()
    assert capi.jpeg_plan([plain, other])[1] == 2
    assert np.array_equal(ck.jpeg_coefficients_device([other])[1][0], coef)
    _, got, quant = ck.jpeg_coefficients_device([plain, other, plain])
    assert all(np.array_equal(g, coef) for g in got)
    assert np.array_equal(quant, capi.jpeg_coefficients([plain, other, plain])[2])


def _restart_batch():
    """the batch of five (136 x 200, 4:2:0, a quant table per frame) coded again by the library's coder with one MCU row per
    restart interval: 9 strands a frame"""
    from camkifu_amd import capi
    streams, exp = jpeg_cases.batch_case()
    info, coef, quant = capi.jpeg_coefficients(streams)
    mcux = sc.mcu_grid(info["h"], info["w"], info["sampling"])[0]
    again = [capi.jpeg_entropy_encode(coef[k], quant[k], info["h"], info["w"], info["sampling"], mcux) for k in range(5)]
    return again, exp, coef


CAUSE = r"ran past its end|unknown Huffman code|DC difference|DC value out of range|coefficient index above 63|restart marker RST\d missing"


def test_a_damaged_frame_is_named_and_the_context_works_on(ck):
    """error paths with bounded reads: frame 2 of the batch cut inside its third strand, and one scan byte of a frame changed at
    an offset the CPU corpus (test_jpeg_strands_cpu) contains"""
    from camkifu_amd import capi
    streams, exp, coef = _restart_batch()
    assert np.array_equal(ck.jpeg_coefficients_device(streams)[1], coef)
    rows, _ = capi.jpeg_plan(streams)
    third = rows[rows[:, 0] == 2][2]
    cut = streams[:2] + [streams[2][:int(third[1] + third[2]) // 2]] + streams[3:]
    with pytest.raises(capi.CkError) as host:
        capi.jpeg_coefficients(cut)
    assert host.value.bad_frame == 2
    with pytest.raises(capi.CkError, match=r"frame 2: .*(%s)" % CAUSE) as e:
        ck.jpeg_coefficients_device(cut)
    assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 2
    assert np.array_equal(ck.jpeg_coefficients_device(streams)[1], coef)             # the next call decodes clean
    ck.jpeg_set_entropy("device")
    try:
        with pytest.raises(capi.CkError, match=r"frame 2: .*(%s)" % CAUSE) as e:
            ck.jpeg_decode(cut)
        assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 2
        assert np.array_equal(ck.jpeg_decode(streams), exp)
        # one byte changed: the first offset of the scan at which the host decoder refuses the flipped bit
        data = jpeg_cases.file_cases()[CASES[0]][0]
        scan = jpeg_ref.segments(data)[1]
        for at in range(scan, len(data)):
            bad = data[:at] + bytes([sc.mutations(data[at], at)[0]]) + data[at + 1:]
            try:
                capi.jpeg_coefficients([bad])
            except capi.CkError:
                break
        else:
            raise AssertionError("no mutation is refused")
        batch = [data, data, bad, data, data]
        with pytest.raises(capi.CkError, match=r"frame 2: .*(%s)" % CAUSE) as e:
            ck.jpeg_decode(batch)
        assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 2
        with pytest.raises(capi.CkError, match=r"frame 2: ") as e:
            ck.jpeg_coefficients_device(batch)
        assert e.value.bad_frame == 2
        good = ck.jpeg_decode([data] * 5)
        assert all(np.array_equal(g, jpeg_cases.file_cases()[CASES[0]][1]) for g in good)
    finally:
        ck.jpeg_set_entropy("host")


def test_avi_capture_and_process_mjpeg_in_device_mode(ck):
    from camkifu_amd import pipeline
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture as cap
    from camkifu_amd.stone.nn_manager import NNManager
    _, frames = jpeg_cases.avi_reference()
    ck.jpeg_set_entropy("device")
    try:
        c = cap.AviMjpegCapture(jpeg_cases.AVI, decode=ck.jpeg_decode)
        got = []
        while True:
            ok, img = c.read()
            if not ok:
                break
            got.append(img)
        assert len(got) == 6 and c.damaged == 1
        for k in range(6):
            assert np.array_equal(got[k], frames[k]), k
    finally:
        ck.jpeg_set_entropy("host")
    ck.cnn_set_weights(NNManager.init_net())
    runs = {}
    for mode in ("host", "device"):
        c = cap.AviMjpegCapture(jpeg_cases.AVI, decode=ck.jpeg_decode)
        ctrl = ControllerHeadless()
        ck.timing_enable(True)
        ck.timing_reset()
        try:
            with pipeline.FastFilePipeline(48, 64, ctrl, ctx=ck, bg_init_frames=2) as pipe:
                out = pipe.process_mjpeg(c, batch=2, file_fps=25, entropy=mode)
                runs[mode] = (repr(out), pipe.frames_done, ctrl.kifu.to_sgf())
            launches = ck.timing_get("jpeg_huff")[1]
        finally:
            ck.timing_enable(False)
            ck.jpeg_set_entropy("host")
        assert (launches > 0) == (mode == "device"), (mode, launches)           # the mode is the one that was asked for
    assert runs["host"][1] == 3 and runs["device"] == runs["host"]

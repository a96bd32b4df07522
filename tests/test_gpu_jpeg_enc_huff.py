"""The Huffman stage of the JPEG encoder on the GPU (k_jpeg_enc_huff.hip): jpeg_entropy_encode_device and jpeg_encode in the
device mode against the host coder and the committed Pillow bytes, byte for byte; passes, refusals, argument errors, the
bytes that come down and the kernels' names in the timing table."""
import ctypes as C

import numpy as np
import pytest

from . import jpeg_enc_cases as cases
from . import jpeg_enc_ref as ref
from . import jpeg_enc_stage_cases as stage
from . import jpeg_ref
from .test_jpeg_enc_stages_cpu import refusal_batches

pytestmark = pytest.mark.gpu
KERNELS = ("jpeg_enc_size", "jpeg_enc_scan", "jpeg_enc_put", "jpeg_enc_stuff")


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture()
def dev(ck):
    """the context in the device mode for one test, in the host mode again behind it"""
    ck.jpeg_set_encode_entropy("device")
    yield ck
    ck.jpeg_set_encode_entropy("host")


def _hbm(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _up16(v):
    return (v + 15) // 16 * 16


@pytest.mark.parametrize("geometry", stage.GEOMETRIES, ids=["%dx%d_%s" % (h, w, stage.SNAME[s]) for h, w, s in stage.GEOMETRIES])
def test_synthetic_cases_equal_the_host_coder(ck, geometry):
    """every content and restart interval; coefficients from host memory and from HBM in turn"""
    from camkifu_amd import capi
    for k, case in enumerate(c for c in stage.all_cases() if c[1:4] == geometry):
        content, h, w, s, ri = case
        coef = stage.coef(case).reshape(1, -1)
        got = ck.jpeg_entropy_encode_device(_hbm(coef) if k & 1 else coef, stage.quant(), h, w, s, ri)
        assert got == capi.jpeg_entropy_encode(coef, stage.quant(), h, w, s, ri), stage.name_of(case)


def test_a_batch_of_five_different_frames_from_both_memories(ck):
    from camkifu_amd import capi
    cs, h, w, s, ri = stage.batch()
    coef = np.stack([stage.coef(c) for c in cs])
    want = capi.jpeg_entropy_encode(coef, stage.quant(), h, w, s, ri)
    assert ck.jpeg_entropy_encode_device(coef, stage.quant(), h, w, s, ri) == want
    assert ck.jpeg_entropy_encode_device(_hbm(coef), stage.quant(), h, w, s, ri) == want


def _groups():
    """the committed cases by (h, w, sampling, quality, restart interval): one call each"""
    out = {}
    for case in cases.all_cases():
        out.setdefault(case[1:], []).append(case)
    return list(out.items())


@pytest.mark.parametrize("part", range(4))
def test_committed_cases_equal_the_host_coder(ck, part):
    """the coefficients of every committed case, grouped by geometry; the first group once more after the others (the
    context's buffers have been other sizes since)"""
    from camkifu_amd import capi
    groups = _groups()[part::4]
    for k, ((h, w, s, q, ri), members) in enumerate(groups + groups[:1]):
        coef = np.stack([cases.ref_forward(c) for c in members])
        got = ck.jpeg_entropy_encode_device(_hbm(coef) if k & 1 else coef, ref.quant_tables(q), h, w, s, ri)
        assert got == capi.jpeg_entropy_encode(coef, ref.quant_tables(q), h, w, s, ri), members
        assert got == [cases.golden(c) for c in members], members


@pytest.mark.parametrize("part", range(4))
def test_encode_in_the_device_mode_gives_pillows_bytes_and_the_host_mode_still_does(ck, part):
    part_cases = cases.all_cases()[part::4]
    ck.jpeg_set_encode_entropy("device")
    try:
        for k, case in enumerate(part_cases):
            img = cases.case_image(case)
            out = ck.jpeg_encode(_hbm(img) if k & 1 else img, quality=case[4], sampling=case[3], restart_interval=case[5])
            assert out == [cases.golden(case)], cases.name_of(case)
    finally:
        ck.jpeg_set_encode_entropy("host")
    for case in part_cases:
        out = ck.jpeg_encode(cases.case_image(case), quality=case[4], sampling=case[3], restart_interval=case[5])
        assert out == [cases.golden(case)], cases.name_of(case)


def test_the_batch_of_five_in_one_pass_and_in_several(dev, monkeypatch):
    """5 frames of 136 x 200: one pass; then one frame per pass, as the host mode's test sets it.  What came down: the
    streams, each rounded up to 16 bytes, 8 bytes per frame and 16 per pass -- less than the coefficients of the host mode"""
    case = cases.BATCH[0]
    frames = np.stack([cases.case_image(case, seed) for seed in range(5)])
    want = [cases.golden(case, seed) for seed in range(5)]
    streams = sum(_up16(len(g)) for g in want)
    assert dev.jpeg_encode(frames, quality=case[4], sampling=case[3]) == want
    assert dev.jpeg_downloaded_bytes() == streams + 8 * 5 + 16
    monkeypatch.setenv("CK_JPEG_PASS_BYTES", "70000")
    assert dev.jpeg_encode(_hbm(frames), quality=case[4], sampling=case[3]) == want
    assert dev.jpeg_downloaded_bytes() == streams + 8 * 5 + 16 * 5
    coef = np.stack([cases.ref_forward(case, seed) for seed in range(5)])
    assert dev.jpeg_entropy_encode_device(coef, ref.quant_tables(case[4]), case[1], case[2], case[3]) == want
    assert dev.jpeg_downloaded_bytes() == streams + 8 * 5 + 16 * 5
    monkeypatch.delenv("CK_JPEG_PASS_BYTES")
    dev.jpeg_set_encode_entropy("host")
    assert dev.jpeg_encode(frames, quality=case[4], sampling=case[3]) == want
    assert dev.jpeg_downloaded_bytes() == coef.nbytes > streams + 8 * 5 + 16 * 5


def test_decode_of_encode_in_the_device_mode_equals_the_reference_decode(dev):
    for case in cases.all_cases()[3::11]:
        data = dev.jpeg_encode(cases.case_image(case), quality=case[4], sampling=case[3], restart_interval=case[5])
        assert np.array_equal(dev.jpeg_decode(data)[0], jpeg_ref.decode(cases.golden(case))), cases.name_of(case)


@pytest.mark.parametrize("ri", (0, 5))
def test_refusals_are_the_host_coders_and_the_context_goes_on(ck, ri):
    from camkifu_amd import capi
    h, w, s, batches = refusal_batches()
    for k, coef in enumerate(batches):
        with pytest.raises(capi.CkError) as host:
            capi.jpeg_entropy_encode(coef, stage.quant(), h, w, s, ri)
        with pytest.raises(capi.CkError) as got:
            ck.jpeg_entropy_encode_device(_hbm(coef) if k & 1 else coef, stage.quant(), h, w, s, ri)
        assert (got.value.code, str(got.value)) == (host.value.code, str(host.value))
    good = np.stack([stage.coef(("ff", h, w, s, ri))] * 2)
    assert ck.jpeg_entropy_encode_device(good, stage.quant(), h, w, s, ri) == [stage.ref_encode(("ff", h, w, s, ri))[0]] * 2


def test_argument_errors_name_the_cause(ck):
    import torch
    from camkifu_amd import capi
    with pytest.raises(capi.CkError, match="'host' or 'device'"):
        ck.jpeg_set_encode_entropy("gpu")
    L = capi.lib()
    assert L.ck_jpeg_set_encode_entropy(ck._h, 2) == capi.CK_ERR_ARG and b"entropy mode 2" in L.ck_last_error(ck._h)
    h, w, s = 17, 33, ref.S420
    case = ("ff", h, w, s, 0)
    q = stage.quant()
    bound = capi.jpeg_encode_bound(h, w, s)
    out, ln = np.zeros(bound, np.uint8), (C.c_size_t * 1)()
    pq, pout = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    flat = torch.zeros(stage.coef(case).size + 8, dtype=torch.int16, device="cuda:0")
    flat[1:-7] = _hbm(stage.coef(case))
    torch.cuda.synchronize()
    off = C.c_void_p(flat.data_ptr() + 2)
    assert L.ck_jpeg_entropy_encode_device(ck._h, off, capi.CK_DEVICE, pq, 1, h, w, s, 0, pout, bound, ln) == capi.CK_ERR_ARG
    assert b"16 bytes" in L.ck_last_error(ck._h)
    assert L.ck_jpeg_entropy_encode_device(ck._h, None, capi.CK_DEVICE, pq, 1, h, w, s, 0, pout, bound, ln) == capi.CK_ERR_ARG
    assert b"NULL" in L.ck_last_error(ck._h)
    host = np.array(stage.coef(case))
    ph = host.ctypes.data_as(C.c_void_p)
    assert L.ck_jpeg_entropy_encode_device(ck._h, ph, capi.CK_HOST, pq, 1, h, w, s, 0, pout, bound - 1, ln) == capi.CK_ERR_ARG
    assert b"smaller than the bound" in L.ck_last_error(ck._h) and not out.any()
    assert L.ck_jpeg_entropy_encode_device(ck._h, ph, 7, pq, 1, h, w, s, 0, pout, bound, ln) == capi.CK_ERR_ARG
    assert b"memory space" in L.ck_last_error(ck._h)
    assert L.ck_jpeg_downloaded_bytes(ck._h, None) == capi.CK_ERR_ARG
    bad = q.copy()
    bad[1, 3] = 0
    with pytest.raises(capi.CkError, match="frame 0: quant entry 67"):
        ck.jpeg_entropy_encode_device(host.reshape(1, -1), bad, h, w, s)
    with pytest.raises(capi.CkError, match="coef"):
        ck.jpeg_entropy_encode_device(host.reshape(1, -1)[:, :-64], q, h, w, s)
    assert ck.jpeg_entropy_encode_device(host.reshape(1, -1), q, h, w, s) == [stage.ref_encode(case)[0]]


def test_the_kernels_are_in_the_timing_table_in_the_device_mode_only(ck):
    img = cases.case_image(cases.BATCH[0])
    ck.timing_enable(True)
    try:
        ck.timing_reset()
        ck.jpeg_encode(img)
        assert ck.timing_get("jpeg_enc")[1] == 1 and all(ck.timing_get(k)[1] == 0 for k in KERNELS)
        ck.jpeg_set_encode_entropy("device")
        ck.timing_reset()
        ck.jpeg_encode(img)
        assert ck.timing_get("jpeg_enc")[1] == 1
        counts = {k: ck.timing_get(k)[1] for k in KERNELS}
        assert counts == {"jpeg_enc_size": 1, "jpeg_enc_scan": 1, "jpeg_enc_put": 1, "jpeg_enc_stuff": 2}
    finally:
        ck.jpeg_set_encode_entropy("host")
        ck.timing_enable(False)

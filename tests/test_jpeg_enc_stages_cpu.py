"""The stages of the GPU's JPEG entropy coder, run on the host (capi.jpeg_entropy_encode_staged: size, scan, put, stuff in plain
loops over the kernels' tiles), against the host coder, the numpy reference and the committed Pillow bytes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from . import jpeg_enc_cases as cases
from . import jpeg_enc_ref as ref
from . import jpeg_enc_stage_cases as stage


@pytest.fixture(scope="module")
def capi():
    from camkifu_amd import capi
    return capi


def test_the_cases_cross_the_tiles_and_their_seams(capi):
    tb, ty = capi.jpeg_enc_tiles()
    assert tb >= 1 and ty >= 4 and ty % 4 == 0
    stage.check_coverage()


@pytest.mark.parametrize("part", range(4))
def test_committed_cases_give_pillows_bytes(capi, part):
    for case in cases.all_cases()[part::4]:
        content, h, w, s, q, ri = case
        got = capi.jpeg_entropy_encode_staged(cases.ref_forward(case), ref.quant_tables(q), h, w, s, ri)
        assert got == cases.golden(case), cases.name_of(case)


def test_the_committed_batch_gives_pillows_bytes(capi):
    case = cases.BATCH[0]
    coef = np.stack([cases.ref_forward(case, seed) for seed in range(5)])
    got = capi.jpeg_entropy_encode_staged(coef, ref.quant_tables(case[4]), case[1], case[2], case[3], case[5])
    assert got == [cases.golden(case, seed) for seed in range(5)]


@pytest.mark.parametrize("geometry", stage.GEOMETRIES, ids=["%dx%d_%s" % (h, w, stage.SNAME[s]) for h, w, s in stage.GEOMETRIES])
def test_synthetic_cases_equal_the_host_coder_and_the_reference(capi, geometry):
    for case in [c for c in stage.all_cases() if c[1:4] == geometry]:
        content, h, w, s, ri = case
        got = capi.jpeg_entropy_encode_staged(stage.coef(case), stage.quant(), h, w, s, ri)
        assert got == capi.jpeg_entropy_encode(stage.coef(case), stage.quant(), h, w, s, ri), stage.name_of(case)
        assert got == stage.ref_encode(case)[0], stage.name_of(case)


def test_a_batch_of_five_different_frames(capi):
    cs, h, w, s, ri = stage.batch()
    coef = np.stack([stage.coef(c) for c in cs])
    got = capi.jpeg_entropy_encode_staged(coef, stage.quant(), h, w, s, ri)
    assert got == capi.jpeg_entropy_encode(coef, stage.quant(), h, w, s, ri)
    assert got == [stage.ref_encode(c)[0] for c in cs]


def _both(capi, coef, h, w, s, ri=0):
    """(code, message) of the host coder and of the staged one"""
    out = []
    for fn in (capi.jpeg_entropy_encode, capi.jpeg_entropy_encode_staged):
        with pytest.raises(capi.CkError) as e:
            fn(coef, stage.quant(), h, w, s, ri)
        out.append((e.value.code, str(e.value)))
    return out


def refusal_batches():
    """an AC of 1024 in frame 2 (MCU 7, and a later one) and another in frame 3; a DC pair of -32768 / 32767 in frame 1"""
    h, w, s = stage.H, stage.W, ref.S420
    base = np.stack([stage.coef(("ff", h, w, s, 0))] * 5).copy().reshape(5, -1, 64)
    ac = base.copy()
    ac[2, 40, 5] = 1024
    ac[2, 9, 63] = -1024
    ac[3, 0, 1] = 1024
    dc = base.copy()
    dc[1, 20, 0], dc[1, 21, 0] = -32768, 32767
    ac16 = base.copy()
    ac16[4, 100, 63] = -32768
    return h, w, s, [ac.reshape(5, -1), dc.reshape(5, -1), ac16.reshape(5, -1)]


@pytest.mark.parametrize("ri", (0, 5))
def test_refusals_are_the_host_coders(capi, ri):
    h, w, s, batches = refusal_batches()
    seen = []
    for coef in batches:
        host, staged = _both(capi, coef, h, w, s, ri)
        assert staged == host and host[0] == capi.CK_ERR_ARG
        seen.append(host[1])
    assert "frame 2: AC value of 11 bits" in seen[0] and "frame 1: DC difference" in seen[1] and "frame 4: AC value of 16 bits" in seen[2]


def test_a_small_buffer_is_refused_with_nothing_written(capi):
    case = ("ff", stage.H, stage.W, ref.S420, 0)
    coef = np.array(stage.coef(case))
    q = stage.quant()
    bound = capi.jpeg_encode_bound(stage.H, stage.W, ref.S420)
    out, ln = np.zeros(bound, np.uint8), (C.c_size_t * 1)(7)
    args = (coef.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), 1, stage.H, stage.W, ref.S420, 0, out.ctypes.data_as(C.c_void_p))
    assert capi.lib().ck_jpeg_entropy_encode_staged(*args, bound - 1, ln) == capi.CK_ERR_ARG
    assert b"smaller than the bound" in capi.lib().ck_last_error(None) and not out.any()
    assert capi.lib().ck_jpeg_entropy_encode_staged(*args, bound, ln) == 0
    assert out[:ln[0]].tobytes() == stage.ref_encode(case)[0]
    assert capi.lib().ck_jpeg_entropy_encode_staged(None, *args[1:], bound, ln) == capi.CK_ERR_ARG
    assert b"NULL" in capi.lib().ck_last_error(None)


def test_the_references_statistics_of_the_synthetic_cases():
    data, st = stage.ref_encode(("zeros", stage.H, stage.W, ref.S420, 0))
    assert len(data) - len(ref.headers(stage.quant(), stage.H, stage.W, ref.S420, 0)) == 98 and st["stuffed"] == 0 and st["eob"] == 144
    assert stage.ref_encode(("zeros", stage.H, stage.W, ref.S420, 1))[1]["restarts"] == 23
    data, st = stage.ref_encode(("ff", stage.H, stage.W, ref.S420, 0))
    assert (len(data), st["stuffed"], st["max_ac_size"]) == (3307, 888, 10)
    data, st = stage.ref_encode(("full", stage.H, stage.W, ref.GREY, 0))
    assert (len(data), st["stuffed"], st["no_eob"], st["eob"], st["max_dc_size"]) == (26226, 6000, 96, 0, 11)

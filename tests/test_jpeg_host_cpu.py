"""The host half of the JPEG decoder (csrc/ck_jpeg.cpp) through ctypes, no GPU: ck_jpeg_probe and ck_jpeg_coefficients against
the numpy reference on every committed case, the default Huffman tables, the refusals with their messages, truncation."""
import struct

import numpy as np
import pytest

from . import jpeg_cases, jpeg_ref


@pytest.fixture(scope="module")
def capi():
    from camkifu_amd import capi
    capi.build()
    return capi


@pytest.mark.parametrize("part", range(4))
def test_probe_and_coefficients_equal_the_reference(capi, part):
    cases = jpeg_cases.file_cases()
    for name in jpeg_cases.names(4, part):
        data = cases[name][0]
        rinfo, rcoef, rquant = jpeg_cases.ref_coefficients(name)
        assert capi.jpeg_probe(data) == rinfo, name
        info, coef, quant = capi.jpeg_coefficients([data])
        assert info == rinfo and coef.shape == (1, rinfo["blocks"] * 64), name
        assert np.array_equal(coef[0], rcoef), name
        assert np.array_equal(quant[0], rquant), name


def test_a_batch_decodes_in_one_call_with_a_quant_table_per_frame(capi):
    streams, _ = jpeg_cases.batch_case()
    info, coef, quant = capi.jpeg_coefficients(streams)
    assert (info["h"], info["w"], info["sampling"]) == (136, 200, capi.CK_JPEG_420)
    for k, data in enumerate(streams):
        _, rcoef, rquant = jpeg_ref.coefficients(data)
        assert np.array_equal(coef[k], rcoef) and np.array_equal(quant[k], rquant), k
    # a frame of another geometry inside the batch is named
    other = jpeg_cases.file_cases()["ramp_48x64_420_q90_r0"][0]
    with pytest.raises(capi.CkError, match=r"frame 2: 64x48 sampling 3 where the batch is 200x136") as e:
        capi.jpeg_coefficients(streams[:2] + [other] + streams[2:])
    assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 2


@pytest.mark.parametrize("name", ["noise_48x64_420_q90_r0", "ramp_47x61_422_q90_r3", "noise_17x33_444_q5_r0", "noise_50x35_grey_q90_r0"])
def test_a_frame_without_dht_gets_the_default_tables(capi, name):
    data = jpeg_cases.file_cases()[name][0]
    bare = jpeg_cases.strip_dht(data)
    assert len(bare) < len(data) - 100 and b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")]
    _, rcoef, rquant = jpeg_cases.ref_coefficients(name)
    info, coef, quant = capi.jpeg_coefficients([bare])
    assert np.array_equal(coef[0], rcoef) and np.array_equal(quant[0], rquant)
    assert np.array_equal(jpeg_ref.coefficients(bare)[1], rcoef)          # (and the reference agrees on the tables)


def _patch(data, marker, offset, value):
    """the stream with payload byte `offset` of its first `marker` segment replaced"""
    segs, _ = jpeg_ref.segments(data)
    o = next(o for m, o, ln in segs if m == marker)
    return data[:o + offset] + bytes([value]) + data[o + offset + 1:]


def _retag(data, marker, new):
    segs, _ = jpeg_ref.segments(data)
    o = next(o for m, o, ln in segs if m == marker)
    return data[:o - 3] + bytes([new]) + data[o - 2:]


def _insert_after_soi(data, seg):
    return data[:2] + seg + data[2:]


def _refused():
    base = jpeg_cases.file_cases()["ramp_48x64_420_q90_r0"][0]
    segs, scan_at = jpeg_ref.segments(base)
    sos = next(o for m, o, ln in segs if m == 0xDA)
    adobe = b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0)
    return {
        "progressive": (_retag(base, 0xC0, 0xC2), r"SOF2 .*only baseline SOF0"),
        "extended": (_retag(base, 0xC0, 0xC1), r"SOF1 .*only baseline SOF0"),
        "arithmetic": (_retag(base, 0xC0, 0xC9), r"SOF9 .*only baseline SOF0"),
        "twelve_bits": (_patch(base, 0xC0, 0, 12), r"sample precision 12"),
        "luma_4x1": (_patch(base, 0xC0, 7, 0x41), r"sampling 4x1 1x1 1x1: only luma"),
        "luma_1x2": (_patch(base, 0xC0, 7, 0x12), r"sampling 1x2 1x1 1x1: only luma"),
        "chroma_2x1": (_patch(base, 0xC0, 10, 0x21), r"sampling 2x2 2x1 1x1: only luma"),
        "adobe_rgb": (_insert_after_soi(base, adobe), r"Adobe APP14 transform 0"),
        "several_scans": (base[:sos - 2] + struct.pack(">HBBBBBB", 8, 1, 1, 0, 0, 63, 0) + base[scan_at:],
                          r"a scan of 1 of the 3 components: only one interleaved scan"),
        "no_soi": (b"\x00" + base[1:], r"no SOI"),
    }


@pytest.mark.parametrize("kind", sorted(_refused()))
def test_each_refused_kind_of_stream_is_ck_err_data_with_its_message(capi, kind):
    data, message = _refused()[kind]
    with pytest.raises(capi.CkError, match=message) as e:
        capi.jpeg_probe(data)
    assert e.value.code == capi.CK_ERR_DATA == 5
    with pytest.raises(capi.CkError) as e:
        capi.jpeg_coefficients([data])
    assert e.value.code == capi.CK_ERR_DATA


def test_adobe_transform_1_and_comments_are_skipped(capi):
    name = "ramp_48x64_420_q90_r0"
    base = jpeg_cases.file_cases()[name][0]
    adobe = b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 1)
    com = b"\xff\xfe" + struct.pack(">H", 7) + b"hello"
    _, coef, _ = capi.jpeg_coefficients([_insert_after_soi(base, adobe + com)])
    assert np.array_equal(coef[0], jpeg_cases.ref_coefficients(name)[1])


def test_damaged_entropy_data_is_named(capi):
    name = "noise_48x64_420_q90_r3"
    data = jpeg_cases.file_cases()[name][0]
    scan = data.index(b"\xff\xda")
    first = data.index(b"\xff\xd0", scan)
    # restart markers out of order
    swapped = data[:first + 1] + b"\xd1" + data[first + 2:]
    with pytest.raises(capi.CkError, match=r"frame 0: restart marker RST0 missing or out of order") as e:
        capi.jpeg_coefficients([swapped])
    assert e.value.code == capi.CK_ERR_DATA
    # a restart interval larger than the file says: the marker comes where data is expected
    with pytest.raises(capi.CkError, match=r"ran past its end|unknown Huffman code|coefficient index") as e:
        capi.jpeg_coefficients([_patch(data, 0xDD, 1, 200)])
    assert e.value.code == capi.CK_ERR_DATA


@pytest.mark.parametrize("name", ["noise_48x64_420_q90_r3", "ramp_47x61_422_q100_r0", "noise_17x33_grey_q5_r0"])
def test_truncation_at_every_97th_byte_is_data_error_or_ok(capi, name):
    data = jpeg_cases.file_cases()[name][0]
    seen = set()
    for cut in range(0, len(data), 97):
        try:
            capi.jpeg_coefficients([data[:cut]])
            seen.add(capi.CK_OK)
        except capi.CkError as e:
            assert e.code == capi.CK_ERR_DATA, (cut, e)
            seen.add(e.code)
    assert capi.CK_ERR_DATA in seen

"""The strand decoder on the host, no GPU: the planner (csrc/ck_jpeg_plan.cpp behind ck_jpeg_plan) on hand-built streams, and
the decoder the GPU kernel runs (csrc/ck_jpeg_strand.h behind ck_jpeg_coefficients_strands) against the host decoder
(ck_jpeg_coefficients) and the numpy reference: every committed case, round trips through the library's own coder,
damaged streams, and the strands of a call decoded in reverse order."""
import numpy as np
import pytest

from . import jpeg_cases, jpeg_ref
from . import jpeg_strand_cases as sc
from .test_jpeg_sanitize_cpu import CASES


@pytest.fixture(scope="module")
def capi():
    from camkifu_amd import capi
    capi.build()
    return capi


# ---- the planner -----------------------------------------------------------------------------------------------------------
def _rows(capi, streams):
    rows, sets = capi.jpeg_plan(streams)
    return [tuple(int(v) for v in r) for r in rows], sets


def _check_rows(data, rows, ri, total, frame=0):
    """rows of one frame against the stream's own markers: begin behind SOS or behind a marker, end on the next FF that no
    00 follows, MCUs counted in steps of ri"""
    scan = jpeg_ref.segments(data)[1]
    need = -(-total // ri) if ri else 1
    assert len(rows) == need
    for k, (f, b, e, first, n, _) in enumerate(rows):
        assert f == frame and first == k * (ri or total) and n == min(ri or total, total - first)
        assert b == scan if k == 0 else data[b - 2:b] == bytes([0xFF, 0xD0 + (k - 1) % 8])
        assert e == len(data) or (data[e] == 0xFF and data[e + 1:e + 2] != b"\x00")
        assert b"\xff" not in data[b:e].replace(b"\xff\x00", b"")


@pytest.mark.parametrize("ri", ["1", "3", "row", "all", "more"])
def test_strand_rows_for_each_restart_interval(capi, ri):
    h, w, sampling = 48, 64, capi.CK_JPEG_420                      # 4 x 3 MCUs
    total, mcux = 12, 4
    n = {"1": 1, "3": 3, "row": mcux, "all": total, "more": total + 5}[ri]
    data = sc.coded(h, w, sampling, n, seed=1)
    rows, sets = _rows(capi, [data])
    _check_rows(data, rows, n if n < total else 0, total)
    assert sets == 1
    assert len(rows) == {"1": 12, "3": 4, "row": 3, "all": 1, "more": 1}[ri]


def test_more_than_eight_strands_wrap_the_marker_number(capi):
    data = sc.coded(48, 64, capi.CK_JPEG_420, 1, seed=2)
    rows, _ = _rows(capi, [data])
    assert len(rows) == 12
    _check_rows(data, rows, 1, 12)
    assert data[rows[9][1] - 2:rows[9][1]] == b"\xff\xd0"           # the ninth marker is RST0 again


def test_fill_bytes_before_a_marker_and_a_stuffed_byte_at_a_strands_end(capi):
    data = sc.coded(48, 64, capi.CK_JPEG_420, 3, seed=3)
    rows, _ = _rows(capi, [data])
    at = rows[1][1] - 2                                               # the first marker
    filled = data[:at] + b"\xff\xff\xff" + data[at:]
    rows2, _ = _rows(capi, [filled])
    assert rows2[0] == rows[0] and rows2[1][1:3] == (rows[1][1] + 3, rows[1][2] + 3)
    _, coef, _ = capi.jpeg_coefficients_strands([filled])
    assert np.array_equal(coef, capi.jpeg_coefficients([data])[1]) and np.array_equal(coef, capi.jpeg_coefficients([filled])[1])
    # a strand whose last data byte is a stuffed FF 00: found among the coded streams, not constructed
    data, rows = sc.stream_with_stuffed_strand_end(capi)
    k = next(k for k, r in enumerate(rows[:-1]) if data[r[2] - 2:r[2]] == b"\xff\x00")
    assert data[rows[k][2]] == 0xFF and data[rows[k][2] + 1] == 0xD0 + k % 8
    assert np.array_equal(capi.jpeg_coefficients_strands([data])[1], capi.jpeg_coefficients([data])[1])


def test_markers_out_of_order_missing_and_surplus(capi):
    data = sc.coded(48, 64, capi.CK_JPEG_420, 3, seed=4)
    rows, _ = _rows(capi, [data])
    second = rows[2][1] - 2
    swapped = data[:second + 1] + b"\xd0" + data[second + 2:]         # RST0 where RST1 is due
    with pytest.raises(capi.CkError, match=r"frame 0: restart marker RST1 missing or out of order before MCU 6") as e:
        capi.jpeg_plan([swapped])
    assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 0
    missing = data[:second] + data[second + 2:]                       # the marker cut out: too few strands before EOI
    with pytest.raises(capi.CkError, match=r"restart marker RST\d missing or out of order before MCU") as e:
        capi.jpeg_plan([missing])
    for bad in (swapped, missing):
        with pytest.raises(capi.CkError) as e1:
            capi.jpeg_coefficients([bad])
        with pytest.raises(capi.CkError) as e2:
            capi.jpeg_coefficients_strands([bad])
        assert e1.value.code == e2.value.code == capi.CK_ERR_DATA
    # surplus data behind the last MCU is not looked at: another marker and more entropy-coded bytes before EOI
    surplus = data[:-2] + b"\xff\xd3" + data[rows[1][1]:rows[1][2]] + b"\xff\xd9"
    rows3, _ = _rows(capi, [surplus])
    assert rows3 == rows
    assert np.array_equal(capi.jpeg_coefficients_strands([surplus])[1], capi.jpeg_coefficients([data])[1])
    assert np.array_equal(capi.jpeg_coefficients([surplus])[1], capi.jpeg_coefficients([data])[1])


def test_table_sets_are_shared_by_content(capi):
    data = jpeg_cases.file_cases()["noise_48x64_420_q90_r3"][0]
    other = jpeg_cases.file_cases()["ramp_48x64_420_q5_r3"][0]
    assert _rows(capi, [data, other, data])[1] == 1                   # equal DHT (Annex K.3 written out)
    bare = jpeg_cases.strip_dht(data)
    assert _rows(capi, [bare, bare])[1] == 1                          # without DHT
    assert _rows(capi, [bare, data])[1] == 1                          # ... which are the same tables again
    swapped = sc.swap_luma_chroma_tables(data)                        # another DHT: luma and chroma tables exchanged
    rows, sets = _rows(capi, [data, swapped, data])
    assert sets == 2 and [r[5] for r in rows if r[3] == 0] == [0, 1, 0]


def test_a_capacity_one_too_small_says_how_many_rows_there_are(capi):
    import ctypes as C
    data = sc.coded(48, 64, capi.CK_JPEG_420, 3, seed=5)
    ptrs, lens, keep = capi._jpeg_streams([data])
    info = capi.jpeg_probe(data)
    geom = capi.JpegInfo(info["h"], info["w"], info["sampling"], info["restart_interval"], info["blocks"])
    rows = np.full((3, 6), -1, np.int64)
    count, sets, bad = C.c_longlong(0), C.c_int32(0), C.c_int32(-1)
    rc = capi.lib().ck_jpeg_plan(ptrs, lens, 1, C.byref(geom), rows.ctypes.data_as(C.c_void_p), 3, C.byref(count), C.byref(sets), C.byref(bad))
    assert rc == capi.CK_ERR_CAPACITY and count.value == 4 and (rows == -1).all()
    rows = np.full((4, 6), -1, np.int64)
    rc = capi.lib().ck_jpeg_plan(ptrs, lens, 1, C.byref(geom), rows.ctypes.data_as(C.c_void_p), 4, C.byref(count), C.byref(sets), C.byref(bad))
    assert rc == 0 and count.value == 4 and sets.value == 1 and (rows[:, 4] == 3).all()


# ---- equality with the host decoder ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_every_committed_case_equals_the_host_decoder_and_the_reference(capi, part):
    cases = jpeg_cases.file_cases()
    assert len(cases) == 298
    for name in jpeg_cases.names(4, part):
        data = cases[name][0]
        rinfo, rcoef, rquant = jpeg_cases.ref_coefficients(name)
        info, coef, quant = capi.jpeg_coefficients([data])
        sinfo, scoef, squant = capi.jpeg_coefficients_strands([data])
        assert sinfo == info == rinfo, name
        assert np.array_equal(scoef, coef) and np.array_equal(scoef[0], rcoef), name
        assert np.array_equal(squant, quant) and np.array_equal(squant[0], rquant), name


# ---- round trips through the library's own coder ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.ROUND_TRIP_SHAPES, ids=lambda s: "%dx%d_s%d" % s)
def test_round_trips_decode_to_the_coefficients_they_were_coded_from(capi, shape):
    h, w, sampling = shape
    for ri, data, coef, quant in sc.round_trips(h, w, sampling):
        info, got, gq = capi.jpeg_coefficients_strands([data])
        assert info["restart_interval"] == ri
        assert np.array_equal(got[0], coef), (shape, ri)
        assert np.array_equal(gq[0][:1 if sampling == capi.CK_JPEG_GREY else 3], quant[:1 if sampling == capi.CK_JPEG_GREY else 3])
        assert np.array_equal(capi.jpeg_coefficients([data])[1][0], coef), (shape, ri)


def test_the_round_trip_sets_hold_what_they_are_meant_to(capi):
    """a guard on the generator, not on the decoder: it passes without the strand decoder"""
    coef = sc.random_coefficients(48, 64, capi.CK_JPEG_420, seed=0).reshape(-1, 64)
    assert (np.abs(coef[:, 1:]) == 1023).sum() > 50 and (coef == 0).all(axis=1).sum() >= 2
    data = sc.coded(48, 64, capi.CK_JPEG_420, 2, seed=0)
    assert data.count(b"\xff\x00") > 10                              # many stuffed bytes


# ---- damage --------------------------------------------------------------------------------------------------------------------
def _decision(fn, streams):
    try:
        return fn(streams)[1], None
    except Exception as e:                                           # noqa: BLE001  (CkError: its code and frame are compared)
        return None, (e.code, e.bad_frame)


@pytest.mark.parametrize("name", CASES)
def test_damaged_streams_get_the_host_decoders_decision(capi, name):
    """truncated at every offset and with single-byte mutations at every offset of the scan: the same accept / refuse
    decision as the host decoder, the same coefficients when accepted; and EVERY refused variant whose headers are whole also
    inside a batch of five -- at place 1 .. 4 in turn, the refused variant before it at place 4 behind it, so that a frame
    the planner refuses meets an earlier frame that fails in the decoder and the other way round: the same first bad frame"""
    data = jpeg_cases.file_cases()[name][0]
    scan = jpeg_ref.segments(data)[1]
    variants = [(data[:cut], cut >= scan) for cut in range(len(data))]        # (the stream, are its headers whole?)
    for at in range(scan, len(data)):
        for v in sc.mutations(data[at], at):
            variants.append((data[:at] + bytes([v]) + data[at + 1:], True))
    refused, batches, before = 0, 0, None
    for k, (bad, whole_headers) in enumerate(variants):
        want, werr = _decision(capi.jpeg_coefficients, [bad])
        got, gerr = _decision(capi.jpeg_coefficients_strands, [bad])
        assert (werr is None) == (gerr is None), (name, k, werr, gerr)
        if werr is None:
            assert np.array_equal(want, got), (name, k)
            continue
        assert werr == gerr, (name, k, werr, gerr)
        refused += 1
        if not whole_headers:
            continue
        at = 1 + batches % 4
        batch = [data] * 5
        batch[at] = bad
        if at < 4 and before is not None:
            batch[4] = before
        _, werr = _decision(capi.jpeg_coefficients, batch)
        _, gerr = _decision(capi.jpeg_coefficients_strands, batch)
        assert werr == gerr == (capi.CK_ERR_DATA, at), (name, k, werr, gerr)
        batches, before = batches + 1, bad
    assert refused > len(data) // 2 and batches > 0


def test_a_frame_with_other_tables_for_cr_than_for_cb_decodes_as_on_the_host(capi):
    """the host decoder accepts a frame whose Cr names other tables than its Cb, so the strand decoder does: a table set has a
    pair per component.  One such frame that is valid (jpeg_strand_cases.cr_with_luma_dc_table), and forty that are not (Cr
    takes both luma tables, which the data was not coded for): the decisions and the coefficients agree on all."""
    other, coef, plain = sc.cr_with_luma_dc_table()
    for fn in (capi.jpeg_coefficients, capi.jpeg_coefficients_strands):
        assert np.array_equal(fn([other])[1][0], coef) and np.array_equal(fn([plain, other])[1][1], coef)
    rows, sets = capi.jpeg_plan([plain, other, plain])
    assert sets == 2 and [int(r[5]) for r in rows if r[3] == 0] == [0, 1, 0]
    for seed in range(40):
        data = sc.coded(17, 33, capi.CK_JPEG_444, 2, 300 + seed)
        segs, _ = jpeg_ref.segments(data)
        sos = next(o for m, o, ln in segs if m == 0xDA)
        bad = data[:sos + 6] + b"\x00" + data[sos + 7:]
        want, werr = _decision(capi.jpeg_coefficients, [bad])
        got, gerr = _decision(capi.jpeg_coefficients_strands, [bad])
        assert werr == gerr and (werr is not None or np.array_equal(want, got)), (seed, werr, gerr)


# ---- independence --------------------------------------------------------------------------------------------------------------
def test_the_strands_of_a_call_in_reverse_order_give_the_same_bytes(capi, tmp_path):
    """ck_jpeg_strands_host takes the order as an argument; tools/sanitize/jpeg_strand_fuzz.cpp --call (built plain here, under
    the sanitizers in test_jpeg_strands_sanitize_cpu) decodes four streams with 12, 6, 4 and 3 strands as ONE call, first
    strand first and last strand first, whole and with each frame in turn cut: the same bytes, the host decoder's, and the
    same first bad frame"""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "camkifu_amd", "csrc")
    exe = str(tmp_path / "jpeg_strand_call")
    res = subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(root, "include"),
                          os.path.join(root, "tools", "sanitize", "jpeg_strand_fuzz.cpp"), os.path.join(csrc, "ck_jpeg.cpp"),
                          os.path.join(csrc, "ck_jpeg_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    files = []
    for ri in (1, 2, 3, 4):
        files.append(str(tmp_path / ("ri%d.jpg" % ri)))
        with open(files[-1], "wb") as f:
            f.write(sc.coded(48, 64, capi.CK_JPEG_420, ri, seed=10 + ri))
    run = subprocess.run([exe, "--call"] + files, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "one call of 4 frames" in run.stdout and "both strand orders give the host decoder's bytes" in run.stdout
    # and through the library: the call as a whole, and the frame that is cut is the one named
    streams = [open(f, "rb").read() for f in files]
    assert np.array_equal(capi.jpeg_coefficients_strands(streams)[1], capi.jpeg_coefficients(streams)[1])
    with pytest.raises(capi.CkError, match="frame 2: ") as e:
        capi.jpeg_coefficients_strands(streams[:2] + [streams[2][:len(streams[2]) - 40]] + streams[3:])
    assert e.value.bad_frame == 2

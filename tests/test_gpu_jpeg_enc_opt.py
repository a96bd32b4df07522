"""Optimised Huffman tables on the GPU (jpeg_enc_histo and jpeg_enc_tables in k_jpeg_enc_huff.hip, and size, put and stuff
with a frame's own tables and header): jpeg_entropy_encode_device(optimize=True) and jpeg_encode(optimize=True) against the
host coder and the committed Pillow bytes, byte for byte; the kernels' counters and tables against ck_jpeg_histogram and
ck_jpeg_optimal_table; what comes down; the standard mode untouched; the film decoded again in every entropy mode."""
import numpy as np
import pytest

from . import jpeg_enc_cases as base
from . import jpeg_enc_opt_cases as cases
from . import jpeg_enc_ref as ref
from . import jpeg_ref

pytestmark = pytest.mark.gpu
KERNELS = ("jpeg_enc_histo", "jpeg_enc_tables", "jpeg_enc_size", "jpeg_enc_scan", "jpeg_enc_put", "jpeg_enc_stuff")


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
    ck.jpeg_set_encode_tables("standard")


def _hbm(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def _up16(v):
    return (v + 15) // 16 * 16


def _dht_tables(stream):
    """[(bits, vals)] of the stream's DHT segments, in their order"""
    out = []
    for marker, at, n in jpeg_ref.segments(stream)[0]:
        if marker == 0xC4:
            body = bytes(stream[at:at + n])
            assert body[0] == [0x00, 0x10, 0x01, 0x11][len(out)] and len(body) == 17 + sum(body[1:17])
            out.append((list(body[1:17]), list(body[17:])))
    return out


@pytest.mark.parametrize("part", range(4))
def test_committed_cases_equal_the_host_coder_and_pillow(ck, part):
    """every case, one call each, coefficients from host memory and from HBM in turn; the first once more at the end (the
    context's buffers have been other sizes since)"""
    from camkifu_amd import capi
    mine = cases.all_cases()[part::4]
    for k, c in enumerate(mine + mine[:1]):
        coef, q = cases.ref_forward(c).reshape(1, -1), ref.quant_tables(c[4])
        got = ck.jpeg_entropy_encode_device(_hbm(coef) if k & 1 else coef, q, c[1], c[2], c[3], c[5], optimize=True)
        want = capi.jpeg_entropy_encode(coef, q, c[1], c[2], c[3], c[5], optimize=True)
        assert [len(g) for g in got] == [len(g) for g in want] and got == want == [cases.golden(c)], cases.name_of(c)


@pytest.mark.parametrize("name", sorted(cases.built()))
def test_built_coefficients_zrl_no_eob_and_limited_lengths(ck, name):
    from camkifu_amd import capi
    coef, h, w, s, ri = cases.built()[name]
    q = ref.quant_tables(90)
    want = capi.jpeg_entropy_encode(coef, q, h, w, s, ri, optimize=True)
    assert want == cases.built_ref(name)
    two = np.stack([coef, np.zeros_like(coef)])                            # (the second frame: one-symbol tables)
    assert ck.jpeg_entropy_encode_device(two, q, h, w, s, ri, optimize=True) == capi.jpeg_entropy_encode(two, q, h, w, s, ri, optimize=True)
    assert ck.jpeg_entropy_encode_device(_hbm(coef.reshape(1, -1)), q, h, w, s, ri, optimize=True) == [want]
    assert np.array_equal(ck.jpeg_encode_histograms(1)[0], capi.jpeg_histogram(coef, h, w, s, ri))


def test_a_batch_of_three_pictures_counters_tables_lengths_and_what_comes_down(dev, monkeypatch):
    from camkifu_amd import capi
    c0 = cases.BATCH[0]
    h, w, s, quality = c0[1], c0[2], c0[3], c0[4]
    frames = np.stack([cases.case_image(c) for c in cases.BATCH])
    coef = np.stack([cases.ref_forward(c) for c in cases.BATCH])
    want = [cases.golden(c) for c in cases.BATCH]
    streams = sum(_up16(len(g)) for g in want)
    assert dev.jpeg_encode(frames, quality=quality, sampling=s, optimize=True) == want
    assert dev.jpeg_downloaded_bytes() == streams + 8 * 3 + 16
    # the kernels' counters and the tables in the streams are the host's
    counts = dev.jpeg_encode_histograms(3)
    assert np.array_equal(counts, capi.jpeg_histogram(coef, h, w, s))
    for f in range(3):
        tables = _dht_tables(want[f])
        assert len(tables) == 4
        for t, (bits, vals) in enumerate(tables):
            hb, hv = capi.jpeg_optimal_table(counts[f, t])
            assert (bits, vals) == (list(hb), list(hv)), (f, t)
    assert len({g.index(b"\xff\xda") for g in want}) == 3                  # three header lengths
    # the same from coefficients, in host memory and in HBM; then a frame per pass: 16 bytes more each
    assert dev.jpeg_entropy_encode_device(coef, ref.quant_tables(quality), h, w, s, optimize=True) == want
    assert dev.jpeg_downloaded_bytes() == streams + 8 * 3 + 16
    monkeypatch.setenv("CK_JPEG_PASS_BYTES", "10000")                      # (a frame has 9216 bytes of coefficients)
    assert dev.jpeg_entropy_encode_device(_hbm(coef), ref.quant_tables(quality), h, w, s, optimize=True) == want
    assert dev.jpeg_downloaded_bytes() == streams + 8 * 3 + 16 * 3
    assert np.array_equal(dev.jpeg_encode_histograms(1)[0], counts[2])     # the hook reads the last pass
    dev.jpeg_set_encode_tables("optimised")
    assert dev.jpeg_encode(_hbm(frames), quality=quality, sampling=s) == want
    assert dev.jpeg_downloaded_bytes() == streams + 8 * 3 + 16 * 3
    monkeypatch.delenv("CK_JPEG_PASS_BYTES")
    # the host mode: the same bytes; the coefficients come down
    dev.jpeg_set_encode_entropy("host")
    assert dev.jpeg_encode(frames, quality=quality, sampling=s) == want
    assert dev.jpeg_downloaded_bytes() == coef.nbytes


@pytest.mark.parametrize("part", range(2))
def test_encode_with_optimize_gives_pillows_bytes_in_both_entropy_modes(ck, part):
    mine = cases.all_cases()[part::6]
    for mode in ("device", "host"):
        ck.jpeg_set_encode_entropy(mode)
        try:
            for k, c in enumerate(mine):
                img = cases.case_image(c)
                out = ck.jpeg_encode(_hbm(img) if k & 1 else img, quality=c[4], sampling=c[3], restart_interval=c[5], optimize=True)
                assert out == [cases.golden(c)], (mode, cases.name_of(c))
        finally:
            ck.jpeg_set_encode_entropy("host")


def test_with_the_setting_at_its_default_the_streams_are_the_standard_ones(dev):
    """before and after optimised calls in the same context, per call and per context; jpeg_enc_cases holds Pillow's bytes
    without optimize"""
    mine = [c for c in base.all_cases() if (c[1], c[2]) in ((17, 33), (48, 64))][::3]
    img0 = cases.case_image(cases.BATCH[0])
    for k, c in enumerate(mine):
        img = base.case_image(c)
        assert dev.jpeg_encode(img, quality=c[4], sampling=c[3], restart_interval=c[5]) == [base.golden(c)], base.name_of(c)
        if k % 3 == 0:
            assert dev.jpeg_encode(img0, optimize=True) == [cases.golden(cases.BATCH[0])]
        if k % 3 == 1:
            dev.jpeg_set_encode_tables("optimised")
            assert dev.jpeg_encode(img0) == [cases.golden(cases.BATCH[0])]
            dev.jpeg_set_encode_tables("standard")
        coef = base.ref_forward(c).reshape(1, -1)
        assert dev.jpeg_entropy_encode_device(coef, ref.quant_tables(c[4]), c[1], c[2], c[3], c[5]) == [base.golden(c)]
    from camkifu_amd import capi
    with pytest.raises(capi.CkError, match="'standard' or 'optimised'"):
        dev.jpeg_set_encode_tables("optimized-ish")
    L = capi.lib()
    assert L.ck_jpeg_set_encode_tables(dev._h, 2) == capi.CK_ERR_ARG and b"table mode 2" in L.ck_last_error(dev._h)
    with pytest.raises(capi.CkError, match="the last pass counted 0 frames"):
        dev.jpeg_encode_histograms(1)                                      # the last pass was a standard one


def test_the_optimised_film_decodes_in_every_entropy_mode_to_the_standard_films_coefficients(dev):
    from camkifu_amd import capi
    c0 = cases.BATCH[0]
    frames = np.stack([cases.case_image(c) for c in cases.BATCH])
    film = dev.jpeg_encode(frames, quality=c0[4], sampling=c0[3], optimize=True)
    standard = dev.jpeg_encode(frames, quality=c0[4], sampling=c0[3])
    assert all(len(a) < len(b) for a, b in zip(film, standard))
    _, coef, quant = capi.jpeg_coefficients(film)
    _, coef_std, quant_std = capi.jpeg_coefficients(standard)
    assert np.array_equal(coef, coef_std) and np.array_equal(quant, quant_std)
    assert np.array_equal(coef, np.stack([cases.ref_forward(c) for c in cases.BATCH]))
    pixels = np.stack([jpeg_ref.decode(cases.golden(c)) for c in cases.BATCH])       # of Pillow's bytes
    try:
        for mode in ("host", "device", "device-spans"):
            dev.jpeg_set_entropy(mode)
            assert np.array_equal(dev.jpeg_decode(film), pixels), mode
            if mode != "host":
                assert np.array_equal(dev.jpeg_coefficients_device(film)[1], coef), mode
    finally:
        dev.jpeg_set_entropy("host")


def test_refusals_are_the_host_coders_and_the_context_goes_on(ck):
    from camkifu_amd import capi
    c = ("noise", 17, 23, ref.S420, 90, 2)
    q = ref.quant_tables(c[4])
    good = cases.ref_forward(c)
    for k, (place, value) in enumerate(((64 * 3 + 5, 2000), (64 * 7, -32768), (64 * 11 + 63, -1024))):
        coef = np.stack([good, good, good]).copy()
        coef[1:, place] = value
        with pytest.raises(capi.CkError) as host:
            capi.jpeg_entropy_encode(coef, q, c[1], c[2], c[3], c[5])
        with pytest.raises(capi.CkError) as got:
            ck.jpeg_entropy_encode_device(_hbm(coef) if k & 1 else coef, q, c[1], c[2], c[3], c[5], optimize=True)
        assert (got.value.code, str(got.value)) == (host.value.code, str(host.value)) and "frame 1: " in str(got.value)
    assert ck.jpeg_entropy_encode_device(good.reshape(1, -1), q, c[1], c[2], c[3], c[5], optimize=True) == [cases.golden(c)]


def test_the_two_new_steps_are_in_the_timing_table_with_optimised_tables_only(dev):
    img = cases.case_image(cases.BATCH[0])
    dev.timing_enable(True)
    try:
        dev.timing_reset()
        dev.jpeg_encode(img)
        counts = {k: dev.timing_get(k)[1] for k in KERNELS}
        assert counts == {"jpeg_enc_histo": 0, "jpeg_enc_tables": 0, "jpeg_enc_size": 1, "jpeg_enc_scan": 1, "jpeg_enc_put": 1, "jpeg_enc_stuff": 2}
        dev.timing_reset()
        dev.jpeg_encode(img, optimize=True)
        counts = {k: dev.timing_get(k)[1] for k in KERNELS}
        assert counts == {"jpeg_enc_histo": 1, "jpeg_enc_tables": 1, "jpeg_enc_size": 1, "jpeg_enc_scan": 1, "jpeg_enc_put": 1, "jpeg_enc_stuff": 2}
    finally:
        dev.timing_enable(False)


def test_the_writers_and_the_transcoder_with_optimize(ck, tmp_path):
    """write_jpeg, MjpegWriter and tools/transcode.py hand optimize on to jpeg_encode: the chunks are Pillow's optimised bytes,
    the film is smaller than the standard one and reads back to the same frames; the context's setting is what it was"""
    import importlib.util
    import os

    from camkifu_amd.core import capture
    spec = importlib.util.spec_from_file_location("transcode", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                             "tools", "transcode.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    c0 = cases.BATCH[0]
    film = np.stack([cases.case_image(c) for c in cases.BATCH])
    want = [cases.golden(c) for c in cases.BATCH]
    still = str(tmp_path / "still.jpg")
    assert capture.write_jpeg(still, film[0], quality=c0[4], encode=ck.jpeg_encode, optimize=True) == len(want[0])
    with open(still, "rb") as f:
        assert f.read() == want[0]
    opt_avi, std_avi = str(tmp_path / "opt.avi"), str(tmp_path / "std.avi")
    res = tr.transcode(film, opt_avi, quality=c0[4], batch=2, ctx=ck, optimize=True)
    std = tr.transcode(film, std_avi, quality=c0[4], batch=2, ctx=ck)
    assert res["frames"] == std["frames"] == 3 and res["bytes"] < std["bytes"]
    with open(opt_avi, "rb") as f:
        assert jpeg_ref.avi_index(f.read())["chunks"] == want
    with open(std_avi, "rb") as f:
        assert jpeg_ref.avi_index(f.read())["chunks"] == [ref.encode(fr, c0[4], ref.S420) for fr in film]
    a, b = capture.AviMjpegCapture(opt_avi, decode=ck.jpeg_decode), capture.AviMjpegCapture(std_avi, decode=ck.jpeg_decode)
    for _ in range(3):
        assert np.array_equal(a.read()[1], b.read()[1])

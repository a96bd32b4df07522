"""Optimised Huffman tables on the host: the plain-Python rule (jpeg_enc_opt_ref), the two-pass host coder
(ck_jpeg_entropy_encode_opt) and the kernels' steps in plain loops (ck_jpeg_entropy_encode_opt_staged) each give Pillow's
bytes, optimize=True, on every committed case; ck_jpeg_histogram and ck_jpeg_optimal_table equal the reference; the
refusals are the standard host coder's."""
import numpy as np
import pytest

from camkifu_amd import capi

from . import jpeg_enc_opt_cases as cases
from . import jpeg_enc_opt_ref as opt
from . import jpeg_enc_ref as ref


@pytest.fixture(scope="module", autouse=True)
def _built():
    capi.build()


def _quant(case):
    return ref.quant_tables(case[4])


def test_the_fixture_holds_every_case_and_smaller_streams_than_the_standard_tables():
    from . import jpeg_enc_cases as base
    assert sorted(cases.goldens()) == sorted(cases.name_of(c) for c in cases.all_cases())
    assert len(cases.matrix()) == 96
    # the same picture with the standard tables is in the encoder's own goldens: optimised is smaller
    both = [c for c in cases.all_cases() if cases.name_of(c) in base.goldens() and c[0] != "flat"]
    assert both
    for c in both:
        assert len(cases.golden(c)) < len(base.goldens()[cases.name_of(c)]), cases.name_of(c)


def test_the_reference_gives_pillows_bytes_on_every_case():
    for c in cases.all_cases():
        assert cases.ref_encode(c) == cases.golden(c), cases.name_of(c)


@pytest.mark.parametrize("staged", [False, True], ids=["two-pass", "staged"])
def test_the_host_coders_give_pillows_bytes_on_every_case(staged):
    fn = capi.jpeg_entropy_encode_staged if staged else capi.jpeg_entropy_encode
    for c in cases.all_cases():
        got = fn(cases.ref_forward(c), _quant(c), c[1], c[2], c[3], c[5], optimize=True)
        assert got == cases.golden(c), cases.name_of(c)


@pytest.mark.parametrize("staged", [False, True], ids=["two-pass", "staged"])
def test_a_batch_of_three_pictures_gets_three_table_sets_and_header_lengths(staged):
    fn = capi.jpeg_entropy_encode_staged if staged else capi.jpeg_entropy_encode
    c0 = cases.BATCH[0]
    coef = np.stack([cases.ref_forward(c) for c in cases.BATCH])
    got = fn(coef, _quant(c0), c0[1], c0[2], c0[3], c0[5], optimize=True)
    assert got == [cases.golden(c) for c in cases.BATCH]
    assert len({g.index(b"\xff\xda") for g in got}) == 3              # three header lengths


@pytest.mark.parametrize("name", sorted(cases.built()))
def test_built_coefficients_zrl_no_eob_and_limited_lengths(name):
    coef, h, w, s, ri = cases.built()[name]
    want = cases.built_ref(name)
    q = ref.quant_tables(90)
    assert capi.jpeg_entropy_encode(coef, q, h, w, s, ri, optimize=True) == want
    assert capi.jpeg_entropy_encode_staged(coef, q, h, w, s, ri, optimize=True) == want
    freq = opt.histogram(coef, h, w, s, ri)
    assert np.array_equal(capi.jpeg_histogram(coef, h, w, s, ri), freq)
    if name == "length_limited":
        assert (freq[1] > 0).sum() == 22 and freq[1][0] == 0 and max(opt.code_sizes(freq[1])) == 22       # no EOB; the lengths had to be limited
        assert sorted(freq[1][freq[1] > 0])[:21] == cases.fibonacci(22)[1:]
        dc_bits, _ = opt.optimal_table(freq[0])
        assert (freq[0] > 0).sum() == 12 and max(l for l in range(1, 17) if dc_bits[l - 1]) == 12
    else:
        assert freq[1][0xF0] == 3 + (1 + 2) + 2 and freq[1][0x00] == 1   # runs of 62; 16 and 45; 39: eight ZRL, one EOB


@pytest.mark.parametrize("case", [c for c in cases.all_cases() if (c[1], c[2]) == (17, 23) and c[4] == 90], ids=cases.name_of)
def test_the_histogram_counts_the_coders_symbols_dummy_blocks_and_restarts_included(case):
    coef = cases.ref_forward(case)
    got = capi.jpeg_histogram(coef, case[1], case[2], case[3], case[5])
    want = opt.histogram(coef, case[1], case[2], case[3], case[5])
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    if case[3] == ref.GREY:
        assert not got[2:].any()
    # a batch: frame by frame
    two = capi.jpeg_histogram(np.stack([coef, coef]), case[1], case[2], case[3], case[5])
    assert two.shape == (2, 4, 256) and np.array_equal(two[0], want) and np.array_equal(two[1], want)


@pytest.mark.parametrize("name", sorted(cases.table_inputs()))
def test_the_optimal_table_is_the_references_and_a_valid_code(name):
    freq = cases.table_inputs()[name]
    bits, vals = capi.jpeg_optimal_table(freq.astype(np.uint32))
    rbits, rvals = opt.optimal_table(freq)
    assert list(bits) == rbits and list(vals) == rvals
    assert sorted(vals) == [i for i in range(256) if freq[i]]               # every counted symbol, once
    assert int(bits.sum()) == len(vals)                                     # (so no length is above 16)
    kraft = sum(int(b) * 2 ** (16 - l) for l, b in enumerate(bits, 1))
    assert kraft <= 2 ** 16 - 1                                             # Kraft's sum at most 1, and room for the code of all ones
    codes = opt.code_lengths(bits, vals)
    assert all(code != (1 << length) - 1 for code, length in codes.values())
    if name in ("fibonacci", "big"):
        assert max(opt.code_sizes(freq)) > 16 and bits[15] > 0                 # limited, and the longest length is in use
    if name.startswith("single"):
        assert list(bits) == [1] + [0] * 15
    if name == "equal":
        assert list(bits) == [0] * 7 + [255, 1] + [0] * 7                   # 257 leaves: 255 at depth 8, two at 9, the pseudo-symbol one of them


def test_refusals_are_the_host_coders_same_frame_same_message():
    c = ("noise", 17, 23, ref.S420, 90, 2)
    q = _quant(c)
    good = cases.ref_forward(c)
    for place, value in ((64 * 3 + 5, 2000), (64 * 7, -32768), (64 * 11 + 63, -1024)):
        coef = np.stack([good, good, good]).copy()
        coef[2, place] = value
        coef[1, place] = value
        msgs = []
        for kw in (dict(), dict(optimize=True)):
            for fn in (capi.jpeg_entropy_encode, capi.jpeg_entropy_encode_staged):
                with pytest.raises(capi.CkError) as e:
                    fn(coef, q, c[1], c[2], c[3], c[5], **kw)
                msgs.append(str(e.value))
        assert len(set(msgs)) == 1 and "frame 1: " in msgs[0] and "baseline JPEG has" in msgs[0], msgs
        with pytest.raises(capi.CkError, match="frame 1: .*baseline JPEG has"):
            capi.jpeg_histogram(coef, c[1], c[2], c[3], c[5])
    with pytest.raises(capi.CkError, match="quant entry"):
        capi.jpeg_entropy_encode(good, np.zeros((3, 64), np.uint16), c[1], c[2], c[3], optimize=True)
    with pytest.raises(capi.CkError, match="restart interval"):
        capi.jpeg_entropy_encode(good, q, c[1], c[2], c[3], 65536, optimize=True)


def test_a_frame_of_more_than_2_25_blocks_is_refused_before_anything_is_read():
    """(the entry points refuse a frame of more than 2^28 pixels, which is fewer blocks, in words of their own; the coder's own
    2^25 check is driven by tools/sanitize/jpeg_enc_opt_fuzz.cpp)"""
    import ctypes as C
    L = capi.lib()
    h = w = 65535                                          # 8192 x 8192 blocks of luma alone
    one = np.zeros(64, np.int16)                           # nothing of it is read: the geometry is refused first
    q = ref.quant_tables(90)
    counts = np.zeros((4, 256), np.uint32)
    assert L.ck_jpeg_histogram(one.ctypes.data_as(C.c_void_p), 1, h, w, ref.GREY, 0, counts.ctypes.data_as(C.c_void_p)) == capi.CK_ERR_ARG
    out, lens = np.zeros(16, np.uint8), (C.c_size_t * 1)()
    stride = 1 << 20
    for fn in (L.ck_jpeg_entropy_encode_opt, L.ck_jpeg_entropy_encode_opt_staged):
        rc = fn(one.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), 1, h, w, ref.GREY, 0, out.ctypes.data_as(C.c_void_p), stride, lens)
        assert rc == capi.CK_ERR_ARG and lens[0] == 0


def test_the_bound_holds_for_streams_whose_codes_are_longer_than_the_standard_ones():
    coef, h, w, s, ri = cases.length_limited()
    assert len(cases.built_ref("length_limited")) <= capi.jpeg_encode_bound(h, w, s) == ref.size_bound(h, w, s)


def test_writers_hand_optimize_on_only_when_it_is_set(tmp_path):
    from camkifu_amd.core import capture
    seen = []

    def encode(frames, quality, sampling, **kw):
        seen.append(kw)
        return [b"\xff\xd8\xff\xd9"] * len(frames)

    img = np.zeros((8, 8, 3), np.uint8)
    capture.write_jpeg(str(tmp_path / "a.jpg"), img, encode=encode)
    capture.write_jpeg(str(tmp_path / "b.jpg"), img, encode=encode, optimize=True)
    with capture.MjpegWriter(str(tmp_path / "a.avi"), 8, 8, encode=encode) as wr:
        wr.write(img[None])
    with capture.MjpegWriter(str(tmp_path / "b.avi"), 8, 8, encode=encode, optimize=True, restart_interval=2) as wr:
        wr.write(img[None])
    assert seen == [{}, {"optimize": True}, {}, {"restart_interval": 2, "optimize": True}]

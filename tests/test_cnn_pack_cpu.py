"""The classifier's weight packs (csrc/ck_cnn_pack.cpp) through the ck_cnn_pack_probe hook and ctypes, no GPU: every pack
of three weight sets byte for byte against the numpy restatement of the layouts (tests/cnn_pack_ref.py) and against the
SHA-256 digests of tests/golden/cnn_pack_digests.json, which were recorded from the pack loops as they stood in the .hip
files before they were collapsed into one packer (moved verbatim into a host file, nothing else changed).  Then, on small
cases worked by hand: the padding, the split planes, q8_ok and the e4m3 encoder.

The third weight set is synth.cnn_weights(seed=RANDOM_SEED) with OUT_OF_RANGE written into one conv3 weight.

Mutants of ck_cnn_pack.cpp, each tried once, and the tests that failed for them:
  - flip dropped (Conv::at reads tap (i, j) itself): the reference, the digests, single elements, the planes
  - hi / lo planes swapped in the Split encoder: the reference, the digests, single elements, padding, the planes
  - lane / 16 and lane % 16 exchanged in conv_k32's map: the reference, the digests, single elements, padding, the planes
  - one padding channel non-zero (c < CIN + 1 in Conv::at): the reference, the digests, padding, the planes, q8_ok
  - the q > 6 saturation removed from e4m3_of: NOTHING fails, and nothing can.  e4m3_of clamps |v| to 448 before it splits
    the value, so behind the clamp e == 8 comes with q <= 6: the branch is dead code, and with the clamp taken out instead
    the branch alone saturates and every test passes as well.  The encoder saturates twice; it is kept as the packs have
    always used it.  With the clamp taken out and the q > 6 term removed, test_e4m3_of (480 -> 0x7F), the reference and
    the digests of the out-of-range set fail.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from . import cnn_pack_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnn_pack_digests.json")
RANDOM_SEED = 20261
OUT_OF_RANGE = ((1, 2, 5, 17), 7.5)          # c3w[1, 2, 5, 17] = 7.5: hi = 7.5 * 2^8 = 1920 > 448 * 4


@pytest.fixture(scope="module")
def packlib():
    from camkifu_amd import capi
    capi.build()
    L = C.CDLL(capi.SO_PATH)
    L.ck_cnn_pack_probe.restype = C.c_longlong
    L.ck_cnn_pack_probe.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.ck_cnn_e4m3_probe.restype = None
    L.ck_cnn_e4m3_probe.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def weight_sets():
    from camkifu_amd import synth
    from camkifu_amd.capi import WEIGHT_ORDER
    from camkifu_amd.stone.nn_manager import NNManager
    rnd = synth.cnn_weights(seed=RANDOM_SEED)
    rnd["c3w"][OUT_OF_RANGE[0]] = OUT_OF_RANGE[1]
    sets = dict(shipped=NNManager.init_net(), synth=synth.cnn_weights(), out_of_range=rnd)
    return {s: {k: np.ascontiguousarray(W[k], np.float32) for k in WEIGHT_ORDER} for s, W in sets.items()}


def lib_pack(L, W, name):
    """-> (the pack's bytes, q8_ok) from the library"""
    from camkifu_amd.capi import WEIGHT_ORDER
    ptrs = (C.c_void_p * 12)(*[W[k].ctypes.data for k in WEIGHT_ORDER])
    ok = C.c_int(-1)
    n = L.ck_cnn_pack_probe(ptrs, name.encode(), None, 0, C.byref(ok))
    assert n > 0, name
    buf = np.full(n, 0xA5, np.uint8)
    assert L.ck_cnn_pack_probe(ptrs, name.encode(), buf.ctypes.data, n, None) == n
    return buf.tobytes(), bool(ok.value)


@pytest.fixture(scope="module")
def packs(packlib):
    """set name -> (dict pack name -> bytes from the library, q8_ok)"""
    out = {}
    for s, W in weight_sets().items():
        got = {name: lib_pack(packlib, W, name) for name in ref.PACKS}
        assert len({ok for _, ok in got.values()}) == 1
        out[s] = ({name: b for name, (b, _) in got.items()}, got["c1w"][1])
    return out


def _view(packs, s, name, dtype, shape):
    return np.frombuffer(packs[s][0][name], dtype).reshape(shape)


def test_unknown_pack_name(packlib):
    W = weight_sets()["synth"]
    from camkifu_amd.capi import WEIGHT_ORDER
    ptrs = (C.c_void_p * 12)(*[W[k].ctypes.data for k in WEIGHT_ORDER])
    assert packlib.ck_cnn_pack_probe(ptrs, b"c9w", None, 0, None) == -1


@pytest.mark.parametrize("s", ["shipped", "synth", "out_of_range"])
def test_packs_equal_the_reference(packs, s):
    want, want_ok = ref.pack_all(weight_sets()[s])
    got, got_ok = packs[s]
    for name in ref.PACKS:
        assert len(got[name]) == len(want[name]), name
        if got[name] != want[name]:
            a, b = np.frombuffer(got[name], np.uint8), np.frombuffer(want[name], np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError("%s of %s: %d bytes differ, the first at %d" % (name, s, bad.size, bad[0]))
    assert got_ok == want_ok == (s != "out_of_range")


@pytest.mark.parametrize("s", ["shipped", "synth", "out_of_range"])
def test_packs_have_the_recorded_digests(packs, s):
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == ["out_of_range", "shipped", "synth"] and sorted(golden[s]) == sorted(ref.PACKS + ("q8_ok",))
    for name in ref.PACKS:
        assert hashlib.sha256(packs[s][0][name]).hexdigest() == golden[s][name], name
    assert packs[s][1] == golden[s]["q8_ok"]


def test_plain_copies(packs):
    W = weight_sets()["shipped"]
    for name in ("c1b", "c2b", "c3b", "c4b", "d1b", "d2w", "d2b"):
        assert packs["shipped"][0][name] == W[name].tobytes(), name


def test_single_elements_worked_by_hand(packs):
    """one element of each kind of layout, its place worked out on paper from the layout comments"""
    W = weight_sets()["synth"]
    # conv2 f32, k = (tap 7 = (1, 2), cin 9) = 7 * 32 + 9 = 233: step 58 = group 14 e 2, kslot 1; cout 21 = tile 1 column 5
    v = _view(packs, "synth", "c2w", np.float32, (2, 50, 64, 4))
    assert v[1, 14, 16 + 5, 2] == W["c2w"][4 - 1, 4 - 2, 9, 21]
    # conv1 f32, k = (1, 3, 2) = 1 * 15 + 3 * 3 + 2 = 26: step 6 kslot 2; cout 30 = tile 1 column 14
    v = _view(packs, "synth", "c1w", np.float32, (2, 19, 64))
    assert v[1, 6, 32 + 14] == W["c1w"][3, 1, 2, 30]
    # dense 1 f32, input 1001 = 4 * 250 + 1: pair 125 e 0, kslot 1; output 37 = tile 2 column 5
    v = _view(packs, "synth", "d1w", np.float32, (10, 405, 64, 2))
    assert v[2, 125, 16 + 5, 0] == W["d1w"][1001, 37]
    # conv4 bf16, tap (2, 0), cin 77 = block 2, kslot 1, e 5: step 6 * 3 + 2 = 20; cout 89 = tile 5 column 9
    v = _view(packs, "synth", "c4w_bf", np.uint16, (6, 27, 64, 8))
    assert v[5, 20, 16 + 9, 5] == ref.bf16(W["c4w"][0, 2, 77, 89])
    # conv1 fp16 rows, kernel row 3, columns (2, 3) = pair 1: f = 10 = step 2 kslot 2; column 3 cin 1 = e 5; cout 3
    v = _view(packs, "synth", "c1w_f16", np.float16, (2, 4, 64, 8))
    assert v[0, 2, 32 + 3, 5] == np.float16(W["c1w"][4 - 3, 4 - 3, 1, 3])
    # dense 1 bf16 over the padded maps, pixel 20 channel 50: k = 20 * 96 + 50 = 1970 = 32 * 61 + 8 * 2 + 2; output 159
    v = _view(packs, "synth", "d1w_bfp", np.uint16, (10, 108, 64, 8))
    assert v[9, 61, 32 + 15, 2] == ref.bf16(W["d1w"][20 * 90 + 50, 159])
    # conv1 of the split mode, kernel row 3 = step 1 kslot 2 or 3; slot (kw 3, cin 1) = 10 = 8 + 2: kslot 3, e 2; cout 17
    v = _view(packs, "synth", "c1w_h2", np.float16, (2, 3, 2, 64, 8))
    hi, lo = ref.split(W["c1w"][4 - 3, 4 - 3, 1, 17])
    assert v[1, 1, 0, 48 + 1, 2] == hi and v[1, 1, 1, 48 + 1, 2] == lo
    # conv3 split, tap (0, 1), cin 31: step 1, kslot 3, e 7; cout 40 = tile 2 column 8
    v = _view(packs, "synth", "c3w_h2", np.float16, (6, 9, 2, 64, 8))
    hi, lo = ref.split(W["c3w"][2, 1, 31, 40])
    assert v[2, 1, 0, 48 + 8, 7] == hi and v[2, 1, 1, 48 + 8, 7] == lo
    # conv1 for the e4m3 mode: the fp16 rows' place, the planes outermost
    v = _view(packs, "synth", "c1w_q8", np.float16, (2, 2, 4, 64, 8))
    hi, lo = ref.split(W["c1w"][4 - 3, 4 - 3, 1, 3])
    assert v[0, 0, 2, 32 + 3, 5] == hi and v[1, 0, 2, 32 + 3, 5] == lo
    # conv2 cross terms, tap (3, 3) = second half of pair 3 * 3 + 1 = 10, cin 20 = group 1 (lo) / 3 (hi), e 4; cout 21
    v = _view(packs, "synth", "c2x_q8", np.uint8, (2, 18, 64, 32))
    hi, lo = ref.split(W["c2w"][4 - 3, 4 - 3, 20, 21])
    assert v[1, 10, 16 + 5, 16 + 4] == ref.e4m3(np.float32(lo) * 512) and v[1, 10, 48 + 5, 16 + 4] == ref.e4m3(np.float32(hi) / 4)
    # conv4 cross terms, k-step 13 = tap 4 = (1, 1), block 1: second half of pair 6; cin 32 + 3 = group 0 / 2, e 3; cout 0
    v = _view(packs, "synth", "c4x_q8", np.uint8, (6, 14, 64, 32))
    hi, lo = ref.split(W["c4w"][1, 1, 35, 0])
    assert v[0, 6, 0, 16 + 3] == ref.e4m3(np.float32(lo) * 512) and v[0, 6, 32, 16 + 3] == ref.e4m3(np.float32(hi) / 4)


def test_padding_is_zero(packs):
    """the padding of every layout is zero bytes and what lies next to it is not (no weight of the random set is zero)"""
    s = "out_of_range"

    def zero_beside(v, pad, full):
        assert not v[pad].any() and v[full].all()

    # cin 3 -> 4: every fourth element of the conv1 rows
    # (of a split pack only the hi plane is all non-zero: a lo half is zero whenever hi holds the weight exactly)
    for name, shape in (("c1w_f16", (1, 2, 4, 64, 2, 4)), ("c1w_q8", (2, 2, 4, 64, 2, 4))):
        v = _view(packs, s, name, np.uint16, shape)
        zero_beside(v[:, :, :3], np.s_[..., 3], np.s_[0, ..., 0, :3])                 # (steps 0 .. 2: all 12 units are real)
    # ... the third column pair (4, -) has one column, and the 16th unit (step 3, kslot 3) does not exist
    v = _view(packs, s, "c1w_f16", np.uint16, (2, 4, 4, 16, 2, 4))
    zero_beside(v, np.s_[:, 3, 3], np.s_[:, 3, 2, :, 0, :3])
    zero_beside(v, np.s_[:, 0, 2, :, 1], np.s_[:, 0, 2, :, 0, :3])                    # f = 2: columns (4, -)
    # cin 90 -> 96 and cout 90 -> 96 in the 16-bit conv4 fragments: block 2, kslot 3 holds cin 88 .. 95
    for name, planes in (("c4w_bf", 1), ("c4w_h2", 2)):
        v = _view(packs, s, name, np.uint16, (6, 9, 3, planes, 4, 16, 8))
        zero_beside(v[:5], np.s_[:, :, 2, :, 3, :, 2:], np.s_[:, :, 2, 0, 3, :, :2])
        zero_beside(v[5], np.s_[..., 10:, :], np.s_[:, :2, 0, :, :10, :])
    for name, planes in (("c3w_bf", 1), ("c3w_h2", 2)):
        v = _view(packs, s, name, np.uint16, (6, 9, planes, 4, 16, 8))
        zero_beside(v[5], np.s_[..., 10:, :], np.s_[:, 0, :, :10, :])
    # cout 90 -> 96 in the f32 fragments; cin 90 -> 92 of conv4: k-steps of 4 never straddle a tap (92 = 4 * 23), step 22 of
    # each tap holds cin 88 .. 91, and group 51 holds steps 204 .. 207 of which 207 does not exist
    v = _view(packs, s, "c3w", np.uint32, (6, 18, 4, 16, 4))
    zero_beside(v[5], np.s_[..., 10:, :], np.s_[..., :10, :])
    v = _view(packs, s, "c4w", np.uint32, (6, 52, 4, 16, 4))
    zero_beside(v[5], np.s_[..., 10:, :], np.s_[:5, :, :10, :])                          # (groups 0 .. 4: cin 0 .. 79 of tap 0)
    zero_beside(v[:5], np.s_[:, 51, :, :, 3], np.s_[:, 51, :2, :, :3])                # step 206 = tap 8 step 22: kslots 0, 1 real
    zero_beside(v[:5], np.s_[:, 5, 2:, :, 2], np.s_[:, 5, :2, :, 2])                  # step 22 = 4 * 5 + 2: cin 90, 91 are padding
    # k = 75 of conv1: step 18, kslot 3
    v = _view(packs, s, "c1w", np.uint32, (2, 19, 4, 16))
    zero_beside(v, np.s_[:, 18, 3], np.s_[:, 18, :3])
    # k >= 3240 of dense 1: 3240 = 32 * 101 + 8, so step 101 keeps kslot 0 only
    v = _view(packs, s, "d1w_h2", np.uint16, (10, 104, 2, 4, 16, 8))
    zero_beside(v, np.s_[:, 101, :, 1:], np.s_[:, 101, 0, 0])
    assert not v[:, 102:].any() and v[:, :101, 0].all()
    # channels 90 .. 95 of the padded maps
    v = _view(packs, s, "d1w_bfp", np.uint16, (10, 36, 3, 4, 16, 8))
    zero_beside(v, np.s_[:, :, 2, 3, :, 2:], np.s_[:, :, 2, 3, :, :2])
    # the empty halves of the cross-term pairs.  (A single code can be zero next to them: a small term rounds to it.  Of the
    # halves that exist, every lane of the hi groups holds some non-zero code.)
    for name, nt, npair, empty in (("c2x_q8", 2, 18, [2, 5, 8, 11, 14, 17]), ("c3x_q8", 6, 8, [1, 3, 5, 7]), ("c4x_q8", 6, 14, [13])):
        v = _view(packs, s, name, np.uint8, (nt, npair, 4, 16, 2, 16))
        assert not v[:, empty, :, :, 1].any()
        assert v[:nt - 1 if nt == 6 else nt, :, 2:, :, 0].any(axis=-1).all()
        if nt == 6:
            assert not v[5, :, :, 10:].any()
    v = _view(packs, s, "c4x_q8", np.uint8, (6, 14, 4, 16, 32))
    assert not v[:, 1, 1::2, :, 10:16].any() and not v[:, 2, 1::2, :, 26:].any()       # k-steps 2 and 5 are blocks 2: cin 64 + 16 + 10 ..
    assert v[:5, 1, 3, :, :10].any(axis=-1).all() and v[:5, 2, 3, :, 16:26].any(axis=-1).all()


def test_planes_reassemble_the_scaled_weight(packs):
    """hi + lo = w x 2^8 to within one fp16 ulp of lo, on whole packs through the reference's source maps"""
    for s, W in weight_sets().items():
        for name, src, axis in (("c1w_h2", ref.conv1_h2_rows(W["c1w"]), 2), ("c2w_h2", ref.conv_k32(W["c2w"], 32, 32), 2),
                                ("c3w_h2", ref.conv_k32(W["c3w"], 32, 96), 2), ("c4w_h2", ref.conv_k32(W["c4w"], 96, 96), 2),
                                ("d1w_h2", ref.fc1_k32(W["d1w"], False), 2), ("c1w_q8", ref.conv1_rows(W["c1w"]), 0)):
            shape = src.shape[:axis] + (2,) + src.shape[axis:]
            hi, lo = np.moveaxis(_view(packs, s, name, np.float16, shape), axis, 0).astype(np.float64)
            err = np.abs(src.astype(np.float64) * 256 - (hi + lo))
            assert (err <= np.spacing(np.abs(lo).astype(np.float16)).astype(np.float64)).all(), (s, name)
            assert (np.abs(lo) <= np.spacing(np.abs(hi).astype(np.float16)).astype(np.float64) / 2).all(), (s, name)     # lo is hi's rounding error
    # by hand: 1 / 3 x 2^8 = 85.3333358765 (f32) -> hi = 85.3125 (ulp 2^-4), lo = 0.0208358765 -> 0.020828247 (ulp 2^-21 x 2^5 = 2^-16 ..)
    hi, lo = ref.split(np.float32(1) / np.float32(3))
    assert float(hi) == 85.3125 and abs(float(lo) - (float(np.float32(1) / np.float32(3)) * 256 - 85.3125)) <= 2.0 ** -16


def test_q8_ok_follows_the_largest_hi(packlib):
    """the flag turns at 448 x 4 = 1792 exactly: 7.0 x 2^8 = 1792 is inside, the next fp16 hi (1793 -> 1794, w = 1793 / 256) is not;
    conv1's weights do not count (its products stay on the fp16 pipe)"""
    W = weight_sets()["synth"]
    for name, at in (("c2w", (0, 0, 0, 0)), ("c3w", (2, 2, 31, 89)), ("c4w", (1, 1, 89, 89))):
        for value, ok in ((7.0, True), (-7.0, True), (1793.0 / 256, False), (-8.0, False)):
            V = dict(W)
            V[name] = W[name].copy()
            V[name][at] = value
            assert lib_pack(packlib, V, "c2x_q8")[1] is ok, (name, value)
    V = dict(W)
    V["c1w"] = W["c1w"] * np.float32(4096)
    assert lib_pack(packlib, V, "c2x_q8")[1] is True


def _e4m3_lib(L, v):
    v = np.ascontiguousarray(v, np.float32)
    out = np.full(v.size, 0xA5, np.uint8)
    L.ck_cnn_e4m3_probe(v.ctypes.data, v.size, out.ctypes.data)
    return out


def test_e4m3_of(packlib):
    vals = ref.e4m3_values()
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F])
    # the table itself, on a few codes worked by hand: 0x01 = 2^-9, 0x07 = 7 x 2^-9, 0x08 = 2^-6, 0x38 = 1, 0x7E = 448
    assert [vals[c] for c in (0x01, 0x07, 0x08, 0x38, 0x3C, 0x7E, 0xFE)] == [2.0 ** -9, 7 * 2.0 ** -9, 2.0 ** -6, 1.0, 1.5, 448.0, -448.0]
    # every code's exact value comes back as that code (-0 = 0x80 has the value zero: code 0)
    got = _e4m3_lib(packlib, vals[codes])
    assert np.array_equal(got, np.where(codes == 0x80, 0, codes))
    # the midpoints between neighbours go to the even code, and a step to either side of them to the nearer one
    pos = np.arange(0x7E)
    mid = ((vals[pos] + vals[pos + 1]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (vals[pos] + vals[pos + 1]) / 2)           # (exact in f32)
    even = np.where(pos % 2 == 0, pos, pos + 1)
    assert np.array_equal(_e4m3_lib(packlib, mid), even)
    assert np.array_equal(_e4m3_lib(packlib, -mid), even | 0x80)
    assert np.array_equal(_e4m3_lib(packlib, np.nextafter(mid, np.float32(0))), pos)
    assert np.array_equal(_e4m3_lib(packlib, np.nextafter(mid, np.float32(1000))), pos + 1)
    # saturation, the subnormal boundary, zeros, NaN
    cases = [(448.0, 0x7E), (-448.0, 0xFE), (449.0, 0x7E), (-449.0, 0xFE), (464.0, 0x7E), (480.0, 0x7E), (1e30, 0x7E), (np.inf, 0x7E),
             (-np.inf, 0xFE), (432.0, 0x7E), (431.9, 0x7D),
             (2.0 ** -6, 0x08), (-2.0 ** -6, 0x88), (2.0 ** -6 - 2.0 ** -10, 0x08), (2.0 ** -6 - 2.0 ** -9, 0x07), (2.0 ** -6 + 2.0 ** -10, 0x08),
             (2.0 ** -6 + 2.0 ** -9, 0x09), (2.0 ** -10, 0x00), (2.0 ** -10 * 1.01, 0x01), (3 * 2.0 ** -10, 0x02),
             (0.0, 0x00), (-0.0, 0x00), (np.nan, 0x00)]
    v = np.array([c[0] for c in cases], np.float32)
    assert _e4m3_lib(packlib, v).tolist() == [c[1] for c in cases]
    assert ref.e4m3(v).tolist() == [c[1] for c in cases]
    # and the reference agrees with the library on a dense sweep
    rng = np.random.default_rng(7)
    sweep = np.concatenate([rng.standard_normal(20000) * s for s in (1e-3, 0.05, 1, 30, 400)]).astype(np.float32)
    assert np.array_equal(_e4m3_lib(packlib, sweep), ref.e4m3(sweep))

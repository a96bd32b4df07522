"""What tests/test_gpu_alignment.py and tests/test_alignment_cpu.py need.

A device tensor handed to capi.Context is taken as it lies: its data_ptr() crosses the C ABI.  torch's allocator hands out
blocks on 512 bytes, so a test that wants another alignment has to make it:

    place(array, offset)   a contiguous tensor that holds `array`, data_ptr() % 16 == offset, inside ONE allocation with
                           `pad` bytes of 0x5A in front of it and behind it (the guard bands)
    untouched(placed)      asserts that every byte of both bands is still 0x5A
    unchanged(placed, a)   asserts that the tensor still holds the bytes of `a`

The bands lie inside the test's own allocation: a store that strays is caught by reading them back, never by a fault.

The tables: ARGS names the element type of every device-capable argument of every method of tests/handover_cases.METHODS
(the offsets of a type: OFFSETS), OUT the element type of what every method with an `out=` parameter writes, REFUSALS the
alignments the library insists on (ALLOWED: the same per capi method, argument and offset).  rows() gives, per method, the rows
of tests/scratch_cases.py that serve and the rows on shapes of this file's own: the handover inputs are too small for some
of the wide paths (96 x 128 holds no interior median tile), so each such row restates the kernel's own condition in
`reaches` and computes its expected value from the plain reference of the method's own test file (`expect`).  Of the four
jpeg_encode rows of tests/scratch_cases.py only the first (host entropy coder, standard tables) has its frames placed: the
other three differ behind the forward kernel, which is the one that reads the frames.

C_EDGES lists the device OUTPUTS of the C ABI that capi never lets a caller place (it allocates them itself) and that reach
a kernel with dword stores: the `edges` of ck_board_edges, ck_goban_canny and ck_canny.  They are placed through ctypes."""
import functools

import numpy as np

from tests import handover_cases as hc
from tests import scratch_cases as sc

GUARD = hc.SENTINEL                      # 0x5A
PAD = 64
OFFSETS = {1: (0, 1, 2, 3, 4, 8), 2: (0, 2, 4, 8), 4: (0, 4, 8)}       # by element size


def stops_at_a_hip_error(test):
    """a HIP error ends the session: nothing more is started on a card that has faulted"""
    @functools.wraps(test)
    def run(*args, **kw):
        import pytest
        from camkifu_amd import capi
        try:
            return test(*args, **kw)
        except capi.CkError as e:
            if getattr(e, "code", None) == capi.CK_ERR_HIP:
                pytest.exit("HIP error, the session ends here: %s" % e, returncode=3)
            raise
    return run


# ------------------------------------------------------------------------------------------------ placement
def place(array, offset, pad=PAD, device="cuda:0"):
    """-> a contiguous tensor on `device` holding `array` (uint16 as int16: the bits count), data_ptr() % 16 == offset"""
    import torch
    a = np.array(array, order="C", copy=True)          # (a copy: the table's arrays may be read-only, which torch.from_numpy warns of)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    assert 0 <= offset < 16 and offset % a.itemsize == 0 and pad >= 16, (offset, a.dtype, pad)
    nbytes = a.nbytes
    flat = torch.full((nbytes + 2 * pad + 32,), GUARD, dtype=torch.uint8, device=device)
    start = pad + (offset - (flat.data_ptr() + pad)) % 16
    flat[start:start + nbytes].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
    t = flat[start:start + nbytes].view(getattr(torch, a.dtype.name)).view(a.shape)
    if t.is_cuda:
        torch.cuda.current_stream().synchronize()
    assert t.is_contiguous() and t.data_ptr() % 16 == offset and t.data_ptr() == flat.data_ptr() + start
    assert start >= pad and flat.numel() - (start + nbytes) >= pad
    t._placed = (flat, start, nbytes)
    return t


def bands(placed):
    """-> (the bytes in front of the tensor, the bytes behind it) as numpy arrays"""
    flat, start, nbytes = placed._placed
    host = flat.cpu().numpy()
    return host[:start], host[start + nbytes:]


def untouched(placed):
    for where, band in zip(("in front of", "behind"), bands(placed)):
        bad = np.nonzero(band != GUARD)[0]
        assert bad.size == 0, "%d bytes of the guard band %s the tensor were written, the first at %d of %d: 0x%02X" % (
            bad.size, where, int(bad[0]), band.size, int(band[bad[0]]))


def unchanged(placed, array):
    flat, start, nbytes = placed._placed
    a = np.ascontiguousarray(array)
    assert flat[start:start + nbytes].cpu().numpy().tobytes() == a.tobytes(), "the call changed its input"


# ------------------------------------------------------------------------------------------------ the tables
U8, I16, U16, I32, F32 = np.uint8, np.int16, np.uint16, np.int32, np.float32
ARGS = dict(median15=(U8,), median=(U8,), goban_canny=(U8,), canny=(U8,), board_edges=(U8,), board_lines=(U8,), board_detect=(U8,),
            board_detect_records=(U8, U8), cnn_regions_records=(U8, U8), i420_to_bgr=(U8,), i420_to_bgr_levels=(U8,),
            jpeg_reconstruct=(I16, U16), jpeg_forward=(U8,), jpeg_encode=(U8,), jpeg_entropy_encode_device=(I16,), overlay_draw=(U8,),
            pyr_down=(U8,), warp_perspective=(U8,), mog2_apply=(U8,), mog2_band_run=(U8,), cnn_set_weights=(F32,) * 12,
            train_create=(F32,) * 12, cnn_predict=(U8,), cnn_maps=(U8,), cnn_regions=(U8,), train_step=(U8,), train_grads=(U8,),
            train_apply=(F32,) * 12, harvest_patches=(U8, I32), augment_patches=(U8,), stones_detect=(U8,), stones_run=(U8,),
            zone_counts=(U8,), contour_stones=(U8, U8), cluster_stones=(U8,), contours_external=(U8,), find_intersections=(U8,),
            png_encode=(U8,))
# png_encode takes frames in HBM too and is younger than the handover table: it has its turn here all the same
METHODS = tuple(hc.METHODS) + ("png_encode",)
TURNS = list(hc.TURNS) + [("png_encode", 0)]
# the arguments a method writes in place: their result is checked in the placed tensor itself
IN_PLACE = {("overlay_draw", 0), ("board_detect_records", 1), ("cnn_regions_records", 1)}
# capi wants all of these methods' arrays in one memory space: the arguments whose turn it is not lie in HBM too, at offset 0
ONE_SPACE = ("cnn_set_weights", "train_create", "jpeg_reconstruct", "contour_stones")
# every capi.Context method with an `out=` parameter: the element type it writes, the rows that serve
OUT = dict(i420_to_bgr=U8, jpeg_decode=U8, jpeg_reconstruct=U8, jpeg_forward=I16, png_decode=U8, pyr_down=U8, warp_perspective=U8,
           augment_patches=U8)
OUT_ROWS = dict(i420_to_bgr=("i420_to_bgr", "i420_to_bgr_levels", "i420_to_bgr 6x10"), jpeg_decode=("jpeg_decode_host", "jpeg_decode_device", "jpeg_decode_device_spans"),
                jpeg_reconstruct=("jpeg_reconstruct", "jpeg_reconstruct 16x18"), jpeg_forward=("jpeg_forward", "jpeg_forward 16x22"),
                png_decode=("png_decode_host", "png_decode_device"), pyr_down=("pyr_down", "pyr_down 66x264"),
                warp_perspective=("warp_perspective", "warp_perspective dsize 7"), augment_patches=("augment_patches",))
OUT_NEEDS_DEVICE_INPUT = ("warp_perspective",)       # "out must live where the frames live"
C_EDGES = ("ck_board_edges", "ck_goban_canny", "ck_canny")

# The alignments the library insists on: (capi method, argument, C entry point, C argument, bytes, message).  The argument
# is the index of tests/handover_cases.py, "out" for an `out=`, or None where no capi call can reach the refusal (capi
# allocates that output itself); include/camkifu_amd.h, "Alignment of device memory", lists the same, entry for entry,
# and tests/test_gpu_arg_contract.py has a case for each.
REFUSALS = (
    ("jpeg_reconstruct", 0, "ck_jpeg_reconstruct", "coef", 16, "coefficients and quant tables must lie on 16 bytes"),
    ("jpeg_reconstruct", 1, "ck_jpeg_reconstruct", "quant", 16, "coefficients and quant tables must lie on 16 bytes"),
    ("jpeg_coefficients_device", None, "ck_jpeg_coefficients_device", "coef", 16, "coefficients and quant tables must lie on 16 bytes"),
    ("jpeg_coefficients_device", None, "ck_jpeg_coefficients_device", "quant", 16, "coefficients and quant tables must lie on 16 bytes"),
    ("jpeg_forward", "out", "ck_jpeg_forward", "coef", 16, "coefficients must lie on 16 bytes"),
    ("jpeg_entropy_encode_device", 0, "ck_jpeg_entropy_encode_device", "coef", 16, "coefficients must lie on 16 bytes"),
    ("harvest_patches", 0, "ck_harvest_patches", "goban", 4, "goban images in device memory must be 4-byte aligned"),
    ("harvest_patches", None, "ck_harvest_patches", "x", 8, "x in device memory must be 8-byte aligned, src 4-byte aligned"),
    ("harvest_patches", None, "ck_harvest_patches", "src", 4, "x in device memory must be 8-byte aligned, src 4-byte aligned"),
    ("augment_patches", 0, "ck_augment_patches", "x", 4, "patches in device memory must be 4-byte aligned"),
    ("augment_patches", "out", "ck_augment_patches", "x_out", 4, "patches in device memory must be 4-byte aligned"),
    ("board_detect_records", 1, "ck_board_detect_records", "rec", 8, "records must be 8-byte aligned"),
    ("cnn_regions_records", 1, "ck_cnn_regions_records", "rec", 8, "records must be 8-byte aligned"),
)


def _size_of(method, arg):
    return np.dtype(OUT[method] if arg == "out" else ARGS[method][arg]).itemsize


# (method, argument, offset) -> the fragment of the message: the ONLY way a call may pass without matching its reference
ALLOWED = {(m, a, off): msg for m, a, _, _, align, msg in REFUSALS if a is not None
           for off in OFFSETS[_size_of(m, a)] if off % align}


def offsets_of(method, arg):
    return OFFSETS[_size_of(method, arg)]


def shared_offsets(method):
    """the offsets every device-capable argument of `method` can take: those of its largest element type"""
    return OFFSETS[max(np.dtype(t).itemsize for t in ARGS[method])]


# ------------------------------------------------------------------------------------------------ rows on shapes of their own
MT = 48                                  # k_median.hip: a workgroup's tile of medians
NMS_TW, NMS_TH = 64, 28                  # k_canny.hip: a tile of the NMS kernel


def median_interior_tiles(h, w, k):
    """tiles (ty, tx) that take the wide loads of median_mfma_kernel: `ox >= HK && ox - HK + 65 < w && oy >= HK && oy - HK + 63 < h`"""
    hk = k // 2
    return [(ty, tx) for ty in range((h + MT - 1) // MT) for tx in range((w + MT - 1) // MT)
            if tx * MT >= hk and tx * MT - hk + 65 < w and ty * MT >= hk and ty * MT - hk + 63 < h]


def flat_nms_tiles(frame, reach):
    """NMS tiles (ty, tx) that k_canny.hip skips with its dword stores: every median tile under the tile's pixel region
    (2-pixel halo) spans no level at all, which holds where the frame is constant under those tiles and `reach` pixels round
    them (the halo of the medians in front) -- hi == lo, so `6 * (hi - lo) <= low` for any threshold low >= 0"""
    h, w = frame.shape[:2]
    out = []
    for ty in range((h + NMS_TH - 1) // NMS_TH):
        for tx in range((w + NMS_TW - 1) // NMS_TW):
            xa, xb = max(tx * NMS_TW - 2, 0) // MT, min(tx * NMS_TW + NMS_TW + 1, w - 1) // MT
            ya, yb = max(ty * NMS_TH - 2, 0) // MT, min(ty * NMS_TH + NMS_TH + 1, h - 1) // MT
            part = frame[max(ya * MT - reach, 0):(yb + 1) * MT + reach, max(xa * MT - reach, 0):(xb + 1) * MT + reach]
            if (part == part[0, 0]).all():
                out.append((ty, tx))
    return out


def flat_tile_frames():
    """two 120 x 200 frames that are one level except for a block of strong steps in the lower right corner: the NMS tiles of
    the upper left are flat, w % 4 == 0 and h * w % 4 == 0 (so `idx & 3 == 0` holds for every dword of a row)"""
    rng = np.random.default_rng(61)
    frames = np.empty((2, 120, 200, 3), np.uint8)
    for f in range(2):
        frames[f] = 100 + 20 * f
        frames[f, 76:112, 150:190] = rng.integers(0, 2, (36, 40, 1)) * 120 + 40          # a texture of strong steps
        frames[f, 84:104, 160:180, f] = 230
    return frames


class Row(sc.Row):
    """a row on a shape of this file's own: args (the device-capable arguments), run(c, place=None, **kw), check(got),
    reaches() (asserts that the input takes the path the row is named for), expect() (the plain reference's answer)"""

    def __init__(self, name, args, call, want, compare, reaches):
        self.args = tuple(args)
        self.reaches = reaches
        self.expect = lambda: sc.expected("align " + name, want)
        sc.Row.__init__(self, name, lambda c, place=None, **kw: call(c, sc.placed(self.args, place), **kw),
                        lambda got: compare(got, self.expect()), None)


def own_rows(ora):
    """-> {method: [Row]}: needs no GPU (the references and the oracle run on the CPU)"""
    from camkifu_amd import capi
    from tests import board_ref as BR
    from tests import filter_ref as fr
    from tests import jpeg_enc_ref as jenc
    from tests import jpeg_ref
    from tests import pyr_cases
    from tests import pyr_ref
    T = {}

    def add(method, name, args, call, want, compare, reaches):
        assert len(args) == len(ARGS[method])
        T.setdefault(method, []).append(Row(name, args, call, want, compare, reaches))

    def eq(what):
        return lambda got, want: sc._eq(got, want, what)

    # ---- K1: an interior tile, rows of whole dwords and rows that are not
    for k, method, shapes in ((15, "median15", ((108, 108), (108, 110))), (5, "median", ((110, 112), (110, 114)))):
        for j, (h, w) in enumerate(shapes):
            frames = hc._noise(70 + k + j, (1, h, w, 3))

            def reaches(h=h, w=w, k=k, j=j):
                hmin, wmin = MT - k // 2 + 64, MT - k // 2 + 66                  # the kernel's condition for tile (1, 1)
                assert median_interior_tiles(h, w, k) == [(1, 1)] and (w % 4 == 0) == (j == 0)
                assert not median_interior_tiles(hmin - 1, w, k) and not median_interior_tiles(h, wmin - 1, k)
                # the smallest such frame with rows of whole dwords, and one width off a dword (median15: 108 x 108, three
                # rows and one column above the least, as the rows of whole dwords were asked for at 108)
                assert (h, w) == ((108, 108 + 2 * j) if k == 15 else (hmin, -(-wmin // 4) * 4 + 2 * j))
            add(method, "%s %dx%d" % (method, h, w), [frames],
                (lambda c, x, k=k: c.median15(x[0])) if k == 15 else (lambda c, x, k=k: c.median(x[0], k)),
                lambda frames=frames, k=k: np.stack([fr.median(f, k) for f in frames]), eq("%s %dx%d" % (method, h, w)), reaches)

    # ---- K2 behind K1: flat tiles, skipped with dword stores
    flat = flat_tile_frames()

    def flat_reaches(reach, medians):
        def reaches():
            n, h, w, _ = flat.shape
            assert w % 4 == 0 and (h * w) % 4 == 0
            for k in medians:                                                       # the medians in front take their wide loads too
                assert median_interior_tiles(h, w, k) and not median_interior_tiles(96, 128, k), k
            for f in flat:
                tiles = flat_nms_tiles(f, reach)
                assert (0, 0) in tiles and len(tiles) < ((h + NMS_TH - 1) // NMS_TH) * ((w + NMS_TW - 1) // NMS_TW)    # flat tiles and others
        return reaches

    def cmp_edges(what):
        def compare(got, want):
            for j, wj in enumerate(want):
                sc._eq(sc._np(got)[j], wj["edges"], "%s frame %d" % (what, j))
        return compare
    add("board_edges", "board_edges flat tiles", [flat], lambda c, x: c.board_edges(x[0]), lambda: [fr.board_edges(f) for f in flat],
        cmp_edges("board_edges flat tiles"), flat_reaches(7, (15,)))

    def cmp_goban_canny(got, want):
        edges, otsu = got
        for j, wj in enumerate(want):
            assert otsu[j] == wj["otsu"], ("goban_canny flat tiles", j, otsu[j], wj["otsu"])
            sc._eq(sc._np(edges)[j], wj["edges"], "goban_canny flat tiles frame %d" % j)
    add("goban_canny", "goban_canny flat tiles", [flat], lambda c, x: list(c.goban_canny(x[0], want_otsu=True)),
        lambda: [fr.goban_canny(f) for f in flat], cmp_goban_canny, flat_reaches(6 + 3, (13, 7)))

    def cmp_detect(got, want):
        res, lines = got
        for j, ref in enumerate(want):
            r = res[j]
            out = dict(status=int(r["status"]), n_contours=int(r["n_contours"]), n_lines=int(r["n_lines"]),
                       biggest_area=float(r["biggest_area"]), lines=lines[j, :min(int(r["n_lines"]), lines.shape[1])])
            assert out["n_contours"] == ref["n_contours"] and out["status"] == ref["status"], ("board_detect flat tiles", j)
            if ref["status"] != BR.NO_CONTOUR:
                assert abs(out["biggest_area"] - ref["biggest_area"]) <= 1e-5 * max(1.0, ref["biggest_area"]), j
                assert out["n_lines"] == len(ref["lines"]) and np.array_equal(out["lines"], ref["lines"][:len(out["lines"])]), j
    add("board_detect", "board_detect flat tiles", [flat], lambda c, x: list(c.board_detect(x[0], raw=True)),
        lambda: [BR.board_lines(fr.board_edges(f)["edges"]) for f in flat], cmp_detect, flat_reaches(7, (15,)))

    # ---- frame source
    i420 = hc._noise(80, (2, 6 * 10 * 3 // 2))

    def narrow_i420():
        assert 10 % 4 != 0 and (16 * 24 * 3 // 2) % 4 == 0 and 24 % 4 == 0          # (the handover input, 16 x 24, takes the wide form)
    add("i420_to_bgr", "i420_to_bgr 6x10", [i420], lambda c, x, **kw: c.i420_to_bgr(x[0], 6, 10, **kw),
        lambda: np.stack([ora.i420_to_bgr(f, 6, 10) for f in i420]), eq("i420_to_bgr 6x10"), narrow_i420)
    case = pyr_cases.BY_NAME["noise 66x264"]
    interior = case["make"]()[None]

    def pyr_reaches():
        assert interior.shape[1:3] == pyr_cases.SMALLEST_INTERIOR and pyr_cases.interior_tiles(66, 264) == [(1, 1)]
        case["prop"](interior[0])
    add("pyr_down", "pyr_down 66x264", [interior], lambda c, x, **kw: c.pyr_down(x[0], 1, **kw),
        lambda: pyr_ref.pyr_down_batch(interior, 1), eq("pyr_down 66x264"), pyr_reaches)
    small = hc._noise(1, (2, 16, 24, 3))

    def warp_reaches():
        assert (3 * 8) % 4 == 0 and (3 * 7) % 4 != 0                                # (dsize 8: the handover input)
    add("warp_perspective", "warp_perspective dsize 7", [small], lambda c, x, **kw: c.warp_perspective(x[0], hc.M_SMALL, dsize=7, **kw),
        lambda: np.stack([ora.warp_perspective(f, hc.M_SMALL, (7, 7)) for f in small]), eq("warp_perspective dsize 7"), warp_reaches)

    # ---- JPEG: a width that is no multiple of 4 (the handover inputs are 16 and 24 wide)
    odd = hc._noise(81, (2, 16, 22, 3))
    q90 = jenc.quant_tables(90)
    assert capi.CK_JPEG_420 == jenc.S420

    def not_wide(w):
        def reaches():
            assert w % 4 != 0 and 16 % 4 == 0 and 24 % 4 == 0
        return reaches
    add("jpeg_forward", "jpeg_forward 16x22", [odd], lambda c, x, **kw: c.jpeg_forward(x[0], q90, capi.CK_JPEG_420, **kw),
        lambda: np.stack([jenc.forward(f, q90, jenc.S420) for f in odd]), eq("jpeg_forward 16x22"), not_wide(22))

    def cmp_streams(got, want):
        assert list(got) == list(want), "jpeg_encode 16x22"
    add("jpeg_encode", "jpeg_encode 16x22", [odd], lambda c, x: c.jpeg_encode(x[0], quality=85, restart_interval=1),
        lambda: [jenc.encode(f, 85, jenc.S420, 1) for f in odd], cmp_streams, not_wide(22))
    frames18 = hc._noise(82, (2, 16, 18, 3)) // 4 + 90
    parts = [jpeg_ref.coefficients(jenc.encode(f, 80, jenc.S420, 0)) for f in frames18]
    coef18 = np.stack([p[1] for p in parts]).astype(np.int16)
    quant18 = np.stack([p[2] for p in parts]).astype(np.uint16)
    add("jpeg_reconstruct", "jpeg_reconstruct 16x18", [coef18, quant18],
        lambda c, x, **kw: c.jpeg_reconstruct(x[0], x[1], 16, 18, capi.CK_JPEG_420, **kw),
        lambda: np.stack([jpeg_ref.reconstruct(coef18[f], quant18[f], 16, 18, jenc.S420) for f in range(2)]), eq("jpeg_reconstruct 16x18"),
        not_wide(18))
    return T


OWN = dict(median15=("median15 108x108", "median15 108x110"), median=("median 110x112", "median 110x114"),
           board_edges=("board_edges flat tiles",), goban_canny=("goban_canny flat tiles",), board_detect=("board_detect flat tiles",),
           i420_to_bgr=("i420_to_bgr 6x10",), pyr_down=("pyr_down 66x264",), warp_perspective=("warp_perspective dsize 7",),
           jpeg_forward=("jpeg_forward 16x22",), jpeg_encode=("jpeg_encode 16x22",), jpeg_reconstruct=("jpeg_reconstruct 16x18",))
ROWS_OF = {m: (m,) + OWN.get(m, ()) for m in hc.METHODS}       # the method's row of tests/scratch_cases.py first (the handover input)
ROWS_OF["png_encode"] = ("png_encode", "png_encode_runs")


def rows(ck, ora):
    """-> {name: row} of every row the alignment tests run: the table of tests/scratch_cases.py and the rows of this file"""
    table = dict(sc.build(ck, ora))
    own = own_rows(ora)
    assert {m: tuple(r.name for r in v) for m, v in own.items()} == OWN
    for v in own.values():
        for r in v:
            assert r.name not in table
            table[r.name] = r
    return table

"""What tests/test_gpu_scratch.py needs: a table of every capi.Context method that runs kernels.  A row has

    run(c)      the case: the smallest input at which the entry point's kernels still take their ordinary paths (the inputs of
                tests/handover_cases.py where they serve: 16 x 24 and 96 x 128 frames, one 380 x 380 goban, n <= 3)
    check(got)  the result against the expected value, which comes from the plain reference the entry point's own test file
                uses, never from the library; it is computed once per process and left unchanged
    grow(c)     the same entry point on at least twice the frames (and a larger image where it takes a shape): it only
                leaves the context's buffers larger than the case needs

run takes two things more, for tests/test_gpu_alignment.py: `place`, a function (k, array) -> what the call gets in place of
argument k of the method's device-capable arguments (numbered as in tests/handover_cases.py; None: the arrays themselves),
and keywords such as `out=` for the methods that take them.  The rows of HOST_STREAM_ROWS that decode or inflate take
host streams only: they have no device-capable argument and never call `place` (jpeg_decode_*, jpeg_coefficients_device,
png_decode_*, png_inflate_device); the three further jpeg_encode rows keep their frames in host memory.

Methods with state: a MOG2 row's case feeds ONE model a long run and then a short one and is compared over the whole
history; a trainer row takes a fresh handle per run; the cluster row resets the generator.  The classifier rows run the
exact network "gather" of tests/cnn_exact_cases.py, whose answer is the same bits in every mode, and go through all four
modes; the rows that classify a warped frame (stones_detect, stones_run) use its weights too: every layer of that network
hands single pixel values on, so its sums are exact for any 8-bit image and the float64 model is the one right answer."""
import functools
import zlib

import numpy as np

from tests import handover_cases as hc

FILL_BYTES = (0x00, 0xFF, 0x55)
_expected = {}


def expected(name, make):
    """the expected value of a row, computed once"""
    if name not in _expected:
        _expected[name] = make()
    return _expected[name]


class Row:
    def __init__(self, name, run, check, grow):
        self.name, self.run, self.check, self.grow = name, run, check, grow


def placed(args, place):
    """the device-capable arguments of a call as `place` hands them over (None: as they are)"""
    return list(args) if place is None else [place(k, a) for k, a in enumerate(args)]


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _eq(got, want, what):
    got = _np(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    assert np.array_equal(got, want), "%s: %d of %d elements differ" % (what, int((got != want).sum()), want.size)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def big_frames():
    return hc._noise(31, (4, 144, 200, 3))


def _edge_maps(n, h, w, seed):
    """edge maps for a grow call: a few outlines and 2 % of single pixels"""
    rng = np.random.default_rng(seed)
    e = ((rng.random((n, h, w)) < 0.02) * 255).astype(np.uint8)
    for f in range(n):
        for k in range(3):
            y0, x0 = 4 + 9 * k + f, 6 + 11 * k
            e[f, y0, x0:w - x0] = e[f, h - y0, x0:w - x0] = 255
            e[f, y0:h - y0 + 1, x0] = e[f, y0:h - y0 + 1, w - x0 - 1] = 255
    return e


# ------------------------------------------------------------------------------------------------ the exact network
MODES = ("f16x2", "fp32", "bf16", "f16q8")


def _mode(name):
    from camkifu_amd import capi
    return {"f16x2": capi.CK_CNN_F16X2, "fp32": capi.CK_CNN_FP32, "bf16": capi.CK_CNN_BF16, "f16q8": capi.CK_CNN_F16Q8}[name]


@functools.lru_cache(maxsize=None)
def exact_net():
    from tests import cnn_exact_cases as ec
    c = ec.case("gather")
    assert c["agree"] and set(c["modes"]) == set(MODES)
    return c["W"], c["gobans"]


def exact_answer(name, gobans):
    """the float64 model of the exact network on `gobans` (its bits are those of every mode) -> dict of read-only arrays"""
    from tests import cnn_mode_ref as mr

    def make():
        o = mr.forward(exact_net()[0], gobans, "f16x2")
        lab, conf, stones, conf19 = mr.decode(o["y"])
        assert np.array_equal(lab, o["logits"].argmax(-1))
        o = dict(o, labels=lab, stones=stones)
        for v in o.values():
            v.setflags(write=False)
        return o
    return expected(name, make)


def in_every_mode(c, call):
    """call() under each classifier mode in turn -> {mode: result}; the context is back in its default mode afterwards"""
    from camkifu_amd import capi
    out = {}
    try:
        for m in MODES:
            c.cnn_set_mode(_mode(m))
            out[m] = call()
    finally:
        c.cnn_set_mode(capi.CK_CNN_DEFAULT)
    return out


def check_y(y, ref, what):
    """y against the float64 model within cnn_exact_cases.Y_EXACT, as tests/test_gpu_cnn_exact.py holds it"""
    from tests import cnn_exact_cases as ec
    gap = float(np.abs(_np(y).astype(np.float64) - ref["y"]).max())
    assert gap <= ec.Y_EXACT, (what, gap)


def check_conf(conf, y, what, grid=False):
    """confidences against decode_kernel's rule applied to the library's own y (float64, index order), bit for bit"""
    from tests import cnn_mode_ref as mr
    _, c100, _, c19 = mr.decode(_np(y))
    want = np.ascontiguousarray(c19 if grid else c100)
    assert np.array_equal(np.ascontiguousarray(_np(conf)).reshape(want.shape).view(np.uint64), want.view(np.uint64)), what


# ------------------------------------------------------------------------------------------------ the table
def build(ck, ora):
    """-> {name: Row}.  `ck` serves tests/handover_cases.build, which derives a few INPUTS with it (edge maps, JPEG
    coefficients); no expected value comes from it.  `ora`: the oracle, for the two entry points whose own tests have no
    plain reference (the I420 conversion, the warp)."""
    from camkifu_amd import capi
    from camkifu_amd.core import overlay
    from tests import board_ref as BR
    from tests import cluster_cases as cc
    from tests import cluster_ref as cr
    from tests import filter_ref as fr
    from tests import harvest_ref as hr
    from tests import jpeg_enc_opt_ref as jopt
    from tests import jpeg_enc_ref as jenc
    from tests import jpeg_ref
    from tests import mog2_scenes as ms
    from tests import overlay_ref
    from tests import png_cases
    from tests import png_ref
    from tests import pyr_ref
    from tests import stone_cases as K
    from tests import stone_ref as SR
    from tests import train_cases as tc
    from tests import train_ref as tr
    H = hc.build(ck)
    T = {}
    big = big_frames()

    def add(name, run, check, grow):
        assert name not in T
        T[name] = Row(name, run, check, grow)

    def of(name):
        """the handover case `name` on its content A"""
        return lambda c, place=None, **kw: H[name].run(c, placed(H[name].a, place), **kw)

    def grown(name, *args):
        """the handover case's call on other arguments"""
        return lambda c: H[name].run(c, args)

    def frames_of(name):
        return H[name].a[0]

    # ---- K1, K2 -------------------------------------------------------------------------------------------------------
    def per_frame(name, ref):
        return expected(name, lambda: [ref(f) for f in frames_of(name)])

    def check_median(name, k):
        def check(got):
            _eq(got, np.stack(per_frame(name, lambda f: fr.median(f, k))), name)
        return check
    add("median15", of("median15"), check_median("median15", 15), grown("median15", big))
    add("median", of("median"), check_median("median", 5), grown("median", big))

    def check_goban_canny(got):
        edges, otsu = got
        for j, w in enumerate(per_frame("goban_canny", fr.goban_canny)):
            assert otsu[j] == w["otsu"], ("goban_canny", j, otsu[j], w["otsu"])
            _eq(_np(edges)[j], w["edges"], "goban_canny frame %d" % j)
    add("goban_canny", of("goban_canny"), check_goban_canny, grown("goban_canny", big))

    def check_canny(got):
        edges, m = got
        for j, w in enumerate(per_frame("canny", lambda f: fr.canny(f, 25, 75))):
            _eq(_np(m)[j], w["map"], "canny map %d" % j)
            _eq(_np(edges)[j], w["edges"], "canny edges %d" % j)
    add("canny", of("canny"), check_canny, grown("canny", big))

    def check_board_edges(got):
        for j, w in enumerate(per_frame("board_edges", fr.board_edges)):
            _eq(_np(got)[j], w["edges"], "board_edges frame %d" % j)
    add("board_edges", of("board_edges"), check_board_edges, grown("board_edges", big))

    # ---- K3 .. K6 -----------------------------------------------------------------------------------------------------
    def check_board(out, ghost, ref, what):
        """one frame against board_ref.board_lines, as tests/test_gpu_board_lines.py::_check holds it"""
        assert out["n_contours"] == ref["n_contours"] and out["status"] == ref["status"], what
        if ref["status"] == BR.NO_CONTOUR:
            return
        assert abs(out["biggest_area"] - ref["biggest_area"]) <= 1e-5 * max(1.0, ref["biggest_area"]), what
        if ghost is not None:
            _eq(ghost, ref["ghost"], what + " ghost")
        assert out["n_lines"] == len(ref["lines"]), what
        assert np.array_equal(out["lines"], ref["lines"][:len(out["lines"])]), what

    def check_board_lines(got):
        out, ghost = got
        for j, ref in enumerate(per_frame("board_lines", BR.board_lines)):
            check_board(out[j], _np(ghost)[j], ref, "board_lines frame %d" % j)
    add("board_lines", of("board_lines"), check_board_lines, grown("board_lines", _edge_maps(4, 144, 200, 5)))

    def detect_refs(name):
        return expected(name, lambda: [BR.board_lines(fr.board_edges(f)["edges"]) for f in frames_of(name)])

    def check_board_detect(got):
        res, lines = got
        for j, ref in enumerate(detect_refs("board_detect")):
            r = res[j]
            out = dict(status=int(r["status"]), n_contours=int(r["n_contours"]), n_lines=int(r["n_lines"]),
                       biggest_area=float(r["biggest_area"]), lines=lines[j, :min(int(r["n_lines"]), lines.shape[1])])
            assert int(r["reserved"]) == 0
            check_board(out, None, ref, "board_detect frame %d" % j)
    add("board_detect", of("board_detect"), check_board_detect, grown("board_detect", big))

    def check_board_records(got):
        rec = _np(got).view(capi.REC_DTYPE).reshape(-1)
        for j, ref in enumerate(detect_refs("board_detect_records")):
            r = rec[j]
            kept = min(int(r["n_lines"]), capi.REC_LMAX)
            out = dict(status=int(r["status"]), n_contours=int(r["n_contours"]), n_lines=int(r["n_lines"]),
                       biggest_area=float(r["biggest_area"]), lines=r["lines"][:kept])
            check_board(out, None, ref, "board_detect_records frame %d" % j)
            assert int(r["flags"]) == (capi.REC_LINES_CUT if int(r["n_lines"]) > capi.REC_LMAX else 0)
            assert not r["lines"][kept:].any()
            # the stones half stays as the caller left it
            assert (r["region_label"] == 0xEE).all() and (r["region_conf"].view(np.uint8) == 0xEE).all() and (r["pad"] == 0xEE).all()
    add("board_detect_records", of("board_detect_records"), check_board_records,
        lambda c: c.board_detect_records(big, np.zeros(4, capi.REC_DTYPE)))

    # ---- frame source -------------------------------------------------------------------------------------------------
    def i420_frames():
        return expected("i420 frames", lambda: np.stack([ora.i420_to_bgr(f, 16, 24) for f in frames_of("i420_to_bgr")]))
    big_i420 = hc._noise(32, (4, 48 * 64 * 3 // 2))
    add("i420_to_bgr", of("i420_to_bgr"), lambda got: _eq(got, i420_frames(), "i420_to_bgr"),
        lambda c: c.i420_to_bgr(big_i420, 48, 64))
    assert np.array_equal(frames_of("i420_to_bgr"), frames_of("i420_to_bgr_levels"))
    add("i420_to_bgr_levels", of("i420_to_bgr_levels"),
        lambda got: _eq(got, expected("i420 levels", lambda: pyr_ref.pyr_down_batch(i420_frames(), 1)), "i420_to_bgr levels=1"),
        lambda c: c.i420_to_bgr(big_i420, 48, 64, levels=2))
    add("pyr_down", of("pyr_down"), lambda got: _eq(got, expected("pyr_down", lambda: pyr_ref.pyr_down_batch(frames_of("pyr_down"), 1)), "pyr_down"),
        lambda c: c.pyr_down(big, 3))
    add("warp_perspective", of("warp_perspective"),
        lambda got: _eq(got, expected("warp", lambda: np.stack([ora.warp_perspective(f, hc.M_SMALL, (8, 8)) for f in frames_of("warp_perspective")])),
                        "warp_perspective"),
        lambda c: c.warp_perspective(big, hc.M_BOARD, dsize=64))

    # ---- JPEG ---------------------------------------------------------------------------------------------------------
    coef_a, quant_a = H["jpeg_reconstruct"].a
    add("jpeg_reconstruct", of("jpeg_reconstruct"),
        lambda got: _eq(got, expected("jpeg_reconstruct", lambda: np.stack([jpeg_ref.reconstruct(coef_a[f], quant_a[f], 16, 16, jenc.S420)
                                                                            for f in range(len(coef_a))])), "jpeg_reconstruct"),
        lambda c: c.jpeg_reconstruct(*big_coefficients(), 48, 64, capi.CK_JPEG_420))
    q90, q85 = jenc.quant_tables(90), jenc.quant_tables(85)
    assert capi.CK_JPEG_420 == jenc.S420

    @functools.lru_cache(maxsize=None)
    def big_jpeg():
        frames = hc._noise(33, (4, 48, 64, 3)) // 4 + 90
        return frames, [jenc.encode(f, 80, jenc.S420, 2) for f in frames]

    @functools.lru_cache(maxsize=None)
    def big_coefficients():
        parts = [jpeg_ref.coefficients(s) for s in big_jpeg()[1]]
        return (np.stack([p[1] for p in parts]).astype(np.int16), np.stack([p[2] for p in parts]).astype(np.uint16))
    add("jpeg_forward", of("jpeg_forward"),
        lambda got: _eq(got, expected("jpeg_forward", lambda: np.stack([jenc.forward(f, q90, jenc.S420) for f in frames_of("jpeg_forward")])), "jpeg_forward"),
        lambda c: c.jpeg_forward(big, q90, capi.CK_JPEG_444))

    def encode_row(name, tables, entropy):
        ref = jopt if tables == "optimised" else jenc

        def run(c, place=None):
            c.jpeg_set_encode_entropy(entropy)
            try:
                return c.jpeg_encode(placed([frames_of("jpeg_encode")], place)[0], quality=85, restart_interval=1, optimize=tables == "optimised")
            finally:
                c.jpeg_set_encode_entropy("host")

        def grow(c):
            c.jpeg_set_encode_entropy(entropy)
            try:
                c.jpeg_encode(big, quality=70, sampling=capi.CK_JPEG_422, optimize=tables == "optimised")
            finally:
                c.jpeg_set_encode_entropy("host")

        def check(got):
            want = expected("jpeg_encode " + tables, lambda: [ref.encode(f, 85, jenc.S420, 1) for f in frames_of("jpeg_encode")])
            assert got == want, name
        add(name, run, check, grow)
    encode_row("jpeg_encode", "standard", "host")
    encode_row("jpeg_encode_optimised", "optimised", "host")
    encode_row("jpeg_encode_device", "standard", "device")
    encode_row("jpeg_encode_optimised_device", "optimised", "device")
    add("jpeg_entropy_encode_device", of("jpeg_entropy_encode_device"),
        lambda got: _eq_list(got, expected("entropy_encode", lambda: [jenc.entropy_encode(cf, q90, 16, 16, jenc.S420) for cf in coef_a]),
                             "jpeg_entropy_encode_device"),
        lambda c: c.jpeg_entropy_encode_device(big_coefficients()[0], q85, 48, 64, capi.CK_JPEG_420, restart_interval=3))

    def _eq_list(got, want, what):
        assert list(got) == list(want), what

    @functools.lru_cache(maxsize=None)
    def small_jpeg():
        """two 24 x 40 frames in restart intervals of 2 MCUs: six strands a frame, strands of several spans at 8 bytes a span"""
        frames = hc._noise(34, (2, 24, 40, 3))
        return [jenc.encode(f, 90, jenc.S420, 2) for f in frames]

    def decode_row(mode):
        def run(c, place=None, **kw):
            c.jpeg_set_entropy(mode)
            if mode == "device-spans":
                c.jpeg_set_span_bytes(8)
            try:
                return c.jpeg_decode(small_jpeg(), **kw)
            finally:
                c.jpeg_set_entropy("host")

        def grow(c):
            c.jpeg_set_entropy(mode)
            try:
                c.jpeg_decode(big_jpeg()[1])
            finally:
                c.jpeg_set_entropy("host")
        add("jpeg_decode_" + mode.replace("-", "_"), run,
            lambda got: _eq(got, expected("jpeg_decode", lambda: np.stack([jpeg_ref.decode(s) for s in small_jpeg()])), "jpeg_decode " + mode), grow)
    for mode in ("host", "device", "device-spans"):
        decode_row(mode)

    def check_coefficients(got):
        info, coef, quant = got
        want = expected("jpeg_coefficients", lambda: [jpeg_ref.coefficients(s) for s in small_jpeg()])
        assert (info["h"], info["w"], info["sampling"], info["restart_interval"]) == (24, 40, capi.CK_JPEG_420, 2)
        for f, (_, cf, q) in enumerate(want):
            _eq(coef[f], np.asarray(cf, np.int16), "coefficients of frame %d" % f)
            _eq(quant[f], np.asarray(q, np.uint16), "quant tables of frame %d" % f)
    add("jpeg_coefficients_device", lambda c, place=None: c.jpeg_coefficients_device(small_jpeg()), check_coefficients,
        lambda c: c.jpeg_coefficients_device(big_jpeg()[1]))

    # ---- PNG ----------------------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def small_png():
        """16 x 24 files of three colour types (palette, 16-bit grey + alpha, RGB), every filter type in use"""
        return [png_cases.image(24, 16, ct, d, seed=k) for k, (ct, d) in enumerate(((3, 4), (4, 16), (2, 8)))]

    @functools.lru_cache(maxsize=None)
    def big_png():
        return [png_cases.image(200, 144, ct, d, seed=10 + k, smooth=True)[0] for k, (ct, d) in enumerate(((2, 8), (6, 8), (0, 8), (2, 16), (3, 8), (2, 8)))]

    def png_decode_row(inflate):
        def check(got):
            for f, (data, bgr) in enumerate(small_png()):
                assert np.array_equal(png_ref.decode(data), bgr)           # (the two statements of the reference agree)
                _eq(_np(got)[f], bgr, "png_decode %s frame %d" % (inflate, f))
        add("png_decode_" + inflate, lambda c, place=None, **kw: c.png_decode([d for d, _ in small_png()], inflate=inflate, **kw), check,
            lambda c: c.png_decode(big_png(), inflate=inflate))
    png_decode_row("host")
    png_decode_row("device")

    @functools.lru_cache(maxsize=None)
    def png_frames():
        f = hc._noise(35, (2, 16, 24, 3))
        f[1, 4:12, 3:20] = 7                                       # runs of equal bytes for the runs mode
        g = big_frames() // 32 * 32
        return f, g

    def png_encode_row(runs):
        name = "png_encode_runs" if runs else "png_encode"
        add(name, lambda c, place=None: c.png_encode(placed([png_frames()[0]], place)[0], runs=runs),
            lambda got: _eq_list(got, expected(name, lambda: capi.png_encode_staged(png_frames()[0], None, runs=runs)), name),
            lambda c: c.png_encode(png_frames()[1], runs=runs))
    png_encode_row(False)
    png_encode_row(True)

    @functools.lru_cache(maxsize=None)
    def z_streams():
        rng = np.random.default_rng(36)
        small = [bytes(rng.integers(0, 4, 700, dtype=np.uint8)), b"go " * 300, bytes(rng.integers(0, 256, 90, dtype=np.uint8))]
        large = [bytes(rng.integers(0, 8, 40000, dtype=np.uint8)) for _ in range(6)]
        return small, [zlib.compress(b, 9) for b in small], [zlib.compress(b, 6) for b in large]

    def check_inflate(got):
        for f, (r, want) in enumerate(zip(got, z_streams()[0])):
            assert (r["cause"], r["total"], r["produced"]) == (0, len(want), len(want)) and r["data"] == want, ("png_inflate_device", f)
    add("png_inflate_device", lambda c, place=None: c.png_inflate_device(z_streams()[1]), check_inflate, lambda c: c.png_inflate_device(z_streams()[2]))

    # ---- overlays ------------------------------------------------------------------------------------------------------
    def check_overlay(got):
        def make():
            dl = overlay.DisplayList().disc(8, 6, 3).segment(1, 1, 20, 12)
            prims, start, text = overlay.pack([dl, dl])
            glyphs = np.stack([capi.overlay_glyph(ch) for ch in range(32, 127)])
            return overlay_ref.paint(frames_of("overlay_draw"), prims, start, text, glyphs)[0]
        _eq(got, expected("overlay_draw", make), "overlay_draw")
    big_dl = overlay.DisplayList().rect(5, 5, 150, 100, (10, 200, 30), thickness=2).text(8, 8, "scratch", (255, 255, 255)).disc(100, 70, 30, 77)
    add("overlay_draw", of("overlay_draw"), check_overlay, lambda c: c.overlay_draw(big.copy(), [big_dl] * 4))

    # ---- K9: one model, a long run and then a short one ------------------------------------------------------------------
    def mog2_row(name, h, w, last_band):
        # the mosaic of tests/mog2_scenes.py under the automatic rate and then the product's two rates.  (With a rate of 0.2
        # or above among the first frames the oracle and mog2_scenes.reference part by one ulp in a weight -- the masks stay
        # equal -- and the library sides with the oracle: docs/lab_notes.md, note 18.  Not a matter of scratch: left out.)
        frames = ms.mosaic(h, w, range(7), seed=37)
        rates = [-1.0, -1.0, -1.0, 0.01, 0.01, 0.005, 0.005]
        long_run, short_run = slice(0, 5), slice(5, 7)

        def counts_of(mask):
            m = (mask != 0).astype(np.int32)
            m[:, w - 1] = 0
            if last_band:
                m[h - 1, :] = 0
            return m.reshape(h // 20, 20, w // 20, 20).sum((1, 3), dtype=np.int32)

        def run(c, place=None):
            def put(a):
                return placed([np.ascontiguousarray(a)], place)[0]
            hd = c.mog2_create(h, w)
            try:
                if name == "mog2_apply":
                    got = [_np(c.mog2_apply(hd, put(frames[t]), rates[t])) for t in range(7)]
                else:
                    got = list(_np(c.mog2_band_run(hd, put(frames[long_run]), rates[long_run], last_band))) + \
                        list(_np(c.mog2_band_run(hd, put(frames[short_run]), rates[short_run], last_band)))
                return got, c.mog2_state(hd)
            finally:
                c.mog2_destroy(hd)

        def check(got):
            masks, state = expected(name, lambda: ms.reference(list(frames), rates, return_state=True))
            for t in range(7):
                _eq(got[0][t], np.asarray(masks[t], np.uint8) if name == "mog2_apply" else counts_of(np.asarray(masks[t])), "%s frame %d" % (name, t))
            assert ms.state_mismatch(got[1], state) is None, (name, ms.state_mismatch(got[1], state))

        def grow(c):
            hd = c.mog2_create(2 * h, w)
            try:
                more = hc._noise(39, (14, 2 * h, w, 3))
                if name == "mog2_apply":
                    for f in more[:2]:
                        c.mog2_apply(hd, f, 0.01)
                else:
                    c.mog2_band_run(hd, more, [0.01] * 14, last_band)
            finally:
                c.mog2_destroy(hd)
        add(name, run, check, grow)
    mog2_row("mog2_apply", 20, 40, False)
    mog2_row("mog2_band_run", 20, 380, True)
    masks = H["zone_counts"].a[0]
    add("zone_counts", of("zone_counts"), lambda got: _eq(got, expected("zone_counts", lambda: ms.zone_counts(masks)), "zone_counts"),
        lambda c: c.zone_counts(np.stack([masks, masks[::-1].copy(), masks[:, ::-1].copy()])))

    # ---- K10 .. K12: the exact network, every mode --------------------------------------------------------------------------
    W, gather = exact_net()
    more_gobans = np.concatenate([gather, hc._noise(40, (2, 380, 380, 3)) // 64])

    def with_exact(call, gobans=gather):
        def run(c, place=None):
            c.cnn_set_weights(W)
            g = placed([gobans], place)[0]
            return in_every_mode(c, lambda: call(c, g))
        return run

    def check_modes(check_one):
        def check(got):
            assert sorted(got) == sorted(MODES)
            for m in MODES:
                check_one(got[m], exact_answer("gather", gather), m)
        return check

    def check_predict(got, ref, m):
        y, stones, conf = got
        check_y(y, ref, "cnn_predict " + m)
        _eq(stones, ref["stones"], "cnn_predict stones " + m)
        check_conf(conf, y, "cnn_predict conf " + m, grid=True)
    add("cnn_predict", with_exact(lambda c, g: c.cnn_predict(g)), check_modes(check_predict), with_exact(lambda c, g: c.cnn_predict(g), more_gobans))

    def check_maps(got, ref, m):
        for k, a in zip(("pool2", "pool4"), got):
            assert np.array_equal(a.view(np.uint32), _bits(ref[k])), "cnn_maps %s %s: %d elements differ" % (k, m, int((a.view(np.uint32) != _bits(ref[k])).sum()))
    add("cnn_maps", with_exact(lambda c, g: c.cnn_maps(g)), check_modes(check_maps), with_exact(lambda c, g: c.cnn_maps(g), more_gobans))

    def check_regions(got, ref, m):
        # the confidences follow from y, which this call does not return: a cnn_predict of the same mode gives it
        rl, rc, y = got
        _eq(_np(rl).reshape(1, 100), ref["labels"], "cnn_regions labels " + m)
        check_y(y, ref, "cnn_regions y " + m)
        check_conf(rc, y, "cnn_regions conf " + m)
    add("cnn_regions", with_exact(lambda c, g: tuple(c.cnn_regions(g)) + (c.cnn_predict(g)[0],)), check_modes(check_regions),
        with_exact(lambda c, g: c.cnn_regions(g), more_gobans))

    def run_set_weights(c, place=None):
        c.cnn_set_weights(hc.weights(2))                           # another network first: every pack is written again
        c.cnn_set_weights(dict(zip(capi.WEIGHT_ORDER, placed([W[k] for k in capi.WEIGHT_ORDER], place))))
        return in_every_mode(c, lambda: tuple(c.cnn_regions(gather)) + (c.cnn_predict(gather)[0],))
    add("cnn_set_weights", run_set_weights, check_modes(check_regions), lambda c: c.cnn_set_weights(hc.weights(3)))

    def run_region_records(c, place=None):
        c.cnn_set_weights(W)
        rec = np.full((1, capi.REC_BYTES), 0xEE, np.uint8)
        g = placed([gather], place)[0]

        def call():
            rows = rec.copy() if place is None else place(1, rec.copy())       # (a buffer of its own for every mode)
            rows = rows.view(capi.REC_DTYPE).reshape(1) if isinstance(rows, np.ndarray) else rows
            got = c.cnn_regions_records(g, rows)
            assert got is rows
            return _np(got).view(capi.REC_DTYPE).reshape(1), c.cnn_predict(g)[0]
        return in_every_mode(c, call)

    def check_region_records(got, ref, m):
        rec, y = got
        _eq(rec["region_label"].reshape(1, 100), ref["labels"], "cnn_regions_records labels " + m)
        check_y(y, ref, "cnn_regions_records y " + m)
        check_conf(rec["region_conf"], y, "cnn_regions_records conf " + m)
        part = np.ascontiguousarray(rec).view(np.uint8).reshape(-1)[:capi.REC_DTYPE.fields["region_conf"][1]]
        assert (part == 0xEE).all() and (rec["pad"] == 0xEE).all()                 # the board half stays as the caller left it
    add("cnn_regions_records", run_region_records, check_modes(check_region_records),
        with_exact(lambda c, g: c.cnn_regions_records(g, np.zeros(3, capi.REC_DTYPE)), more_gobans))

    # ---- the stones path on frames: the warp, then the exact network (and a background model) -------------------------------
    scenes = frames_of("stones_detect")

    def warped_answer():
        gobans = expected("warped gobans", lambda: np.stack([ora.warp_perspective(f, hc.M_BOARD, (380, 380)) for f in scenes]))
        return gobans, exact_answer("warped", gobans)

    def run_stones_detect(c, place=None):
        c.cnn_set_weights(W)
        s = placed([scenes], place)[0]
        return c.stones_detect(s, hc.M_BOARD), c.cnn_predict(c.warp_perspective(s, hc.M_BOARD))[0]

    def check_stones_detect(got):
        (labels, conf), y = got
        ref = warped_answer()[1]
        _eq(labels, ref["stones"], "stones_detect")
        check_y(y, ref, "stones_detect y")
        check_conf(conf, y, "stones_detect conf", grid=True)

    def grow_stones(c):
        c.cnn_set_weights(W)
        c.stones_detect(big, hc.M_BOARD)
    add("stones_detect", run_stones_detect, check_stones_detect, grow_stones)

    def run_stones_run(c, place=None):
        c.cnn_set_weights(W)
        s = placed([scenes], place)[0]
        hd = c.mog2_create(380, 380)
        try:
            return (c.stones_run(s, hc.M_BOARD, want_grid=True), c.stones_run(s, hc.M_BOARD, mog2=hd, learning_rates=[-1.0, 0.05]),
                    c.cnn_predict(c.warp_perspective(s, hc.M_BOARD))[0])
        finally:
            c.mog2_destroy(hd)

    def check_stones_run(got):
        plain, with_bg, y = got
        gobans, ref = warped_answer()
        for out in (plain, with_bg):
            _eq(_np(out["region_label"]).reshape(2, 100), ref["labels"], "stones_run labels")
            check_conf(out["region_conf"], y, "stones_run conf")
        check_y(y, ref, "stones_run y")
        _eq(plain["labels"], ref["stones"], "stones_run grid")
        check_conf(plain["conf"], y, "stones_run grid conf", grid=True)
        assert plain["fgcount"] is None
        # the background model has seen the two gobans in order: the oracle's mask of each, counted per zone
        def counts():
            model = ora.MOG2(380, 380, 3)
            return np.stack([ms.zone_counts(model.apply(g, r)) for g, r in zip(gobans, (-1.0, 0.05))])
        _eq(with_bg["fgcount"], expected("stones_run fgcount", counts), "stones_run fgcount")

    def grow_stones_run(c):
        c.cnn_set_weights(W)
        hd = c.mog2_create(380, 380)
        try:
            c.stones_run(big, hc.M_BOARD, mog2=hd, learning_rates=[-1.0] * 4, want_grid=True)
        finally:
            c.mog2_destroy(hd)
    add("stones_run", run_stones_run, check_stones_run, grow_stones_run)

    # ---- the trainer: a fresh handle per run ------------------------------------------------------------------------------
    x3, y3 = tc.cases()["n3"]
    x65, y65 = tc.cases()["n65"]
    W0 = tc.weights()

    def on_trainer(call, args=(), create_placed=False):
        """call(c, hd, *args as `place` hands them over); create_placed: the trainer's own weights are the arguments"""
        def run(c, place=None):
            a = placed(args, place)
            hd = c.train_create(dict(zip(tr.ORDER, a)) if create_placed else W0)
            try:
                return call(c, hd) if create_placed else call(c, hd, *a)
            finally:
                c.train_destroy(hd)
        return run

    def check_grads(got):
        from tests.test_gpu_train import TOL
        loss, grads, masks = got
        l_ref, g_ref = tc.reference("n3")
        assert masks is None and abs(loss - l_ref) / abs(l_ref) <= TOL, ("train_grads", loss, l_ref)
        for k, e in tr.grad_error(grads, g_ref).items():
            assert e <= TOL, ("train_grads", k, e)
    add("train_grads", on_trainer(lambda c, hd, x: c.train_grads(hd, x, y3, dropout=False), [x3]), check_grads,
        on_trainer(lambda c, hd: c.train_grads(hd, x65, y65, dropout=True, seed=3)))

    def run_step(c, hd, x):
        _, grads, _ = c.train_grads(hd, x, y3, dropout=False)
        loss = c.train_step(hd, x, y3, lr=0.001, dropout=False)
        return loss, grads, c.train_weights(hd), c.train_adam_state(hd)

    def check_adam(w, m, v, steps, grads, what):
        """one update from the float32 gradients the library computed: tests/test_gpu_train.py::test_adam_alone's bounds"""
        ref = tr.Adam(W0, state=np.float32)
        ref.apply(grads, lr=0.001)
        assert steps == 1
        for k in tr.ORDER:
            assert tr.ulps(w[k], ref.w[k]).max() <= 2, (what, k)
            assert tr.ulps(m[k], ref.m[k]).max() <= 1 and tr.ulps(v[k], ref.v[k]).max() <= 1, (what, k)

    def check_step(got):
        loss, grads, w, (m, v, steps) = got
        check_grads((loss, grads, None))
        check_adam(w, m, v, steps, grads, "train_step")
    add("train_step", on_trainer(run_step, [x3]), check_step, on_trainer(lambda c, hd: c.train_step(hd, x65, y65, dropout=True, seed=4)))
    given = {k: (np.random.default_rng(41 + i).standard_normal(W0[k].shape) * 1e-2).astype(np.float32) for i, k in enumerate(tr.ORDER)}

    def run_apply(c, hd, *grads):
        c.train_apply(hd, dict(zip(tr.ORDER, grads)), lr=0.001)
        return c.train_weights(hd), c.train_adam_state(hd)
    add("train_apply", on_trainer(run_apply, [given[k] for k in tr.ORDER]), lambda got: check_adam(got[0], got[1][0], got[1][1], got[1][2], given, "train_apply"),
        on_trainer(lambda c, hd: c.train_grads(hd, x65, y65)))

    def check_create(got):
        for k in tr.ORDER:
            assert np.array_equal(_bits(got[k]), _bits(W0[k])), ("train_create", k)
    add("train_create", on_trainer(lambda c, hd: c.train_weights(hd), [W0[k] for k in tr.ORDER], create_placed=True), check_create, on_trainer(lambda c, hd: c.train_grads(hd, x65, y65)))

    # ---- training data ------------------------------------------------------------------------------------------------------
    goban_h, calm_h = H["harvest_patches"].a
    pos = ((hc._rng(8).random((1, 19, 19)) < 0.45) * hc._rng(9).integers(1, 3, (1, 19, 19))).astype(np.uint8)     # (handover_cases' positions)

    def check_harvest(got):
        x, labels, src, found = got
        rx, rl, rs, n = expected("harvest", lambda: hr.harvest_ref(goban_h, calm_h, [0], pos))
        _eq(x, rx, "harvest x")
        _eq(labels, rl, "harvest labels")
        _eq(src, rs, "harvest src")
        assert found == n > 0

    def grow_harvest(c):
        g = hr.hashed_bytes((3, 380, 380, 3), salt=5)
        c.harvest_patches(g, np.zeros((3, 19, 19), np.int32), [0, 0, 0], pos)
    add("harvest_patches", of("harvest_patches"), check_harvest, grow_harvest)
    codes = np.array([1, 6, 3], np.uint8)
    add("augment_patches", of("augment_patches"),
        lambda got: _eq(got, expected("augment", lambda: hr.augment_ref(H["augment_patches"].a[0], codes)), "augment_patches"),
        lambda c: c.augment_patches(x65, np.arange(65) % 8))

    # ---- the stones finders on goban images -----------------------------------------------------------------------------------
    rects = K.zones_of(K.posgrid())
    board, fg = H["contour_stones"].a

    def check_contour_stones(got):
        stones, zones, mask = got
        ref = expected("contour_stones", lambda: SR.find_stones(board, fg, rects))
        _eq(mask, ref["mask"], "contour_stones mask")
        _eq(zones, ref["zones"], "contour_stones zones")
        _eq(stones, ref["stones"], "contour_stones stones")
    add("contour_stones", of("contour_stones"), check_contour_stones,
        lambda c: c.contour_stones(np.stack([board, K.stone_board(7)]), np.stack([fg, fg[::-1].copy()]), rects))
    c16 = next(c for c in cc.cases() if c[0] == "sized16")
    imgs16, rects16, jobs16 = c16[1], c16[2], c16[3][[2, 4]]            # 1024 pixels (resident) and 20736 (streaming)
    mask16 = cr.circle_mask(rects16, cc.SIDE)
    whole = next(c for c in cc.cases() if c[0] == "columns")

    def run_cluster(c, place=None):
        c.rng_state = 0xffffffff
        return c.cluster_stones(placed([imgs16], place)[0], rects16, mask16, jobs=jobs16, want_all=True), c.rng_state

    def check_cluster(got):
        from tests.test_gpu_cluster import _same
        want, state = expected("cluster", lambda: cc.reference(imgs16, rects16, mask16, jobs16))
        _same(got[0], want)
        assert got[1] == state

    def grow_cluster(c):
        c.cluster_stones(whole[1], whole[2], cr.circle_mask(whole[2], cc.SIDE), jobs=np.concatenate([whole[3], whole[3]]))
    add("cluster_stones", run_cluster, check_cluster, grow_cluster)
    maps = H["contours_external"].a[0]

    def check_contours(got):
        ref = expected("contours", lambda: [SR.follow_contours(e) for e in maps])
        assert len(got) == len(ref)
        for f, (g_map, r_map) in enumerate(zip(got, ref)):
            assert [(k["start"], k["nvert"]) for k in g_map] == [(k["start"], k["nvert"]) for k in r_map], ("contours_external", f)
            for g, r in zip(g_map, r_map):
                pix = set(map(tuple, g["pix"].tolist()))
                assert len(pix) == len(g["pix"]) and pix == r["pix"], ("contours_external", f, r["start"])
    add("contours_external", lambda c, place=None: c.contours_external(placed([maps], place)[0], want_points=True), check_contours,
        lambda c: c.contours_external(_edge_maps(4, 144, 200, 6), want_points=True))
    # the goban image of tests/handover_cases.py under noise of +-10 levels: on the synthetic images of tests/stone_cases.py
    # every gradient is far from both thresholds and Canny's map is the same at any Otsu level; here a level one off moves
    # more than a thousand edge pixels, so the histogram behind the level is held too
    gimg = np.clip(H["find_intersections"].a[0].astype(np.int16) + hc._rng(50).integers(-10, 11, (380, 380, 3)), 0, 255).astype(np.uint8)
    mtx = K.posgrid()

    def check_grid(got):
        grid, found, edges = got
        ref = expected("find_intersections", lambda: SR.find_intersections(gimg, mtx, rects))
        _eq(edges, ref["edges"], "find_intersections edges")
        for key in sorted(set(found) | set(ref["found"])):
            assert found.get(key) == ref["found"].get(key), ("find_intersections", key)
        _eq(grid, ref["grid"], "find_intersections grid")
    add("find_intersections", lambda c, place=None: c.find_intersections(placed([gimg], place)[0], mtx, rects, want_lines=True), check_grid,
        lambda c: c.find_intersections(np.stack([gimg, K.goban_image(3, 4), gimg[::-1].copy()]), mtx, rects))
    return T


# every capi.Context method that runs kernels: the 37 of tests/handover_cases.METHODS and the ones that take host streams only
HOST_STREAM_ROWS = ("jpeg_decode_host", "jpeg_decode_device", "jpeg_decode_device_spans", "jpeg_coefficients_device", "png_decode_host",
                    "png_decode_device", "png_encode", "png_encode_runs", "jpeg_encode_optimised", "jpeg_encode_device",
                    "jpeg_encode_optimised_device", "png_inflate_device")
NAMES = tuple(hc.METHODS) + HOST_STREAM_ROWS

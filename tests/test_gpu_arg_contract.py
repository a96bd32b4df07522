"""The argument contract of the C ABI (camkifu_amd/csrc/ck_api.hip, ck_api_jpeg.hip, ck_api_png.hip): one case per distinct refusal that an entry point
makes before it launches anything -- the error number and a fragment of the message ck_last_error gives.  The calls go
through ctypes directly, past the checks of capi.Context.  Every pointer that is not NULL points at a buffer large
enough for the shapes used (2 frames of 8 x 8), so no case hands a kernel a bad pointer even if a check were lost; an
invalid OUTPUT space is not tested for that reason (the library treats it as device memory, unchecked).

The refusals by ALIGNMENT (include/camkifu_amd.h, "Alignment of device memory"; tests/align_cases.REFUSALS) follow the same rule:
the pointer that is off points into a 1 MiB block of device memory of this file's own, so a lost check hands the kernel a
valid, merely misaligned pointer."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 4            # CK_ERR_ARG, CK_ERR_STATE
HOST, DEV = 0, 1
BAD_SPACE = 7
S444 = 1                     # CK_JPEG_444 (Env asserts it)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Env:
    """one context without classifier weights, a live 40 x 60 MOG2 model, a destroyed one, a live trainer, a destroyed one"""

    def __init__(self):
        from camkifu_amd import capi
        self.L = capi.lib()
        self.ck = capi.Context(0)
        self.h = self.ck._h
        rng = np.random.default_rng(11)
        self.buf = rng.integers(0, 256, 1 << 20, dtype=np.uint8)          # input of any small case
        self.out = np.zeros(1 << 20, np.uint8)                            # output of any small case
        self.goban = rng.integers(0, 256, (1, 380, 380, 3), dtype=np.uint8)
        self.M = np.tile(np.eye(3).reshape(1, 9), (3, 1))
        self.rects = np.zeros((19, 19, 4), np.int32)
        self.mog = self.ck.mog2_create(40, 60)
        self.mog_dead = self.ck.mog2_create(40, 60)
        self.ck.mog2_destroy(self.mog_dead)
        w = {k: (rng.standard_normal(capi.WEIGHT_SHAPES[k]) * 0.05).astype(np.float32) for k in capi.WEIGHT_ORDER}
        self.wptr = (C.c_void_p * 12)(*(_p(w[k]) for k in capi.WEIGHT_ORDER))
        self.wptr_hole = (C.c_void_p * 12)(*(_p(w[k]) if i != 5 else None for i, k in enumerate(capi.WEIGHT_ORDER)))
        self.keep = w
        self.tr = self.ck.train_create(w)
        self.tr_dead = self.ck.train_create(w)
        self.ck.train_destroy(self.tr_dead)
        self.patches = rng.integers(0, 256, (2, 40, 40, 3), dtype=np.uint8)
        self.lab = np.array([3, 80], np.uint8)
        self.lab_bad = np.array([3, 81], np.uint8)
        # ---- for the refusals by alignment: device memory of this file's own, and valid arguments around the pointer that is off
        import torch
        assert capi.CK_JPEG_444 == S444
        self.dev_in = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
        self.dev_out = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
        assert self.dev_in.data_ptr() % 16 == 0 and self.dev_out.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        self.quant = np.ascontiguousarray(capi.jpeg_quant(90), np.uint16)
        self.jpeg_ptrs, self.jpeg_lens, self.jpeg_keep = capi._jpeg_streams([bytes(64), bytes(64)])
        self.jpeg_geom = capi.JpegInfo(8, 8, S444, 0, capi.jpeg_blocks(8, 8, S444))
        self.jpeg_stride = capi.jpeg_encode_bound(8, 8, S444)
        self.jpeg_len = (C.c_size_t * 2)()
        self.fg = np.zeros((1, 361), np.int32)
        self.state_of = np.zeros(1, np.int32)
        self.positions = np.zeros((1, 361), np.uint8)
        self.found = C.c_int32(0)
        self.codes = np.array([1, 6], np.uint8)
        self.ck_net = capi.Context(0)                                     # a second context WITH weights: the records of the classifier
        self.ck_net.cnn_set_weights(w)

    def close(self):
        self.ck_net.close()
        self.ck.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def _img_cases():
    """(name, call, code, fragment): call(e) -> the entry point's return value"""
    c = []
    add = lambda name, fn, code, frag: c.append((name, fn, code, frag))
    I = lambda e: _p(e.buf)
    O = lambda e: _p(e.out)
    # ---- check_img, through ck_median -------------------------------------------------------------------------------
    add("null_ctx", lambda e: e.L.ck_median(None, I(e), 2, 8, 8, 15, HOST, O(e), HOST), ARG, None)
    add("median_in_null", lambda e: e.L.ck_median(e.h, None, 2, 8, 8, 15, HOST, O(e), HOST), ARG, "image pointer is NULL")
    add("median_n0", lambda e: e.L.ck_median(e.h, I(e), 0, 8, 8, 15, HOST, O(e), HOST), ARG, "bad shape n=0 h=8 w=8")
    add("median_h0", lambda e: e.L.ck_median(e.h, I(e), 2, 0, 8, 15, HOST, O(e), HOST), ARG, "bad shape n=2 h=0 w=8")
    add("median_w_neg", lambda e: e.L.ck_median(e.h, I(e), 2, 8, -1, 15, HOST, O(e), HOST), ARG, "bad shape n=2 h=8 w=-1")
    add("median_too_large", lambda e: e.L.ck_median(e.h, I(e), 1, 32768, 16384, 15, HOST, O(e), HOST), ARG, "image too large")
    add("median_out_null", lambda e: e.L.ck_median(e.h, I(e), 2, 8, 8, 15, HOST, None, HOST), ARG, "out is NULL")
    add("median_window_4", lambda e: e.L.ck_median(e.h, I(e), 2, 8, 8, 4, HOST, O(e), HOST), ARG, "median window 4: odd sizes 3..17 only")
    add("median_window_19", lambda e: e.L.ck_median(e.h, I(e), 2, 8, 8, 19, HOST, O(e), HOST), ARG, "median window 19: odd sizes 3..17 only")
    add("median_in_space_7", lambda e: e.L.ck_median(e.h, I(e), 2, 8, 8, 15, BAD_SPACE, O(e), HOST), ARG, "bad memory space 7")
    add("median15_out_null", lambda e: e.L.ck_median15(e.h, I(e), 2, 8, 8, HOST, None, HOST), ARG, "out is NULL")
    # ---- Canny, edges, lines ----------------------------------------------------------------------------------------
    add("canny_edges_null", lambda e: e.L.ck_canny(e.h, I(e), 2, 8, 8, HOST, 25, 75, None, None, HOST), ARG, "edges is NULL")
    add("canny_in_null", lambda e: e.L.ck_canny(e.h, None, 2, 8, 8, HOST, 25, 75, O(e), None, HOST), ARG, "image pointer is NULL")
    add("canny_in_space_7", lambda e: e.L.ck_canny(e.h, I(e), 2, 8, 8, BAD_SPACE, 25, 75, O(e), None, HOST), ARG, "bad memory space 7")
    add("goban_canny_edges_null", lambda e: e.L.ck_goban_canny(e.h, I(e), 2, 8, 8, HOST, None, HOST, None), ARG, "edges is NULL")
    add("goban_canny_n0", lambda e: e.L.ck_goban_canny(e.h, I(e), 0, 8, 8, HOST, O(e), HOST, None), ARG, "bad shape n=0")
    add("board_edges_null", lambda e: e.L.ck_board_edges(e.h, I(e), 2, 8, 8, HOST, None, HOST), ARG, "edges is NULL")
    add("board_edges_in_space_7", lambda e: e.L.ck_board_edges(e.h, I(e), 2, 8, 8, BAD_SPACE, O(e), HOST), ARG, "bad memory space 7")
    add("board_lines_lines_null", lambda e: e.L.ck_board_lines(e.h, I(e), 2, 8, 8, HOST, -1, None, 16, O(e), None, HOST), ARG, "lines/res NULL or cap <= 0")
    add("board_lines_cap0", lambda e: e.L.ck_board_lines(e.h, I(e), 2, 8, 8, HOST, -1, O(e), 0, O(e), None, HOST), ARG, "lines/res NULL or cap <= 0")
    add("board_lines_2x8", lambda e: e.L.ck_board_lines(e.h, I(e), 2, 2, 8, HOST, -1, O(e), 16, O(e), None, HOST), ARG, "image smaller than 3x3")
    add("board_lines_in_space_7", lambda e: e.L.ck_board_lines(e.h, I(e), 2, 8, 8, BAD_SPACE, -1, O(e), 16, O(e), None, HOST), ARG, "bad memory space 7")
    add("board_detect_res_null", lambda e: e.L.ck_board_detect(e.h, I(e), 2, 8, 8, HOST, -1, O(e), 16, None), ARG, "lines/res NULL or cap <= 0")
    add("board_detect_cap_neg", lambda e: e.L.ck_board_detect(e.h, I(e), 2, 8, 8, HOST, -1, O(e), -3, O(e)), ARG, "lines/res NULL or cap <= 0")
    add("board_detect_8x2", lambda e: e.L.ck_board_detect(e.h, I(e), 2, 8, 2, HOST, -1, O(e), 16, O(e)), ARG, "image smaller than 3x3")
    add("board_detect_in_null", lambda e: e.L.ck_board_detect(e.h, None, 2, 8, 8, HOST, -1, O(e), 16, O(e)), ARG, "image pointer is NULL")
    add("board_records_rec_null", lambda e: e.L.ck_board_detect_records(e.h, I(e), 2, 8, 8, HOST, -1, None, HOST), ARG, "rec is NULL")
    add("board_records_space_7", lambda e: e.L.ck_board_detect_records(e.h, I(e), 2, 8, 8, HOST, -1, O(e), BAD_SPACE), ARG, "bad memory space 7")
    # ---- colour conversion and pyramid ------------------------------------------------------------------------------
    add("i420_out_null", lambda e: e.L.ck_i420_to_bgr(e.h, I(e), 2, 8, 8, HOST, None, HOST), ARG, "bgr is NULL")
    add("i420_odd_h", lambda e: e.L.ck_i420_to_bgr(e.h, I(e), 2, 7, 8, HOST, O(e), HOST), ARG, "I420 needs even dimensions, got 8x7")
    add("i420_odd_w", lambda e: e.L.ck_i420_to_bgr(e.h, I(e), 2, 8, 9, HOST, O(e), HOST), ARG, "I420 needs even dimensions, got 9x8")
    add("i420_in_space_7", lambda e: e.L.ck_i420_to_bgr(e.h, I(e), 2, 8, 8, BAD_SPACE, O(e), HOST), ARG, "bad memory space 7")
    add("pyr_in_null", lambda e: e.L.ck_pyr_down(e.h, None, 2, 8, 8, 1, HOST, O(e), HOST), ARG, "image pointer is NULL")
    add("pyr_out_null", lambda e: e.L.ck_pyr_down(e.h, I(e), 2, 8, 8, 1, HOST, None, HOST), ARG, "image pointer is NULL")
    add("pyr_n0", lambda e: e.L.ck_pyr_down(e.h, I(e), 0, 8, 8, 1, HOST, O(e), HOST), ARG, "bad shape n=0 h=8 w=8")
    add("pyr_levels_0", lambda e: e.L.ck_pyr_down(e.h, I(e), 2, 8, 8, 0, HOST, O(e), HOST), ARG, "pyramid levels 0: at least 1")
    add("pyr_levels_too_many", lambda e: e.L.ck_pyr_down(e.h, I(e), 2, 8, 8, 5, HOST, O(e), HOST), ARG, "pyramid level 4 would take a 1x1 image: sides below 2")
    add("pyr_in_space_7", lambda e: e.L.ck_pyr_down(e.h, I(e), 2, 8, 8, 1, BAD_SPACE, O(e), HOST), ARG, "bad memory space 7")
    add("i420_pyr_out_null", lambda e: e.L.ck_i420_to_bgr_pyr(e.h, I(e), 2, 8, 8, 1, HOST, None, HOST), ARG, "image pointer is NULL")
    add("i420_pyr_w0", lambda e: e.L.ck_i420_to_bgr_pyr(e.h, I(e), 2, 8, 0, 1, HOST, O(e), HOST), ARG, "bad shape n=2 h=8 w=0")
    add("i420_pyr_odd", lambda e: e.L.ck_i420_to_bgr_pyr(e.h, I(e), 2, 6, 7, 1, HOST, O(e), HOST), ARG, "I420 needs even dimensions, got 7x6")
    add("i420_pyr_levels_0", lambda e: e.L.ck_i420_to_bgr_pyr(e.h, I(e), 2, 8, 8, 0, HOST, O(e), HOST), ARG, "pyramid levels 0: at least 1")
    add("i420_pyr_levels_too_many", lambda e: e.L.ck_i420_to_bgr_pyr(e.h, I(e), 2, 4, 8, 3, HOST, O(e), HOST), ARG, "pyramid level 3 would take a 2x1 image: sides below 2")
    add("i420_pyr_in_space_7", lambda e: e.L.ck_i420_to_bgr_pyr(e.h, I(e), 2, 8, 8, 1, BAD_SPACE, O(e), HOST), ARG, "bad memory space 7")
    # ---- warp -------------------------------------------------------------------------------------------------------
    add("warp_out_null", lambda e: e.L.ck_warp_perspective(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 1, 8, None, HOST), ARG, "out NULL or dsize <= 0")
    add("warp_dsize_0", lambda e: e.L.ck_warp_perspective(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 1, 0, O(e), HOST), ARG, "out NULL or dsize <= 0")
    add("warp_M_null", lambda e: e.L.ck_warp_perspective(e.h, I(e), 2, 8, 8, HOST, None, 1, 8, O(e), HOST), ARG, "M is NULL")
    add("warp_m_count_3_n_2", lambda e: e.L.ck_warp_perspective(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 3, 8, O(e), HOST), ARG, "m_count must be 1 or n")
    add("warp_in_space_7", lambda e: e.L.ck_warp_perspective(e.h, I(e), 2, 8, 8, BAD_SPACE, _p(e.M), 1, 8, O(e), HOST), ARG, "bad memory space 7")
    add("stones_detect_m_count", lambda e: e.L.ck_stones_detect(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 3, O(e), None, HOST), ARG, "m_count must be 1 or n")
    add("stones_detect_n0", lambda e: e.L.ck_stones_detect(e.h, I(e), 0, 8, 8, HOST, _p(e.M), 1, O(e), None, HOST), ARG, "bad shape n=0")
    return c


def _model_cases():
    c = []
    add = lambda name, fn, code, frag: c.append((name, fn, code, frag))
    I = lambda e: _p(e.buf)
    O = lambda e: _p(e.out)
    G = lambda e: _p(e.goban)
    R = lambda e: _p(e.rects)
    lr = C.c_double(0.01)
    # ---- classifier: arguments, and use before the weights are set (the context of this file never sets them) ----------
    add("set_weights_null", lambda e: e.L.ck_cnn_set_weights(e.h, None, HOST), ARG, None)
    add("set_weights_hole", lambda e: e.L.ck_cnn_set_weights(e.h, e.wptr_hole, HOST), ARG, "weights[5] is NULL")
    add("set_mode_9", lambda e: e.L.ck_cnn_set_mode(e.h, 9), ARG, "unknown cnn mode 9")
    add("predict_null", lambda e: e.L.ck_cnn_predict(e.h, None, 1, HOST, None, O(e), None, HOST), ARG, "goban NULL or n <= 0")
    add("predict_n0", lambda e: e.L.ck_cnn_predict(e.h, G(e), 0, HOST, None, O(e), None, HOST), ARG, "goban NULL or n <= 0")
    add("predict_in_space_7", lambda e: e.L.ck_cnn_predict(e.h, G(e), 1, BAD_SPACE, None, O(e), None, HOST), ARG, "bad memory space 7")
    add("predict_before_weights", lambda e: e.L.ck_cnn_predict(e.h, G(e), 1, HOST, None, O(e), None, HOST), STATE, "ck_cnn_set_weights has not been called")
    add("maps_n_129", lambda e: e.L.ck_cnn_maps(e.h, G(e), 129, HOST, None, None), ARG, "goban NULL or n outside 1 .. 128")
    add("maps_before_weights", lambda e: e.L.ck_cnn_maps(e.h, G(e), 1, HOST, None, None), STATE, "ck_cnn_set_weights has not been called")
    add("regions_label_null", lambda e: e.L.ck_cnn_regions(e.h, G(e), 1, HOST, None, O(e), HOST), ARG, "NULL argument or n <= 0")
    add("regions_n_neg", lambda e: e.L.ck_cnn_regions(e.h, G(e), -1, HOST, O(e), O(e), HOST), ARG, "NULL argument or n <= 0")
    add("regions_before_weights", lambda e: e.L.ck_cnn_regions(e.h, G(e), 1, HOST, O(e), O(e), HOST), STATE, "ck_cnn_set_weights has not been called")
    add("regions_records_rec_null", lambda e: e.L.ck_cnn_regions_records(e.h, G(e), 1, HOST, None, HOST), ARG, "NULL argument or n <= 0")
    add("regions_records_space_7", lambda e: e.L.ck_cnn_regions_records(e.h, G(e), 1, HOST, O(e), BAD_SPACE), ARG, "bad memory space 7")
    add("regions_records_before_weights", lambda e: e.L.ck_cnn_regions_records(e.h, G(e), 1, HOST, O(e), HOST), STATE, "ck_cnn_set_weights has not been called")
    # ---- ordered stones run and the MOG2 handles -----------------------------------------------------------------------
    add("stones_run_regions_null", lambda e: e.L.ck_stones_run(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 1, -1, None, None, O(e), None, None, None, HOST), ARG, "region outputs are NULL")
    add("stones_run_bad_handle", lambda e: e.L.ck_stones_run(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 1, 99, _p(e.M), O(e), O(e), O(e), None, None, HOST), ARG, "bad mog2 handle 99")
    add("stones_run_dead_handle", lambda e: e.L.ck_stones_run(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 1, e.mog_dead, _p(e.M), O(e), O(e), O(e), None, None, HOST), ARG, "bad mog2 handle %d")
    add("stones_run_rates_null", lambda e: e.L.ck_stones_run(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 1, e.mog, None, O(e), O(e), O(e), None, None, HOST), ARG, "a background model needs learning_rates and fgcount")
    add("stones_run_fgcount_null", lambda e: e.L.ck_stones_run(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 1, e.mog, _p(e.M), O(e), O(e), None, None, None, HOST), ARG, "a background model needs learning_rates and fgcount")
    add("stones_run_model_40x60", lambda e: e.L.ck_stones_run(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 1, e.mog, _p(e.M), O(e), O(e), O(e), None, None, HOST), ARG, "the background model of a stones run is 380x380")
    add("stones_run_m_count", lambda e: e.L.ck_stones_run(e.h, I(e), 2, 8, 8, HOST, _p(e.M), 3, -1, None, O(e), O(e), None, None, None, HOST), ARG, "m_count must be 1 or n")
    add("mog2_create_h0", lambda e: e.L.ck_mog2_create(e.h, 0, 60, C.byref(C.c_int(0))), ARG, None)
    add("mog2_create_w_neg", lambda e: e.L.ck_mog2_create(e.h, 40, -2, C.byref(C.c_int(0))), ARG, None)
    add("mog2_create_handle_null", lambda e: e.L.ck_mog2_create(e.h, 40, 60, None), ARG, None)
    add("mog2_apply_bad_handle", lambda e: e.L.ck_mog2_apply(e.h, -1, I(e), HOST, lr, O(e), HOST), ARG, "bad mog2 handle -1")
    add("mog2_apply_past_the_end", lambda e: e.L.ck_mog2_apply(e.h, 64, I(e), HOST, lr, O(e), HOST), ARG, "bad mog2 handle 64")
    add("mog2_apply_after_destroy", lambda e: e.L.ck_mog2_apply(e.h, e.mog_dead, I(e), HOST, lr, O(e), HOST), ARG, "bad mog2 handle %d")
    add("mog2_apply_null", lambda e: e.L.ck_mog2_apply(e.h, e.mog, None, HOST, lr, O(e), HOST), ARG, "NULL image or mask")
    add("mog2_apply_mask_null", lambda e: e.L.ck_mog2_apply(e.h, e.mog, I(e), HOST, lr, None, HOST), ARG, "NULL image or mask")
    add("mog2_apply_in_space_7", lambda e: e.L.ck_mog2_apply(e.h, e.mog, I(e), BAD_SPACE, lr, O(e), HOST), ARG, "bad memory space 7")
    add("mog2_state_bad_handle", lambda e: e.L.ck_mog2_get_state(e.h, 99, None, None, None, None), ARG, "bad mog2 handle 99")
    add("mog2_state_after_destroy", lambda e: e.L.ck_mog2_get_state(e.h, e.mog_dead, None, None, None, None), ARG, "bad mog2 handle %d")
    add("mog2_destroy_bad_handle", lambda e: e.L.ck_mog2_destroy(e.h, 99), ARG, None)
    add("band_run_bad_handle", lambda e: e.L.ck_mog2_band_run(e.h, 99, I(e), 2, HOST, _p(e.M), 0, O(e), HOST), ARG, "bad mog2 handle 99")
    add("band_run_after_destroy", lambda e: e.L.ck_mog2_band_run(e.h, e.mog_dead, I(e), 2, HOST, _p(e.M), 0, O(e), HOST), ARG, "bad mog2 handle %d")
    add("band_run_rates_null", lambda e: e.L.ck_mog2_band_run(e.h, e.mog, I(e), 2, HOST, None, 0, O(e), HOST), ARG, "NULL argument or n <= 0")
    add("band_run_n0", lambda e: e.L.ck_mog2_band_run(e.h, e.mog, I(e), 0, HOST, _p(e.M), 0, O(e), HOST), ARG, "NULL argument or n <= 0")
    add("band_run_in_space_7", lambda e: e.L.ck_mog2_band_run(e.h, e.mog, I(e), 2, BAD_SPACE, _p(e.M), 0, O(e), HOST), ARG, "bad memory space 7")
    add("zone_counts_null", lambda e: e.L.ck_zone_counts(e.h, None, 1, HOST, O(e), HOST), ARG, "NULL argument or n <= 0")
    add("zone_counts_n0", lambda e: e.L.ck_zone_counts(e.h, I(e), 0, HOST, O(e), HOST), ARG, "NULL argument or n <= 0")
    add("zone_counts_in_space_7", lambda e: e.L.ck_zone_counts(e.h, I(e), 1, BAD_SPACE, O(e), HOST), ARG, "bad memory space 7")
    # ---- the stones finders on goban images ----------------------------------------------------------------------------
    add("contour_stones_null", lambda e: e.L.ck_contour_stones(e.h, G(e), None, 1, 380, HOST, R(e), 0, 19, 0, 19, O(e), None, None), ARG, "NULL argument or n <= 0")
    add("contour_stones_side_50", lambda e: e.L.ck_contour_stones(e.h, G(e), G(e), 1, 50, HOST, R(e), 0, 19, 0, 19, O(e), None, None), ARG, "goban image side 50")
    add("contour_stones_range", lambda e: e.L.ck_contour_stones(e.h, G(e), G(e), 1, 380, HOST, R(e), 5, 5, 0, 20, O(e), None, None), ARG, "intersection range rows [5, 5) columns [0, 20)")
    add("contour_stones_range_neg", lambda e: e.L.ck_contour_stones(e.h, G(e), G(e), 1, 380, HOST, R(e), -1, 19, 0, 19, O(e), None, None), ARG, "intersection range rows [-1, 19) columns [0, 19)")
    add("cluster_stones_no_job", lambda e: e.L.ck_cluster_stones(e.h, G(e), 1, 380, 0, HOST, R(e), I(e), I(e), 0, O(e), O(e), None, None, None, 0, None, None, None), ARG, "NULL argument, n <= 0 or no job")
    add("cluster_stones_mask_null", lambda e: e.L.ck_cluster_stones(e.h, G(e), 1, 380, 0, HOST, R(e), None, I(e), 1, O(e), O(e), None, None, None, 0, None, None, None), ARG, "NULL argument, n <= 0 or no job")
    add("cluster_stones_side_50", lambda e: e.L.ck_cluster_stones(e.h, G(e), 1, 50, 0, HOST, R(e), I(e), I(e), 1, O(e), O(e), None, None, None, 0, None, None, None), ARG, "goban image side 50")
    add("rng_get_null", lambda e: e.L.ck_rng_get(e.h, None), ARG, "state is NULL")
    add("contours_table_null", lambda e: e.L.ck_contours_external(e.h, I(e), 2, 8, 8, HOST, O(e), None, 16, None, 0), ARG, "NULL table")
    add("contours_table_cap_0", lambda e: e.L.ck_contours_external(e.h, I(e), 2, 8, 8, HOST, O(e), O(e), 0, None, 0), ARG, "NULL table")
    add("contours_h0", lambda e: e.L.ck_contours_external(e.h, I(e), 2, 0, 8, HOST, O(e), O(e), 16, None, 0), ARG, "bad shape n=2 h=0 w=8")
    add("intersections_grid_null", lambda e: e.L.ck_find_intersections(e.h, G(e), 1, 380, HOST, I(e), R(e), None, None, None, None), ARG, "NULL argument or n <= 0")
    add("intersections_side_50", lambda e: e.L.ck_find_intersections(e.h, G(e), 1, 50, HOST, I(e), R(e), O(e), None, None, None), ARG, "goban image side 50")
    add("intersections_side_5000", lambda e: e.L.ck_find_intersections(e.h, G(e), 1, 5000, HOST, I(e), R(e), O(e), None, None, None), ARG, "goban image side 5000")
    # ---- trainers ------------------------------------------------------------------------------------------------------
    P = lambda e: _p(e.patches)
    loss = C.c_float(0)
    step = lambda e, hd, x, lab, n, h, w, ch, sp: e.L.ck_train_step(e.h, hd, x, lab, n, h, w, ch, sp, 0.001, 0, 0, C.byref(loss))
    add("train_create_null", lambda e: e.L.ck_train_create(e.h, None, HOST, C.byref(C.c_int(0))), ARG, None)
    add("train_create_handle_null", lambda e: e.L.ck_train_create(e.h, e.wptr, HOST, None), ARG, None)
    add("train_create_hole", lambda e: e.L.ck_train_create(e.h, e.wptr_hole, HOST, C.byref(C.c_int(0))), ARG, "weights[5] is NULL")
    add("train_step_bad_handle", lambda e: step(e, 99, P(e), _p(e.lab), 2, 40, 40, 3, HOST), ARG, "bad trainer handle 99")
    add("train_step_neg_handle", lambda e: step(e, -1, P(e), _p(e.lab), 2, 40, 40, 3, HOST), ARG, "bad trainer handle -1")
    add("train_step_after_destroy", lambda e: step(e, e.tr_dead, P(e), _p(e.lab), 2, 40, 40, 3, HOST), ARG, "bad trainer handle %d")
    add("train_step_x_null", lambda e: step(e, e.tr, None, _p(e.lab), 2, 40, 40, 3, HOST), ARG, "patches or labels NULL")
    add("train_step_labels_null", lambda e: step(e, e.tr, P(e), None, 2, 40, 40, 3, HOST), ARG, "patches or labels NULL")
    add("train_step_n0", lambda e: step(e, e.tr, P(e), _p(e.lab), 0, 40, 40, 3, HOST), ARG, "patches of shape 0 x 40 x 40 x 3")
    add("train_step_39", lambda e: step(e, e.tr, P(e), _p(e.lab), 2, 39, 40, 3, HOST), ARG, "patches of shape 2 x 39 x 40 x 3")
    add("train_step_grey", lambda e: step(e, e.tr, P(e), _p(e.lab), 2, 40, 40, 1, HOST), ARG, "patches of shape 2 x 40 x 40 x 1")
    add("train_step_label_81", lambda e: step(e, e.tr, P(e), _p(e.lab_bad), 2, 40, 40, 3, HOST), ARG, "label 81 of patch 1")
    add("train_step_in_space_7", lambda e: step(e, e.tr, P(e), _p(e.lab), 2, 40, 40, 3, BAD_SPACE), ARG, "bad memory space 7")
    add("train_grads_bad_handle", lambda e: e.L.ck_train_grads(e.h, 99, P(e), _p(e.lab), 2, 40, 40, 3, HOST, 0, 0, -1, C.byref(loss), None, None, None, None), ARG, "bad trainer handle 99")
    add("train_apply_bad_handle", lambda e: e.L.ck_train_apply(e.h, 99, e.wptr, 0.001), ARG, "bad trainer handle 99")
    add("train_apply_null", lambda e: e.L.ck_train_apply(e.h, e.tr, None, 0.001), ARG, "grads is NULL")
    add("train_apply_hole", lambda e: e.L.ck_train_apply(e.h, e.tr, e.wptr_hole, 0.001), ARG, "grads[5] is NULL")
    add("train_weights_after_destroy", lambda e: e.L.ck_train_get_weights(e.h, e.tr_dead, None), ARG, "bad trainer handle %d")
    add("train_adam_bad_handle", lambda e: e.L.ck_train_get_adam_state(e.h, 99, None, None, None), ARG, "bad trainer handle 99")
    add("train_handover_bad_handle", lambda e: e.L.ck_train_handover(e.h, 99), ARG, "bad trainer handle 99")
    add("train_destroy_bad_handle", lambda e: e.L.ck_train_destroy(e.h, 99), ARG, "bad trainer handle 99")
    add("train_destroy_twice", lambda e: e.L.ck_train_destroy(e.h, e.tr_dead), ARG, "bad trainer handle %d")
    add("timing_get_name_null", lambda e: e.L.ck_timing_get(e.h, None, None, None), ARG, None)
    add("scratch_fill_null_ctx", lambda e: e.L.ck_debug_scratch_fill(None, 0, None, None), ARG, None)
    add("scratch_fill_byte_256", lambda e: e.L.ck_debug_scratch_fill(e.h, 256, None, None), ARG, "fill byte 256: 0 .. 255")
    add("scratch_fill_byte_neg", lambda e: e.L.ck_debug_scratch_fill(e.h, -1, None, None), ARG, "fill byte -1: 0 .. 255")
    return c


def _din(e, off=0):
    return C.c_void_p(e.dev_in.data_ptr() + off)


def _dout(e, off=0):
    return C.c_void_p(e.dev_out.data_ptr() + off)


def _harvest(e, goban, in_space, x, src, out_space):
    """one goban image, room for two patches; labels at 64 KiB and src from 128 KiB of the output block"""
    labels = _dout(e, 1 << 16) if out_space == DEV else _p(e.out[1 << 16:])
    return e.L.ck_harvest_patches(e.h, goban, 1, in_space, _p(e.fg), HOST, _p(e.state_of), _p(e.positions), 1, 16, 256, 0, 0,
                                  x, labels, src, 2, out_space, C.byref(e.found))


def _alignment_cases():
    """one case per refusal by alignment: everything else about the call is valid"""
    c = []
    add = lambda name, fn, frag: c.append((name, fn, ARG, frag))
    I = lambda e: _p(e.buf)
    O = lambda e: _p(e.out)
    Q = lambda e: _p(e.quant)
    both = "coefficients and quant tables must lie on 16 bytes"
    add("jpeg_reconstruct_coef_off_16", lambda e: e.L.ck_jpeg_reconstruct(e.h, _din(e, 2), _din(e, 1 << 16), 2, 8, 8, S444, DEV, O(e), HOST), both)
    add("jpeg_reconstruct_quant_off_16", lambda e: e.L.ck_jpeg_reconstruct(e.h, _din(e), _din(e, (1 << 16) + 8), 2, 8, 8, S444, DEV, O(e), HOST), both)
    add("jpeg_coefficients_device_coef_off_16",
        lambda e: e.L.ck_jpeg_coefficients_device(e.h, e.jpeg_ptrs, e.jpeg_lens, 2, C.byref(e.jpeg_geom), _dout(e, 4), _dout(e, 1 << 16), DEV, C.byref(e.found)), both)
    add("jpeg_coefficients_device_quant_off_16",
        lambda e: e.L.ck_jpeg_coefficients_device(e.h, e.jpeg_ptrs, e.jpeg_lens, 2, C.byref(e.jpeg_geom), _dout(e), _dout(e, (1 << 16) + 2), DEV, C.byref(e.found)), both)
    add("jpeg_forward_coef_off_16", lambda e: e.L.ck_jpeg_forward(e.h, I(e), 2, 8, 8, HOST, Q(e), S444, _dout(e, 8), DEV),
        "coefficients must lie on 16 bytes")
    add("jpeg_entropy_encode_device_coef_off_16",
        lambda e: e.L.ck_jpeg_entropy_encode_device(e.h, _din(e, 2), DEV, Q(e), 2, 8, 8, S444, 0, O(e), e.jpeg_stride, e.jpeg_len),
        "coefficients must lie on 16 bytes")
    add("harvest_goban_off_4", lambda e: _harvest(e, _din(e, 2), DEV, O(e), _p(e.out[1 << 17:]), HOST),
        "goban images in device memory must be 4-byte aligned")
    add("harvest_x_off_8", lambda e: _harvest(e, _p(e.goban), HOST, _dout(e, 4), _dout(e, 1 << 17), DEV),
        "x in device memory must be 8-byte aligned, src 4-byte aligned")
    add("harvest_src_off_4", lambda e: _harvest(e, _p(e.goban), HOST, _dout(e), _dout(e, (1 << 17) + 2), DEV),
        "x in device memory must be 8-byte aligned, src 4-byte aligned")
    add("augment_x_off_4", lambda e: e.L.ck_augment_patches(e.h, _din(e, 1), 2, DEV, _p(e.codes), O(e), HOST),
        "patches in device memory must be 4-byte aligned")
    add("augment_x_out_off_4", lambda e: e.L.ck_augment_patches(e.h, _p(e.patches), 2, HOST, _p(e.codes), _dout(e, 2), DEV),
        "patches in device memory must be 4-byte aligned")
    add("board_records_rec_off_8", lambda e: e.L.ck_board_detect_records(e.h, I(e), 2, 8, 8, HOST, -1, _dout(e, 4), DEV),
        "records must be 8-byte aligned")
    return c


CASES = _img_cases() + _model_cases() + _alignment_cases()
assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("name,call,code,frag", CASES, ids=[c[0] for c in CASES])
def test_refused_with_its_code_and_message(env, name, call, code, frag):
    env.ck._chk(env.L.ck_rng_set(env.h, 12345))                  # a call that succeeds: the message below is this case's own
    before = env.L.ck_last_error(env.h)
    assert call(env) == code
    if frag is None:                                             # refused without a message: the last one stays
        assert env.L.ck_last_error(env.h) == before
        return
    if "%d" in frag:
        frag = frag % (env.tr_dead if "trainer" in frag else env.mog_dead)
    assert frag in env.L.ck_last_error(env.h).decode()


def test_region_records_refuse_rows_off_8_bytes(env):
    """k_records_put_regions: reached only with weights, so on the second context; the rows stay as they were"""
    import torch
    L, h = env.L, env.ck_net._h
    env.dev_out.fill_(0xEE)
    torch.cuda.synchronize()
    assert L.ck_cnn_regions_records(h, _p(env.goban), 1, HOST, _dout(env, 4), DEV) == ARG
    assert b"records must be 8-byte aligned" in L.ck_last_error(h)
    assert bool((env.dev_out == 0xEE).all())
    assert L.ck_cnn_regions_records(h, _p(env.goban), 1, HOST, _dout(env, 8), DEV) == 0
    assert not bool((env.dev_out[8:8 + 1440] == 0xEE).all()) and bool((env.dev_out[8 + 1440:] == 0xEE).all())
    env.dev_out.zero_()
    torch.cuda.synchronize()


def test_create_refusals():
    from camkifu_amd import capi
    L = capi.lib()
    assert L.ck_ctx_create(0, None) == ARG and b"out is NULL" in L.ck_last_error(None)
    h = C.c_void_p()
    assert L.ck_ctx_create(4096, C.byref(h)) == ARG and b"device 4096 out of range" in L.ck_last_error(None)
    assert not h.value
    assert L.ck_ctx_create(-1, C.byref(h)) == ARG and b"device -1 out of range" in L.ck_last_error(None)
    assert L.ck_ctx_destroy2(None) == 0


def test_the_context_still_works_after_every_refusal(env):
    """the refusals above left the context usable: one small median, host to host"""
    img = env.buf[:2 * 8 * 8 * 3].reshape(2, 8, 8, 3)
    got = env.ck.median(img, 3)
    assert got.shape == img.shape
    assert env.ck.mog2_apply(env.mog, env.buf[:40 * 60 * 3].reshape(40, 60, 3), 0.01).shape == (40, 60)

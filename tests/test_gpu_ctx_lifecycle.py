"""A context owns its memory: three create -> use -> close cycles in one process, each leaving a live MOG2 model and a
live trainer to go down with the context.  Every result of cycles 2 and 3 equals cycle 1 bit for bit (the stages used draw
no random numbers), and close() returns without error.  Free device memory is not looked at -- the machines are shared;
that every allocation is freed once is what tools/sanitize/buf_stress.cpp proves on the buffer types themselves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 96, 128            # two range tiles each way (CK_RANGE_TILE 48), a plane pitch of 128


def _frames():
    rng = np.random.default_rng(2024)
    fr = rng.integers(90, 120, (2, H, W, 3), dtype=np.uint8)
    fr[0, 14:80, 20:110] = rng.integers(180, 200, (66, 90, 3), dtype=np.uint8)       # a bright board-like rectangle
    fr[1, 8:90, 12:100] = rng.integers(20, 40, (82, 88, 3), dtype=np.uint8)          # a dark one
    fr[1, 30:60, 40:80] = 230
    return fr


def _cycle(capi, weights, frames, i420, goban, model_frames, patches, labels):
    ck = capi.Context(0)
    out = {}
    res, lines = ck.board_detect(frames, raw=True)
    out["board_res"], out["board_lines"] = res.copy(), lines.copy()
    out["goban_canny"], out["otsu"] = ck.goban_canny(frames, want_otsu=True)
    out["pyr"] = ck.pyr_down(frames, 2)
    M = np.array([[1.1, 0.05, -3.0], [0.02, 0.9, 2.0], [1e-4, 2e-4, 1.0]])
    out["warp"] = ck.warp_perspective(frames, M, dsize=64)
    out["bgr"] = ck.i420_to_bgr(i420, H, W)
    a, b = ck.mog2_create(40, 60), ck.mog2_create(40, 60)
    out["fg_a"] = ck.mog2_apply(a, model_frames[0], -1.0)
    out["fg_b"] = ck.mog2_apply(b, model_frames[1], -1.0)
    ck.mog2_destroy(b)
    ck.cnn_set_weights(weights)
    out["region_label"], out["region_conf"] = ck.cnn_regions(goban)
    tr = ck.train_create(weights)
    out["loss"] = np.float32(ck.train_step(tr, patches, labels, lr=0.001, dropout=True, seed=5))
    trained = ck.train_weights(tr)
    for k in capi.WEIGHT_ORDER:
        out["w_" + k] = trained[k]
    ck.close()                                   # model `a` and the trainer are alive: they go with the context
    assert not ck._h
    return out


def test_three_cycles_give_the_same_bits():
    from camkifu_amd import capi
    from camkifu_amd.stone.nn_manager import NNManager
    weights = NNManager.init_net()
    rng = np.random.default_rng(7)
    frames = _frames()
    i420 = rng.integers(0, 256, (2, H * W * 3 // 2), dtype=np.uint8)
    goban = rng.integers(0, 256, (1, 380, 380, 3), dtype=np.uint8)
    model_frames = rng.integers(0, 256, (2, 40, 60, 3), dtype=np.uint8)
    patches = rng.integers(0, 256, (2, 40, 40, 3), dtype=np.uint8)
    labels = np.array([4, 77])
    args = (capi, weights, frames, i420, goban, model_frames, patches, labels)
    first = _cycle(*args)
    assert first["goban_canny"].any() and first["pyr"].shape == (2, 24, 32, 3) and first["fg_a"].shape == (40, 60)
    assert np.isfinite(first["loss"]) and any(not np.array_equal(first["w_" + k], weights[k]) for k in capi.WEIGHT_ORDER)
    for cycle in (2, 3):
        again = _cycle(*args)
        assert again.keys() == first.keys()
        for k in first:
            assert np.array_equal(again[k], first[k]), "cycle %d: %s differs from cycle 1" % (cycle, k)

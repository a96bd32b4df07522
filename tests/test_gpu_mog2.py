"""K9 (MOG2) on the GPU against the CPU oracle through saturation, pruning, the all-pruned update and every kind of
learning rate, in all three forms that share mix_update (k_mog2.hip): the frame form (ck_mog2_apply), the ordered run
of a band (ck_mog2_band_run) and the ordered run of the whole goban (ck_stones_run).  Masks or zone counts are checked
every frame, and the mixture itself (Context.mog2_state against MOG2.state: nmodes, then weight / variance / mean of the
live slots bit for bit, NaN equal to NaN) at checkpoints and at the end, so a state divergence that has not flipped a
pixel yet is seen too.  Scenes and rate schedules: tests/mog2_scenes.py."""
import numpy as np
import pytest

from tests import mog2_scenes as S

pytestmark = pytest.mark.gpu
DST = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same_state(ck, handle, model, what):
    bad = S.state_mismatch(ck.mog2_state(handle), model.state())
    assert bad is None, "%s: %s" % (what, bad)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _chunks(gen, h, w, n, seed, size=40):
    """frames 0 .. n of a scene, made `size` at a time"""
    for t0 in range(0, n, size):
        fr = gen(h, w, range(t0, min(n, t0 + size)), seed)
        for i in range(len(fr)):
            yield t0 + i, fr[i]


def _frame_form(ck, ora, gen, h, w, r, seed, what):
    """the frame form over one sequence, host and device inputs alternating; masks every frame, state at checkpoints"""
    hd, model = ck.mog2_create(h, w), ora.MOG2(h, w, 3)
    try:
        for t, img in _chunks(gen, h, w, len(r), seed):
            got = _host(ck.mog2_apply(hd, _dev(img) if t % 2 else img, float(r[t])))
            want = model.apply(img, float(r[t]))
            assert np.array_equal(got, want), "%s: mask of frame %d (rate %g), %d pixels differ" % (
                what, t, r[t], int((got != want).sum()))
            if t % 10 == 9 or t == len(r) - 1 or r[t] > 0.5 or r[t - 1] > 0.5:
                _same_state(ck, hd, model, "%s, frame %d" % (what, t))
        return model.events()
    finally:
        ck.mog2_destroy(hd)


FRAME_SIZES = [(380, 380), (40, 380), (37, 53), (1, 1)]


@pytest.mark.parametrize("h,w", FRAME_SIZES, ids=["%dx%d" % s for s in FRAME_SIZES])
def test_frame_form_against_the_oracle(ck, ora, h, w):
    """ck_mog2_apply at pixel counts that are (380 x 380 = 564 x 256 + 16) and are not a multiple of 256, through every
    schedule including the reset (the whole goban: the `mixed` schedule, which holds all of them in 120 frames) and
    every scene (the mosaic deals them over the pixels; a 1 x 1 model runs each scene on its own)"""
    schedules = ("mixed",) if h * w > 100000 else S.SCHEDULES
    gens = dict(S.SCENES) if h * w == 1 else dict(mosaic=S.mosaic)
    total = dict.fromkeys(ora.MOG2_EVENTS, 0)
    for name in schedules:
        n = 260 if name == "auto" else 120
        for gname, gen in gens.items():
            ev = _frame_form(ck, ora, gen, h, w, S.rates(name, n), seed=h * 1000 + w, what="%s %s %dx%d" % (gname, name, h, w))
            for k in total:
                total[k] += ev[k]
    if h * w > 1000:                                   # the sequences reached the rare branches
        assert all(v > 0 for v in total.values()), total


def _run_rates(n):
    """rates for ordered runs (no reset): zero, the product's rates and high ones, then the automatic rate to its cap"""
    r = S.rates("auto", n)
    r[1:20] = (0.01, 0.01, 0.005, 0, 0, 0.01, 0.95, 0.6, 0.8, 0.01, 0.01, 0, 0.01, 0.005, 0.005, 0.3, 0.3, 0.01, 0.01)
    return r


def test_band_run_lengths_against_the_oracle(ck, ora):
    """ck_mog2_band_run on one 380-row band with last_band (the whole goban's skip row and column), runs of 1, 3, 4, 5,
    7 and 300 frames in one launch each (the kernel pipelines frames in groups of 4): zone counts of every frame equal
    ora.zone_counts of the oracle's mask, the state after every run equals the oracle's; the automatic rate reaches its
    cap at frame 250 inside the 300-frame run"""
    lengths = (1, 3, 4, 5, 7, 300)
    n = sum(lengths)
    r = _run_rates(n)
    hd, model = ck.mog2_create(380, 380), ora.MOG2(380, 380, 3)
    t0 = 0
    for i, k in enumerate(lengths):
        band = S.mosaic(380, 380, range(t0, t0 + k), seed=17)
        got = _host(ck.mog2_band_run(hd, _dev(band) if i % 2 else band, r[t0:t0 + k], last_band=True))
        assert got.shape == (k, 19, 19)
        for j in range(k):
            mask = model.apply(band[j], float(r[t0 + j]))
            want = S.zone_counts(mask)
            if j in (0, k - 1):
                assert np.array_equal(want, ora.zone_counts(mask))
            assert np.array_equal(got[j], want), "run of %d, frame %d: %d zones differ" % (k, t0 + j, int((got[j] != want).sum()))
        _same_state(ck, hd, model, "after the run of %d (frames %d .. %d)" % (k, t0, t0 + k - 1))
        t0 += k
    ev = model.events()
    assert ev["prune"] > 0 and ev["replace"] > 0 and ev["zero_total"] > 0, ev
    ck.mog2_destroy(hd)


@pytest.fixture(scope="module")
def whole_image_run(ora):
    """40 frames of the mosaic with a high-rate segment, through the whole-image oracle: frames, rates, masks, state"""
    n = 40
    frames = S.mosaic(380, 380, range(n), seed=23)
    r = S.rates("high", n)
    model = ora.MOG2(380, 380, 3)
    masks = np.stack([model.apply(frames[t], float(r[t])) for t in range(n)])
    return frames, r, masks, model.state()


def _rows(state, y0, y1):
    """the pixel rows [y0, y1) of a 380 x 380 mixture, in the layout of a band model of those rows"""
    out = {}
    for k, v in state.items():
        a = v.reshape(v.shape[:-1] + (380, 380))[..., y0:y1, :]
        out[k] = np.ascontiguousarray(a.reshape(v.shape[:-1] + (-1,)))
    return out


@pytest.mark.parametrize("world", [2, 3, 8])
def test_band_states_are_rows_of_the_whole_image(ck, ora, world, whole_image_run):
    """pixel bands as pipeline.band_rows deals them: each band's counts are the matching zone rows of the whole image's,
    and each band's mixture is the matching rows of the whole-image oracle's, bit for bit (two runs: 17 + 23 frames)"""
    from camkifu_amd import pipeline
    frames, r, masks, state = whole_image_run
    want_counts = np.stack([S.zone_counts(m) for m in masks])
    for a, b in pipeline.band_rows(world):
        y0, y1 = 20 * a, min(20 * b, 380)
        last = b == 19
        hd = ck.mog2_create(y1 - y0, 380)
        band = np.ascontiguousarray(frames[:, y0:y1])
        got = np.concatenate([_host(ck.mog2_band_run(hd, band[:17], r[:17], last_band=last)),
                              _host(ck.mog2_band_run(hd, _dev(band[17:]), r[17:], last_band=last))])
        assert np.array_equal(got, want_counts[:, a:b]), "world %d, band rows %d .. %d" % (world, a, b)
        bad = S.state_mismatch(ck.mog2_state(hd), _rows(state, y0, y1))
        assert bad is None, "world %d, band rows %d .. %d: %s" % (world, a, b, bad)
        ck.mog2_destroy(hd)


def test_apply_and_run_interleaved_on_one_handle(ck, ora):
    """apply, run, apply, run on one model: the frame count and the mixture carry over from one form to the other"""
    segs = (("apply", 5), ("run", 7), ("apply", 6), ("run", 9))
    n = sum(k for _, k in segs)
    frames = S.mosaic(380, 380, range(n), seed=29)
    r = np.full(n, 0.01)
    r[0] = -1
    r[8], r[13], r[14], r[21] = 0.95, 0, 0.005, -1
    hd, model = ck.mog2_create(380, 380), ora.MOG2(380, 380, 3)
    t0 = 0
    for form, k in segs:
        if form == "apply":
            for t in range(t0, t0 + k):
                assert np.array_equal(_host(ck.mog2_apply(hd, frames[t], float(r[t]))), model.apply(frames[t], float(r[t]))), t
        else:
            got = _host(ck.mog2_band_run(hd, frames[t0:t0 + k], r[t0:t0 + k], last_band=True))
            for j in range(k):
                assert np.array_equal(got[j], S.zone_counts(model.apply(frames[t0 + j], float(r[t0 + j])))), t0 + j
        _same_state(ck, hd, model, "after %s of frames %d .. %d" % (form, t0, t0 + k - 1))
        t0 += k
    ck.mog2_destroy(hd)


def test_stones_run_hand_clip_against_the_oracle(ck, ora):
    """ck_stones_run over 150 frames of the hand clip in three runs: the hand's modes are pruned between its visits
    (rate 0.3) and it comes back; zone counts every frame and the final mixture equal the oracle's (warp + MOG2)"""
    from camkifu_amd.stone.nn_manager import NNManager
    from tests.test_gpu_ordered import _clip
    ck.cnn_set_weights(NNManager.init_net())
    n = 150
    frames, corners = _clip(n, seed=31)
    M = ora.get_perspective_transform(corners, DST)
    r = np.full(n, 0.3)
    r[:25] = 0.01
    hd, model = ck.mog2_create(380, 380), ora.MOG2(380, 380, 3)
    for t0 in (0, 50, 100):
        got = _host(ck.stones_run(frames[t0:t0 + 50], M, mog2=hd, learning_rates=r[t0:t0 + 50])["fgcount"])
        for j in range(50):
            want = S.zone_counts(model.apply(ora.warp_perspective(frames[t0 + j], M), float(r[t0 + j])))
            assert np.array_equal(got[j], want), "frame %d: %d zones differ" % (t0 + j, int((got[j] != want).sum()))
    _same_state(ck, hd, model, "after 150 frames")
    assert model.events()["prune"] > 0
    ck.mog2_destroy(hd)


def test_high_rate_segment_keeps_the_state_finite(ck, ora):
    """a saturated model (7-colour cycle, 60 frames at 0.01), then rates 0.95 / 0.6 / 0.95, then 0.01 again: every mode
    of a pixel that matches none is pruned in one update.  The frame form (37 x 53) and the run form (a 40-row band)
    keep every live slot finite and equal to the oracle's"""
    n = 84
    r = np.full(n, 0.01)
    r[60:63] = (0.95, 0.6, 0.95)
    for form, (h, w) in (("apply", (37, 53)), ("run", (40, 380))):
        frames = S.cycle(h, w, range(n), seed=37)
        hd, model = ck.mog2_create(h, w), ora.MOG2(h, w, 3)
        if form == "apply":
            for t in range(n):
                assert np.array_equal(_host(ck.mog2_apply(hd, frames[t], float(r[t]))), model.apply(frames[t], float(r[t]))), t
                if t >= 59:
                    _same_state(ck, hd, model, "apply, frame %d" % t)
                    assert np.isfinite(S.live_values(ck.mog2_state(hd))).all(), t
        else:
            for t0, t1 in ((0, 60), (60, 61), (61, 63), (63, n)):
                ck.mog2_band_run(hd, frames[t0:t1], r[t0:t1], last_band=False)
                for t in range(t0, t1):
                    model.apply(frames[t], float(r[t]))
                _same_state(ck, hd, model, "run, frames %d .. %d" % (t0, t1 - 1))
                assert np.isfinite(S.live_values(ck.mog2_state(hd))).all(), (t0, t1)
        assert model.events()["zero_total"] > 0
        ck.mog2_destroy(hd)


def test_exact_weight_ties_bubble_the_matched_mode(ck, ora):
    """two modes of exactly 0.5, then rate 0: every match at mode 1 ties with mode 0 and, by `!(weight < gw[i-1])`,
    moves above it.  Masks cannot see the order of the modes; the state compared after every frame (frame form, 37 x 53)
    and after every run of 1 .. 5 frames (run form, a 40-row band) does"""
    n = 40
    r = S.rates("tie", n)
    for form, (h, w) in (("apply", (37, 53)), ("run", (40, 380))):
        frames = S.tie(h, w, range(n), seed=43)
        hd, model = ck.mog2_create(h, w), ora.MOG2(h, w, 3)
        if form == "apply":
            for t in range(n):
                assert np.array_equal(_host(ck.mog2_apply(hd, frames[t], float(r[t]))), model.apply(frames[t], float(r[t]))), t
                _same_state(ck, hd, model, "apply, frame %d" % t)
        else:
            t0 = 0
            for k in (1, 1, 3, 5, 2, 4) * 3:
                k = min(k, n - t0)
                ck.mog2_band_run(hd, frames[t0:t0 + k], r[t0:t0 + k], last_band=False)
                for t in range(t0, t0 + k):
                    model.apply(frames[t], float(r[t]))
                _same_state(ck, hd, model, "run, frames %d .. %d" % (t0, t0 + k - 1))
                t0 += k
                if t0 >= n:
                    break
        assert model.events()["bubble"] >= h * w * 20
        ck.mog2_destroy(hd)

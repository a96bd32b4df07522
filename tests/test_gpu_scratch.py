"""What a call finds in the context's scratch memory must not change its result.

A ck_ctx holds some forty scratch buffers that grow on demand, never shrink and are shared by unrelated entry points; a
trainer keeps its chunk buffers and partial sums.  Every other GPU test file starts from a fresh context and small shapes,
so a kernel that reads a counter, an accumulator or a list tail it never wrote has only ever met what the driver hands out
for new memory or what the same entry point left a moment ago.  Here every entry point of tests/scratch_cases.py is held to
the plain reference of its own test file

  * on a fresh context (every buffer grows inside the call), after a larger call of the same entry point, and after
    ck_debug_scratch_fill has set every scratch byte to 0x00, 0xFF and 0x55      test_entry_point_whatever_scratch_holds
  * after every other entry point, forwards and backwards on ONE context, a fill between neighbours; and the K2 -> K3
    label reuse of ck_board_detect around a ck_board_lines on the caller's own edge map, with no fill between
                                                                                  test_every_entry_point_after_every_other
  * one trainer through batches of 257, 3, 65, 1 and 257 patches                  test_one_trainer_many_batch_sizes
  * and the hook itself: what it counts, what it must not touch, the two results that lie in scratch between calls
    (the encoder's histograms, the PNG token counters) answering as before the first encode
                                                                                  test_the_hook_itself

docs/lab_notes.md (note 18) goes through the buffers one by one: no value that a call reads before it has written it is
used as an index, a count or a loop bound.  The mutants below are therefore all of the other kind -- what goes stale is
DATA -- and each one says where that shows.  Each was built as a library of its own, run once against this file, and is
not kept:

  1 k_gray_hist without its hipMemsetAsync (k_color.hip)
        the bins are summed in double by ck_otsu_level over i = 0 .. 255, a fixed loop; a bin is never an index or a bound
        -> test_entry_point_whatever_scratch_holds[goban_canny] (the Otsu level, from the second call on) and
           [contour_stones] (its image edges come from the same level), test_every_entry_point_after_every_other
  2 the first chunk's tr_reduce with accumulate = 1 (k_cnn_train.hip, wgrad)
        `g[i] = (float)((double)g[i] + s)` for i < count: a float added at a place of its own
        -> test_one_trainer_many_batch_sizes (the second call on the handle, and every call after a fill: NaN at 0xFF),
           test_entry_point_whatever_scratch_holds[train_step] (its step follows a train_grads on the same handle); the
           other trainer rows make one call on a fresh trainer, whose g ck_train_create has cleared, and do not see it
  3 ck_debug_scratch_fill without the drop of jenc_freq_frames / png_count_frames / png_tokens
        both readers copy as many bytes as the last pass laid out, from where it laid them out, inside a buffer that never
        shrinks; what they then hand back are the filled bytes as counters
        -> test_the_hook_itself
  4 k_grid_lines without the hipMemsetAsync of its histogram (k_gridlines.hip)
        as 1: the 256 bins feed ck_otsu_level only
        -> test_entry_point_whatever_scratch_holds[find_intersections] (on its noisy goban: tests/scratch_cases.py)
  5 k_png_enc_put without the hipMemsetAsync of the packed streams (k_png.hip)
        the codes are OR-ed into dwords of the stream at offsets that come from the scans, not from the stream
        -> test_entry_point_whatever_scratch_holds[png_encode] and [png_encode_runs], test_the_hook_itself"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import scratch_cases as sc
from tests import train_cases as tc
from tests import train_ref as tr
from tests.align_cases import stops_at_a_hip_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(ora):
    """the rows; the context that tests/handover_cases.build derives a few inputs with is closed again"""
    from camkifu_amd import capi
    ctx = capi.Context(0)
    try:
        T = sc.build(ctx, ora)
    finally:
        ctx.close()
    assert sorted(T) == sorted(sc.NAMES) and len(set(sc.NAMES)) == len(sc.NAMES) == 49
    return T


@pytest.fixture()
def ctx():
    from camkifu_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sc.NAMES)
@stops_at_a_hip_error
def test_entry_point_whatever_scratch_holds(table, ctx, name):
    row = table[name]
    row.check(row.run(ctx))                         # a fresh context: every buffer grows inside the call
    row.grow(ctx)
    row.check(row.run(ctx))                         # the smaller call after the larger
    for byte in sc.FILL_BYTES:
        nbytes, nbufs = ctx.scratch_fill(byte)
        assert nbytes > 0 and nbufs > 0, name       # (every one of these entry points keeps something in scratch)
        row.check(row.run(ctx))


@stops_at_a_hip_error
def test_every_entry_point_after_every_other(table, ctx):
    """each call meets buffers sized and last written by unrelated entry points"""
    walk = list(sc.NAMES) + list(reversed(sc.NAMES))
    for k, name in enumerate(walk):
        if k:
            ctx.scratch_fill((0xFF, 0x00, 0x55)[k % 3])
        t0 = time.perf_counter()
        table[name].check(table[name].run(ctx))
        if time.perf_counter() - t0 > 1.0:
            print("%s: %.2f s" % (name, time.perf_counter() - t0))
    # the deliberate reuse: K3 of ck_board_detect keeps the labels K2 left in ctx->labels; ck_board_lines on an edge map of
    # the caller's must not, whatever a ck_board_detect before it left there -- and the other way round
    for name in ("board_detect", "board_lines", "board_detect", "board_detect_records", "board_lines", "board_edges", "board_lines",
                 "board_detect"):
        table[name].check(table[name].run(ctx))


BATCHES = ("n257", "n3", "n65", "n1", "n257")


def _same_grads(a, b):
    return a[0] == b[0] and all(np.array_equal(a[1][k].view(np.uint32), b[1][k].view(np.uint32)) for k in tr.ORDER)


@stops_at_a_hip_error
def test_one_trainer_many_batch_sizes(ctx):
    """a large batch, then small ones, on ONE handle: the chunk buffers and the partial sums of the larger call are still
    there, and tr_reduce adds the second chunk of 257 "onto the sum of the earlier chunks".  Every call within TOL of the
    float64 reference and bit-equal to the same call on a trainer of its own that never saw a fill; then two steps."""
    from camkifu_amd import capi
    from tests.test_gpu_train import TOL
    assert BATCHES[0] == "n%d" % (tc.CHUNK + 1)
    clean = capi.Context(0)                          # never filled
    try:
        fresh = {}
        for name in set(BATCHES):
            hd = clean.train_create(tc.weights())
            fresh[name] = clean.train_grads(hd, *tc.cases()[name], dropout=False)
            clean.train_destroy(hd)
            l_ref, g_ref = tc.reference(name)
            assert abs(fresh[name][0] - l_ref) / abs(l_ref) <= TOL, name
            for k, e in tr.grad_error(fresh[name][1], g_ref).items():
                assert e <= TOL, (name, k, e)
        hd = ctx.train_create(tc.weights())
        for fill in (False, True):
            for k, name in enumerate(BATCHES):
                if fill:
                    ctx.scratch_fill((0xFF, 0x55, 0x00)[k % 3])
                got = ctx.train_grads(hd, *tc.cases()[name], dropout=False)
                l_ref, g_ref = tc.reference(name)
                assert abs(got[0] - l_ref) / abs(l_ref) <= TOL, (name, fill, got[0], l_ref)
                for key, e in tr.grad_error(got[1], g_ref).items():
                    assert e <= TOL, (name, fill, key, e)
                assert _same_grads(got, fresh[name]), (name, "after a fill" if fill else "after " + BATCHES[k - 1] if k else "first")
        # two steps with dropout, a fill in front of each, against a trainer that never saw one
        other = clean.train_create(tc.weights())
        for step, name in enumerate(("n65", "n3")):
            ctx.scratch_fill((0xFF, 0x55)[step])
            x, y = tc.cases()[name]
            assert ctx.train_step(hd, x, y, lr=0.001, dropout=True, seed=9) == clean.train_step(other, x, y, lr=0.001, dropout=True, seed=9)
        w, w_clean = ctx.train_weights(hd), clean.train_weights(other)
        (m, v, steps), (m_clean, v_clean, steps_clean) = ctx.train_adam_state(hd), clean.train_adam_state(other)
        assert steps == steps_clean == 2
        for k in tr.ORDER:
            for a, b in ((w, w_clean), (m, m_clean), (v, v_clean)):
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
            assert not np.array_equal(w[k], tc.weights()[k]), k                  # (the steps did move the weights)
    finally:
        clean.close()


@stops_at_a_hip_error
def test_the_hook_itself(table, ctx):
    from camkifu_amd import capi
    from tests import mog2_scenes as ms
    L = capi.lib()
    assert ctx.scratch_fill(0xAB) == (0, 0)                                     # a fresh context holds no scratch
    row = table["median"]
    row.check(row.run(ctx))
    small = ctx.scratch_fill(0x11)
    assert small[0] > 0 and small[1] > 0
    row.grow(ctx)
    large = ctx.scratch_fill(0x22)
    assert large[0] > small[0] and large[1] >= small[1]
    row.check(row.run(ctx))
    assert ctx.scratch_fill(0x33) == large                                      # never shrunk, and nothing new for the smaller call
    # ---- what is state stays: the classifier's weights, a MOG2 mixture, a trainer's weights and moments
    W, gather = sc.exact_net()
    ctx.cnn_set_weights(W)
    rl0, rc0 = ctx.cnn_regions(gather)
    model = ctx.mog2_create(20, 40)
    frames = np.random.default_rng(5).integers(0, 256, (3, 20, 40, 3), dtype=np.uint8)
    for f in frames:
        ctx.mog2_apply(model, f, 0.05)
    x, y = tc.cases()["n3"]
    trainer = ctx.train_create(tc.weights())
    ctx.train_step(trainer, x, y, lr=0.001, dropout=True, seed=1)
    ctx.train_destroy(trainer)                                                  # (in_stage has its size for the step now)
    without = ctx.scratch_fill(0x44)
    trainer = ctx.train_create(tc.weights())
    ctx.train_step(trainer, x, y, lr=0.001, dropout=True, seed=1)
    before = ctx.mog2_state(model), ctx.train_weights(trainer), ctx.train_adam_state(trainer)
    with_trainer = ctx.scratch_fill(0xFF)
    # the trainer's per-call buffers are filled too: g, lab, the sixteen maps of a chunk, part, lossv (no masks were asked for)
    assert with_trainer[1] == without[1] + 20 and with_trainer[0] > without[0]
    after = ctx.mog2_state(model), ctx.train_weights(trainer), ctx.train_adam_state(trainer)
    for k in ("weight", "variance", "mean", "nmodes"):
        assert before[0][k].tobytes() == after[0][k].tobytes(), k                # (all of it, the slots above nmodes included)
    assert ms.state_mismatch(before[0], after[0]) is None
    for k in tr.ORDER:
        assert before[1][k].tobytes() == after[1][k].tobytes() and before[2][0][k].tobytes() == after[2][0][k].tobytes()
        assert before[2][1][k].tobytes() == after[2][1][k].tobytes(), k
    assert before[2][2] == after[2][2] == 1
    rl1, rc1 = ctx.cnn_regions(gather)
    assert np.array_equal(rl0, rl1) and rc0.tobytes() == rc1.tobytes()
    ctx.train_destroy(trainer)
    assert ctx.scratch_fill(0x00) == without                                    # a trainer that is gone is not filled
    ctx.mog2_destroy(model)
    # ---- the two results that lie in scratch between calls: dropped with it, and back after the next encode
    one, counts = (C.c_longlong * 2)(), np.zeros((2, 4, 256), np.uint32)
    jpeg_none, png_none = b"the last pass counted 0 frames, not 2", b"no ck_png_encode of this context has completed"

    def histograms():
        return L.ck_jpeg_encode_histograms(ctx._h, 2, counts.ctypes.data_as(C.c_void_p)), L.ck_last_error(ctx._h)

    def run_stats():
        return L.ck_png_run_stats(ctx._h, 2, one, one), L.ck_last_error(ctx._h)
    rc, msg = histograms()
    assert rc == capi.CK_ERR_STATE and jpeg_none in msg                          # before any encode
    rc, msg = run_stats()
    assert rc == capi.CK_ERR_STATE and png_none in msg and ctx.png_run_stats() == []
    for byte in (0xFF, 0x00):
        table["jpeg_encode_optimised_device"].check(table["jpeg_encode_optimised_device"].run(ctx))
        table["png_encode_runs"].check(table["png_encode_runs"].run(ctx))
        assert histograms()[0] == capi.CK_OK and run_stats()[0] == capi.CK_OK
        hist, stats = ctx.jpeg_encode_histograms(2), ctx.png_run_stats()
        assert hist.sum() > 0 and len(stats) == 2 and stats[1]["matches"] > 0
        ctx.scratch_fill(byte)
        rc, msg = histograms()
        assert rc == capi.CK_ERR_STATE and jpeg_none in msg, (byte, rc, msg)
        rc, msg = run_stats()
        assert rc == capi.CK_ERR_STATE and png_none in msg and ctx.png_run_stats() == [], (byte, rc, msg)
    table["jpeg_encode_optimised_device"].run(ctx)
    table["png_encode_runs"].run(ctx)
    assert np.array_equal(ctx.jpeg_encode_histograms(2), hist) and ctx.png_run_stats() == stats
    # ---- the argument errors
    assert L.ck_debug_scratch_fill(None, 0, None, None) == capi.CK_ERR_ARG
    for bad in (-1, 256):
        assert L.ck_debug_scratch_fill(ctx._h, bad, None, None) == capi.CK_ERR_ARG and b"fill byte %d: 0 .. 255" % bad in L.ck_last_error(ctx._h)
        with pytest.raises(capi.CkError) as err:
            ctx.scratch_fill(bad)
        assert err.value.code == capi.CK_ERR_ARG
    assert L.ck_debug_scratch_fill(ctx._h, 7, None, None) == capi.CK_OK         # the totals are optional
    row.check(row.run(ctx))

"""The stream-ordered hand-over of device memory (capi.Context._in / _out / _out_on / _rec, Context.wait_stream, the rule of
FastFilePipeline._detect_frames), held on the GPU with the producer STILL PENDING when the pointer crosses the C-ABI.  Everywhere
else in the suite a device tensor is complete before Python sees it, so a ck_stream_wait that did nothing would go unnoticed.

The delay is torch.cuda._sleep, its cycles calibrated against torch events once per module (tests/handover_cases.py: Delay).
Measured on an MI355X, warm, from queuing the producer to the library's ck_stream_wait (time.perf_counter(), five runs): harvest_patches
0.049 .. 0.064 ms (three output allocations come first), train_create 0.028 .. 0.071, stones_run 0.031 .. 0.064, cnn_set_weights
0.039 .. 0.044, median15 0.015 .. 0.018; 2.38 .. 2.40 million _sleep cycles per millisecond.  DELAY_MS = 25 is 350 times the
slowest; test_the_delay_outlasts_the_host_path measures again and asserts a factor of ten.  A case's own set-up (host weights for
the classifier: 21 ms of packing; a fresh background model or trainer) runs BEFORE its producer is queued (Case.run's `produce`
hook).
Every case asserts, immediately before the library call, that an event recorded behind its producer has not completed: a case
whose producer is already done fails as a bad set-up.

The positive control (the `ck` fixture, once per module; test_positive_control_shows_the_stale_result reports it): a stream that
is NOT the current one delays, then copies B over A; the library, called without wait_stream, must return A's result while that
event is still pending -- once with the producer on a side stream and the null stream current, once the other way round.  With
four hardware queues the order in which streams are created decides which of them share one: side streams, then ONE context, kept
the null stream, both side streams and the context apart on an MI355X; one or two more contexts created before it made a pair
share a queue (the call then waited for the delay and read the fresh content).  So the pipeline's test creates no context of its
own.  A control that returns B's result fails every test here.

Not covered, with the reason: jpeg_decode and jpeg_coefficients_device take host streams only (they are in the output tests);
train_apply brings device gradients down through torch itself (`.cpu()` on the current stream), so nothing is handed over --
it is in the table all the same; overlay_draw draws in place, so its image is input and output in one (the input test).
In the recycled-block test every method of the table reuses the noted blocks; none had to be left out.

Found by this file: ck_cnn_set_weights fetched device weights with a plain hipMemcpy, i.e. on the null stream, which nothing
orders behind a non-blocking producer stream -- stale weights with a side stream current ([cnn_set_weights-*-side]).  They now
come down on the context's stream.

Mutants, each built in a scratch copy and run once against this file on an MI355X (the cases that fail, of 208):
    ck_stream_wait returns without recording or waiting      200: every test but the controls, the table's names, the delay's
                                                             measurement and train_apply (whose gradients torch itself brings down)
    _out hands a device `out=` through without _in             2: test_an_out_with_a_pending_writer_and_host_input (i420_to_bgr from
                                                             host memory, jpeg_decode).  With a device INPUT the input's own
                                                             hand-over has already ordered the context behind the late fill: one
                                                             ck_stream_wait orders it behind everything torch has queued
    harvest_patches takes fgcount.data_ptr() directly          2: test_a_device_argument_among_host_arguments[harvest_patches-1] (for
                                                             the same reason only where fgcount is the call's one device tensor)
    ck_i420_to_bgr returns without finish()                    5: test_results_are_complete_on_return_plain_finish, and
                                                             [i420_to_bgr-0-null], [-side], both recycled-block tests of i420_to_bgr
    timed_detect without wait_stream                           2: test_detect_frames_behind_the_callers_side_stream[slice], [gather]"""
import threading

import numpy as np
import pytest

from tests import handover_cases as hc

pytestmark = pytest.mark.gpu


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    """the two side streams (created BEFORE the context) and the calibrated delay"""
    import torch
    e = Env()
    torch.cuda.set_device(0)
    e.side, e.side2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
    e.delay = hc.Delay()
    return e


def _streams(env, which):
    import contextlib
    import torch
    return contextlib.nullcontext() if which == "null" else torch.cuda.stream(env.side)


def _control(ck, env, producer, current):
    """-> dict(stale, fresh, pending_before, pending_after): what the library returned for a tensor whose late writer runs on
    `producer`, a stream nobody ordered the context behind: capi orders it behind `current` only ("null": the null stream)"""
    import torch
    a, b = hc._noise(21, (2, 16, 24, 3)), hc._noise(22, (2, 16, 24, 3))
    want_a, want_b = ck.median(a, 5), ck.median(b, 5)
    assert not np.array_equal(want_a, want_b)
    t, src = hc.to_device(a), hc.to_device(b)
    torch.cuda.synchronize()
    with _streams(env, producer):
        env.delay.queue()
        t.copy_(src)
        ev = hc.Delay.mark()
    before = not ev.query()
    with _streams(env, current):
        got = ck.median(t, 5)                                     # ordered behind the CURRENT stream only
        after = not ev.query()
        got = got.cpu().numpy()
    torch.cuda.synchronize()
    return dict(stale=np.array_equal(got, want_a), fresh=np.array_equal(got, want_b), pending_before=before, pending_after=after)


@pytest.fixture(scope="module")
def ck(env):
    from camkifu_amd import capi
    ctx = capi.Context(0)
    ctx.median(hc._noise(20, (2, 16, 24, 3)), 5)                  # (scratch buffers and kernels are there before anything is timed)
    env.control = {"side": _control(ctx, env, "side", "null"), "null": _control(ctx, env, "null", "side")}
    if not all(c["stale"] and c["pending_before"] and c["pending_after"] for c in env.control.values()):
        ctx.close()
        pytest.fail("the positive control cannot see a missing order on this machine: %r" % (env.control,))
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def table(ck):
    return hc.build(ck)


@pytest.fixture(scope="module")
def want(ck, table):
    """name -> the method's result for content B in host memory, computed once on the same context"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = hc.norm(table[name].run(ck, table[name].b))
        return cache[name]
    return get


@pytest.mark.parametrize("producer", ["side", "null"])
def test_positive_control_shows_the_stale_result(ck, env, producer):
    c = env.control[producer]
    assert c["pending_before"] and c["pending_after"], c          # the call came back while the late writer was still waiting
    assert c["stale"] and not c["fresh"], c


def test_the_table_names_every_method(table):
    assert sorted(table) == sorted(hc.METHODS)
    assert all(len(table[m].a) == len(table[m].b) == hc.N_ARGS.get(m, 1) for m in hc.METHODS)


def test_the_delay_outlasts_the_host_path(ck, env, table):
    """from queuing the producer to the library's event: the slowest methods of the table (three allocations, twelve weight
    tensors) -- DELAY_MS is at least ten times that"""
    import torch
    worst = {}
    for name in ("harvest_patches", "cnn_set_weights", "train_create", "stones_run", "median15"):
        case = table[name]
        for _ in range(2):                                        # (the second run is the warm one)
            dev = [hc.to_device(x) for x in case.b]
            src = hc.to_device(case.b[0])
            torch.cuda.synchronize()
            sec = hc.host_path_seconds(lambda produce: case.run(ck, dev, produce=produce), lambda: (env.delay.queue(1.0), dev[0].copy_(src)))
        worst[name] = sec * 1e3
    print("host path, ms: " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())) +
          "; cycles per ms %.0f; DELAY_MS %.1f" % (env.delay.cycles_per_ms, hc.DELAY_MS))
    assert hc.DELAY_MS >= 10 * max(worst.values()), worst
    assert hc.DELAY_MS >= 20.0


# ------------------------------------------------------------------------------------------------------------ inputs
def _late_input(ck, env, table, want, name, turn, strided=False, alone=False):
    """alone: the other arguments stay in host memory, so that this tensor's hand-over is the call's only one"""
    import torch
    case = table[name]
    fresh = want(name)
    mixed = list(case.b)
    mixed[turn] = case.a[turn]
    stale = hc.norm(case.run(ck, mixed))
    assert not hc.same(stale, fresh), "bad input: contents A and B of argument %d give %s the same result" % (turn, name)
    dev = list(case.b) if alone else [hc.to_device(x) for x in case.b]
    dev[turn] = hc.to_device(case.a[turn], strided)
    src = hc.to_device(case.b[turn])
    torch.cuda.current_stream().synchronize()

    def produce():
        env.delay.queue()
        dev[turn].copy_(src)
        assert not hc.Delay.mark().query(), "bad set-up: the producer had run before the call"
    got = hc.norm(case.run(ck, dev, produce=produce))
    assert not hc.same(got, stale), "%s read argument %d before its producer had run" % (name, turn)
    assert hc.same(got, fresh)


@pytest.mark.parametrize("which", ["null", "side"])
@pytest.mark.parametrize("name,turn", hc.TURNS, ids=["%s-%d" % t for t in hc.TURNS])
def test_an_input_whose_producer_is_pending(ck, env, table, want, name, turn, which):
    """every method, every device argument in turn, with the null stream current and with a side stream current (_in for the
    argument, _out_on for the method's fresh outputs, _rec for the record rows)"""
    with _streams(env, which):
        _late_input(ck, env, table, want, name, turn)


@pytest.mark.parametrize("which", ["null", "side"])
@pytest.mark.parametrize("name,turn", [("harvest_patches", 1), ("board_detect_records", 1), ("cnn_regions_records", 1)])
def test_a_device_argument_among_host_arguments(ck, env, table, want, name, turn, which):
    """the methods that take their arguments from two memory spaces: one hand-over orders the context behind EVERYTHING torch
    has queued, so a second tensor that skipped it shows only where it is the call's one device tensor (the results of
    harvest_patches lie where the goban images do: host memory here)"""
    with _streams(env, which):
        _late_input(ck, env, table, want, name, turn, alone=True)


@pytest.mark.parametrize("which", ["null", "side"])
@pytest.mark.parametrize("name,turn", [("cnn_set_weights", 0), ("cnn_set_weights", 8), ("train_create", 2), ("train_create", 11)])
def test_a_strided_weight_goes_through_contiguous(ck, env, table, want, name, turn, which):
    """a weight tensor that is not contiguous: capi copies it (`.contiguous()`, queued behind the late writer) and hands the
    copy over"""
    with _streams(env, which):
        _late_input(ck, env, table, want, name, turn, strided=True)


# ----------------------------------------------------------------------------------------------------------- outputs
OUT_METHODS = ["i420_to_bgr", "i420_to_bgr_levels", "jpeg_reconstruct", "jpeg_forward", "pyr_down", "warp_perspective", "augment_patches"]


def _pending_out(ck, env, call, fresh):
    """call(out, produce) with a late fill_ queued on `out` by `produce`: the result, not the sentinel"""
    import torch
    out = torch.zeros(fresh.shape, dtype=getattr(torch, fresh.dtype.name), device="cuda:0")
    torch.cuda.current_stream().synchronize()

    def produce():
        env.delay.queue()
        out.fill_(hc.SENTINEL)
        assert not hc.Delay.mark().query(), "bad set-up: the writer had run before the call"
    got = call(out, produce)
    assert got is out
    torch.cuda.current_stream().synchronize()
    got = out.cpu().numpy()
    assert not (got == hc.SENTINEL).all(), "the late fill landed on top of the result"
    assert hc.same(got, fresh)


@pytest.mark.parametrize("which", ["null", "side"])
@pytest.mark.parametrize("name", OUT_METHODS)
def test_an_out_with_a_pending_writer(ck, env, table, want, name, which):
    case = table[name]
    with _streams(env, which):
        dev = [hc.to_device(x) for x in case.b]
        _pending_out(ck, env, lambda out, produce: case.run(ck, dev, produce=produce, out=out), want(name))


@pytest.mark.parametrize("which", ["null", "side"])
def test_an_out_with_a_pending_writer_and_host_input(ck, env, table, want, which):
    """i420_to_bgr (the one method whose out may lie where its input does not) and jpeg_decode (host streams)"""
    from camkifu_amd import capi
    case = table["i420_to_bgr"]
    streams = ck.jpeg_encode(hc._noise(6, (2, 16, 16, 3)), quality=50, sampling=capi.CK_JPEG_420)
    frames = ck.jpeg_decode(streams)
    assert frames.any()
    with _streams(env, which):
        _pending_out(ck, env, lambda out, produce: case.run(ck, case.b, produce=produce, out=out), want("i420_to_bgr"))
        _pending_out(ck, env, lambda out, produce: (produce(), ck.jpeg_decode(streams, out=out))[1], frames)


@pytest.mark.parametrize("which", ["null", "side"])
@pytest.mark.parametrize("name,fill", [("board_detect_records", 0), ("board_detect_records", hc.SENTINEL), ("cnn_regions_records", 0),
                                       ("cnn_regions_records", hc.SENTINEL)])
def test_record_rows_filled_late(ck, env, table, name, fill, which):
    """round 6 at the level of capi: the rows are zero-filled (or filled with a sentinel) on torch's stream AFTER a delay, the
    library then writes its half of them: the rows hold the records, as rows filled in host memory do"""
    import torch
    case = table[name]
    n = len(case.b[1])
    fresh = hc.norm(case.run(ck, [case.b[0], np.full_like(case.b[1], fill)]))
    blank = np.full_like(fresh, fill)
    assert fresh.shape == blank.shape and (fresh != blank).any()
    with _streams(env, which):
        frames = hc.to_device(case.b[0])
        rows = hc.to_device(np.full_like(case.b[1], 0xEE))
        torch.cuda.current_stream().synchronize()

        def produce():
            env.delay.queue()
            rows.fill_(fill)
            assert not hc.Delay.mark().query(), "bad set-up: the rows were filled before the call"
        got = case.run(ck, [frames, rows], produce=produce)
        assert got is rows and n == len(rows)
        got = hc.norm(got)
    assert not hc.same(got, blank), "the late fill blanked the records"
    assert hc.same(got, fresh)


def _spy_on_fresh_outputs(ck):
    """-> (list that takes (shape, dtype name, data_ptr) of every tensor Context._out_on allocates, undo)"""
    seen, real = [], ck._out_on

    def spy(device, shape, dtype):
        t, p, sp = real(device, shape, dtype)
        seen.append((tuple(t.shape), t.dtype, t.data_ptr()))
        return t, p, sp
    ck._out_on = spy

    def undo():
        del ck._out_on
    return seen, undo


def _recycled(ck, env, call, fresh):
    """the blocks the allocator hands out next carry a late fill_: the method's fresh outputs must be those blocks, and hold the
    result"""
    import torch
    seen, undo = _spy_on_fresh_outputs(ck)
    try:
        first = call(None)
        assert hc.same(hc.norm(first), fresh)
        del first
        layout = [(s, d) for s, d, _ in seen]
        assert layout, "the method allocated no device output"
        del seen[:]
        torch.cuda.current_stream().synchronize()
        noted = []

        def produce():
            blocks = [torch.empty(s, dtype=d, device="cuda:0") for s, d in layout]
            noted.extend(t.data_ptr() for t in blocks)
            env.delay.queue()
            for t in blocks:
                t.fill_(hc.SENTINEL)
            del blocks, t                                         # back to the allocator, their fills still queued
            assert not hc.Delay.mark().query(), "bad set-up: the fills had run before the call"
        got = call(produce)
    finally:
        undo()
    assert [p for _, _, p in seen] == noted, "bad set-up: the method's outputs are not the blocks that carry the late fill"
    assert hc.same(hc.norm(got), fresh)


FRESH_OUT = [m for m in hc.METHODS if m not in ("board_detect", "board_detect_records", "cnn_regions_records", "jpeg_encode",
                                                "jpeg_entropy_encode_device", "overlay_draw", "cnn_set_weights", "train_create", "cnn_maps",
                                                "train_step", "train_grads", "train_apply", "contour_stones", "cluster_stones",
                                                "contours_external", "find_intersections")]        # (those have no device result)


@pytest.mark.parametrize("name", FRESH_OUT)
def test_a_fresh_output_in_a_recycled_block(ck, env, table, want, name):
    case = table[name]
    dev = [hc.to_device(x) for x in case.b]
    _recycled(ck, env, lambda produce: case.run(ck, dev, produce=produce), want(name))


@pytest.mark.parametrize("name", ["median15", "cnn_predict", "harvest_patches"])
def test_a_fresh_output_in_a_recycled_block_on_a_side_stream(ck, env, table, want, name):
    import torch
    case = table[name]
    with torch.cuda.stream(env.side):
        dev = [hc.to_device(x) for x in case.b]
        _recycled(ck, env, lambda produce: case.run(ck, dev, produce=produce), want(name))


@pytest.mark.parametrize("name", ["i420_to_bgr", "i420_to_bgr_levels", "augment_patches", "jpeg_decode", "jpeg_coefficients_device"])
def test_a_to_device_output_in_a_recycled_block(ck, env, table, want, name):
    """host input, the result left in HBM (`to_device=`)"""
    from camkifu_amd import capi
    if name in table:
        case = table[name]
        return _recycled(ck, env, lambda produce: case.run(ck, case.b, produce=produce, to_device="cuda:0"), want(name))
    streams = ck.jpeg_encode(hc._noise(6, (2, 16, 16, 3)), quality=50, sampling=capi.CK_JPEG_420, restart_interval=1)
    if name == "jpeg_decode":
        return _recycled(ck, env, lambda produce: (produce and produce(), ck.jpeg_decode(streams, to_device="cuda:0"))[1], ck.jpeg_decode(streams))
    info, coef, quant = ck.jpeg_coefficients_device(streams)
    _recycled(ck, env, lambda produce: (produce and produce(), list(ck.jpeg_coefficients_device(streams, to_device="cuda:0")))[1], hc.norm([info, coef, quant.view(np.int16)]))


# ---------------------------------------------------------------------------------------------- completeness of results
def _behind_a_delay(ck, env, call):
    """the context is ordered behind a side stream that delays; `call` runs; on return the delay must be over, and a clone of
    every device result, taken at once on a second side stream, must hold what the result holds after a synchronisation"""
    import torch
    torch.cuda.synchronize()
    marks = []

    def produce():
        with torch.cuda.stream(env.side):
            env.delay.queue()
            marks.append(hc.Delay.mark())
        ck.wait_stream(env.side)
        assert not marks[0].query(), "bad set-up: the delay had run out before the call"
    got = call(produce)
    done = marks[0].query()
    with torch.cuda.stream(env.side2):
        snaps = [t.clone() for t in hc.device_tensors(got)]
    torch.cuda.synchronize()
    assert done, "the call returned while its work was still queued behind the delay"
    return got, [s.cpu().numpy() for s in snaps]


def _prefilled(fresh):
    import torch
    out = torch.full(fresh.shape, hc.SENTINEL, dtype=getattr(torch, fresh.dtype.name), device="cuda:0")
    torch.cuda.synchronize()
    return out


def test_results_are_complete_on_return_plain_finish(ck, env, table, want):
    case = table["i420_to_bgr"]
    dev, out = [hc.to_device(x) for x in case.b], _prefilled(want("i420_to_bgr"))
    got, snaps = _behind_a_delay(ck, env, lambda produce: case.run(ck, dev, produce=produce, out=out))
    assert got is out and hc.same(snaps[0], want("i420_to_bgr"))


def test_results_are_complete_on_return_jpeg_passes(ck, env, table, want):
    from camkifu_amd import capi
    frames = hc._noise(6, (3, 16, 16, 3))
    streams = ck.jpeg_encode(frames, quality=50, sampling=capi.CK_JPEG_420)
    decoded = ck.jpeg_decode(streams)
    out = _prefilled(decoded)
    got, snaps = _behind_a_delay(ck, env, lambda produce: (produce(), ck.jpeg_decode(streams, out=out))[1])
    assert got is out and hc.same(snaps[0], decoded)
    dev = hc.to_device(frames)
    got, snaps = _behind_a_delay(ck, env, lambda produce: (produce(), ck.jpeg_encode(dev, quality=50, sampling=capi.CK_JPEG_420))[1])
    assert got == streams
    ck.jpeg_set_encode_entropy("device")
    try:
        got, snaps = _behind_a_delay(ck, env, lambda produce: (produce(), ck.jpeg_encode(dev, quality=50, sampling=capi.CK_JPEG_420))[1])
    finally:
        ck.jpeg_set_encode_entropy("host")
    assert got == streams


def test_results_are_complete_on_return_harvest_exits(ck, env, table, want):
    """ck_harvest_patches leaves after its first finish() with outputs in HBM, after a second one with outputs in host memory"""
    case = table["harvest_patches"]
    fresh = want("harvest_patches")
    assert fresh[3] > 0
    dev = [hc.to_device(x) for x in case.b]
    got, snaps = _behind_a_delay(ck, env, lambda produce: case.run(ck, dev, produce=produce))
    assert hc.same(snaps, fresh[:3]) and got[3] == fresh[3]
    got, snaps = _behind_a_delay(ck, env, lambda produce: case.run(ck, [dev[0], case.b[1]], produce=produce))
    assert hc.same(hc.norm(got), fresh)
    got, snaps = _behind_a_delay(ck, env, lambda produce: case.run(ck, case.b, produce=produce))
    assert snaps == [] and hc.same(hc.norm(got), fresh)


def test_results_are_complete_on_return_cnn_predict(ck, env, table, want):
    case = table["cnn_predict"]
    dev = [hc.to_device(x) for x in case.b]
    got, snaps = _behind_a_delay(ck, env, lambda produce: case.run(ck, dev, produce=produce))
    assert len(snaps) == 3 and hc.same(snaps, want("cnn_predict"))


# --------------------------------------------------------------------------------------------------- the pipeline's rule
@pytest.fixture(scope="module")
def pipe(ck):
    """a real FastFilePipeline as tests/test_gpu_parity.py::test_fast_file_pipeline_on_gpu builds one; board path and background
    model on the module's own context, so that no further HIP stream competes for the four hardware queues"""
    from camkifu_amd import pipeline
    from camkifu_amd.controller import ControllerHeadless
    p = pipeline.FastFilePipeline(96, 128, ControllerHeadless(), ctx=ck, ctx_board=ck, ctx_bg=ck, bg_init_frames=6)
    yield p
    p.close()


class _LateGather:
    """frames in HBM whose gather is slow: index_select queues the delay on the caller's stream, then the real gather -- what a
    producer that is still busy looks like to _take (whose own index upload waits on the host for that stream)"""

    def __init__(self, frames, delay, marks):
        self.frames, self.delay, self.marks = frames, delay, marks
        self.device, self.is_cuda = frames.device, True

    def __getitem__(self, key):
        return self.frames[key]

    def index_select(self, dim, index):
        self.delay.queue()
        out = self.frames.index_select(dim, index)
        self.marks.append(hc.Delay.mark())
        return out


def _on_a_thread(fn):
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as why:                               # noqa: B902  handed to the test's thread
            box["error"] = why
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


@pytest.mark.parametrize("idx", [[1, 2, 3], [0, 2, 3]], ids=["slice", "gather"])
def test_detect_frames_behind_the_callers_side_stream(ck, env, pipe, idx):
    """_detect_frames called from a thread whose current stream is a side stream: frames written late and rows zero-filled late
    there, the lane thread (current stream: the null stream) hands them to the library -- only wait_stream orders the two"""
    import torch
    from camkifu_amd import pipeline
    sa, sb = hc._scenes()
    film_a, film_b = np.concatenate([sa, sa]), np.concatenate([sb, sa])        # four frames; the late content differs from the early one
    marks, seen = [], []
    real = ck.wait_stream

    def spy(stream):
        seen.append([not m.query() for m in marks])
        return real(stream)

    def quiet():
        with torch.cuda.stream(env.side):
            frames, rows = hc.to_device(film_b), pipeline.record_buffer(len(idx), "cuda:0")
            env.side.synchronize()
            got = pipe._detect_frames(frames, idx, rows)
            return got.cpu().numpy()

    def late():
        with torch.cuda.stream(env.side):
            frames, src = hc.to_device(film_a), hc.to_device(film_b)
            rows = hc.to_device(np.full((len(idx), pipeline.REC_BYTES), 0xEE, np.uint8))
            env.side.synchronize()
            env.delay.queue()
            frames.copy_(src)
            rows.zero_()
            marks.append(hc.Delay.mark())
            assert not marks[0].query(), "bad set-up: the producer had run before the call"
            given = frames if idx == [1, 2, 3] else _LateGather(frames, env.delay, marks)
            got = pipe._detect_frames(given, idx, rows)
            return got.cpu().numpy()
    want_rows = _on_a_thread(quiet)
    assert want_rows.any()
    ck.wait_stream = spy
    try:
        got = _on_a_thread(late)
    finally:
        del ck.wait_stream
    assert len(seen) == 1 and seen[0] and seen[0][-1], "bad set-up: nothing was pending when the lane took the tensors: %r" % (seen,)
    assert np.array_equal(got, want_rows)


def test_wait_stream_orders_a_worker_behind_the_producers_stream(ck, env, table):
    """Context.wait_stream itself: the main thread produces frames and rows late on a side stream that is nobody's current
    stream; a worker thread orders the context behind it, then calls board_detect_records"""
    import torch
    case = table["board_detect_records"]
    fresh = hc.norm(case.run(ck, case.b))
    frames, src, rows = hc.to_device(case.a[0]), hc.to_device(case.b[0]), hc.to_device(case.a[1])
    torch.cuda.synchronize()
    with torch.cuda.stream(env.side):
        env.delay.queue()
        frames.copy_(src)
        rows.zero_()
        ev = hc.Delay.mark()
    assert not ev.query(), "bad set-up: the producer had run before the worker started"

    def worker():
        torch.cuda.set_device(0)
        pending = not ev.query()
        ck.wait_stream(env.side)
        return pending, ck.board_detect_records(frames, rows)
    pending, got = _on_a_thread(worker)
    assert pending, "bad set-up: the producer had run before the hand-over"
    assert got is rows and hc.same(hc.norm(got), fresh)

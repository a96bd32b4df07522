"""Hand-over of device memory between torch and the library, checked without a GPU: a stubbed
torch.cuda and a recording stand-in for libck_hip.so.  What must hold structurally:
  * every device tensor crosses the C-ABI through Context._in / Context._out, which order the context's stream behind
    torch's current stream (ck_stream_wait) -- for a fresh output AFTER its allocation;
  * the module-level _in refuses a device tensor (a new call site cannot bypass the ordering by accident);
  * pipeline._take keeps its index tensor alive until its gather has run;
  * Context.close() keeps the handle of a context it could not free."""
import ctypes as C
import types

import numpy as np
import pytest

from camkifu_amd import capi, pipeline
from tests.capi_fakes import FakeLib as _FakeLib, FakeStream as _FakeStream, FakeTensor as _FakeTensor, stub_context


@pytest.fixture
def stub(monkeypatch):
    log = []
    ctx, lib = stub_context(monkeypatch, log)
    yield ctx, log
    ctx._h = C.c_void_p()


def test_a_fresh_output_is_ordered_behind_torch_after_its_allocation(stub):
    ctx, log = stub
    like = _FakeTensor(log, name="input")
    out, ptr, space = ctx._out(like, (2, 19, 19), np.uint8)
    assert space == capi.CK_DEVICE and ptr.value == 0x1000
    assert log[:2] == ["torch.empty", "ck_stream_wait(0x5157)"]          # allocate, THEN order; no host wait
    assert "stream.synchronize" not in log


def test_an_input_is_ordered_behind_torch_without_a_host_wait(stub):
    ctx, log = stub
    ptr, space, keep = ctx._in(_FakeTensor(log, name="input"))
    assert space == capi.CK_DEVICE and log == ["ck_stream_wait(0x5157)"]
    a = np.zeros((4, 4, 3), np.uint8)
    ptr, space, keep = ctx._in(a)                                         # host memory: nothing to order
    assert space == capi.CK_HOST and log.count("ck_stream_wait(0x5157)") == 1 and "stream.synchronize" not in log


def test_the_module_level_helper_refuses_device_memory(stub):
    ctx, log = stub
    with pytest.raises(capi.CkError, match="Context._in"):
        capi._in(_FakeTensor(log))


def test_every_device_pointer_in_capi_goes_through_the_two_helpers():
    """no data_ptr() / torch.empty in capi.py outside Context._in / Context._out_on"""
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(capi))
    offenders = []
    for cls in [n for n in tree.body if isinstance(n, ast.ClassDef)]:
        for fn in [n for n in cls.body if isinstance(n, ast.FunctionDef)]:
            for node in ast.walk(fn):
                hit = isinstance(node, ast.Attribute) and node.attr in ("data_ptr", "empty") and isinstance(node.value, ast.Name)
                if hit and (node.attr == "data_ptr" or node.value.id == "torch"):
                    if (cls.name, fn.name) not in (("Context", "_in"), ("Context", "_out_on")):
                        offenders.append((cls.name, fn.name, node.attr))
    assert not offenders, offenders


def test_take_keeps_its_index_tensor_until_the_gather_has_run(monkeypatch):
    """round 6: no host wait in _take.  The gather is queued on the calling thread's torch stream; _take hands back that
    stream (the consumer -- a lane thread -- orders its context behind it: Context.wait_stream) and parks the index tensor on
    the batch's keep list, which finish() clears once the batch's queued work has run."""
    import torch
    log, keep = [], []

    class Frames:
        device = "cuda:0"

        def index_select(self, dim, index):
            log.append("gather queued")
            return _FakeTensor(log, name="gathered")
    producer = _FakeStream(log, handle=0xBEEF)
    monkeypatch.setattr(torch, "as_tensor", lambda idx, device=None: _FakeTensor(log, name="index"))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: producer)
    out, stream = pipeline._take(Frames(), [0, 3, 4, 9], keep)
    assert stream is producer and len(keep) == 1
    assert log == ["gather queued"], log                                  # no synchronize, the index tensor is alive
    # the consumer: a context ordered behind the producer's stream before the pointer crosses the C-ABI
    lib = _FakeLib(log)
    monkeypatch.setattr(capi, "lib", lambda: lib)
    ctx = capi.Context.__new__(capi.Context)
    ctx._h, ctx.device = C.c_void_p(7), 0
    ctx.wait_stream(stream)
    assert log[-1] == "ck_stream_wait(0xbeef)"
    ctx._h = C.c_void_p()
    keep.clear()                                                          # what finish() does
    assert log[-1] == "free index"
    del out
    # consecutive frames are a view: no gather, nothing to wait for
    log.clear()
    fr = np.arange(10)
    part, stream = pipeline._take(fr, [2, 3, 4])
    assert part.tolist() == [2, 3, 4] and stream is None and log == []


def test_a_lane_is_ordered_behind_the_callers_stream_whether_or_not_take_gathered(monkeypatch):
    """The hand-over rule of FastFilePipeline._detect_frames.  One lane, three consecutive frames (_take gathers nothing and
    names no stream), record rows in HBM that the caller allocated on ITS current stream (the exchange thread's): the lane's
    context is ordered behind that stream -- not behind the lane thread's own -- before the library writes the rows.  The
    same for device frames with host rows; with host rows and host frames nothing is ordered at all."""
    import threading
    from concurrent.futures import ThreadPoolExecutor
    import torch
    log, callers = [], []
    xstream, other = _FakeStream(log, handle=0xE8), _FakeStream(log, handle=0xD0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: xstream if threading.get_ident() in callers else other)

    class Lane:
        def wait_stream(self, stream):
            log.append("wait_stream(0x%x)" % stream.cuda_stream)

        def board_detect_records(self, frames, rows):
            log.append("board_detect_records")
            return rows

    class OnDevice(_FakeTensor):
        def __getitem__(self, key):
            return self

        def __len__(self):
            return self.shape[0]
    lane_thread, exchange_thread = ThreadPoolExecutor(1), ThreadPoolExecutor(1)
    pipe = pipeline.FastFilePipeline.__new__(pipeline.FastFilePipeline)
    pipe.compute, pipe.host_seconds = types.SimpleNamespace(lanes=[(Lane(), None)], pools=[(lane_thread, None)]), {}

    def detect(frames, rows):
        callers.append(threading.get_ident())
        pipe._detect_frames(frames, [4, 5, 6], rows)
        seen = [entry for entry in log if not entry.startswith("free")]
        log.clear()
        return seen
    host_frames, host_rows = np.zeros((10, 4, 4, 3), np.uint8), np.zeros(3, pipeline.REC)
    try:
        for frames, rows in ((host_frames, OnDevice(log, (3, pipeline.REC_BYTES), "rows")),
                             (OnDevice(log, (10, 4, 4, 3), "frames"), host_rows)):
            assert exchange_thread.submit(detect, frames, rows).result() == ["wait_stream(0xe8)", "board_detect_records"]
        assert exchange_thread.submit(detect, host_frames, host_rows).result() == ["board_detect_records"]
    finally:
        lane_thread.shutdown()
        exchange_thread.shutdown()


def test_no_host_wait_is_left_in_the_pipeline():
    """the only synchronize() in pipeline.py is the exchange thread's final drain of its own stream"""
    import inspect
    import re
    src = inspect.getsource(pipeline)
    calls = [m.start() for m in re.finditer(r"\.synchronize\(\)", src)]
    assert len(calls) == 1 and "self._xstream.synchronize()" in src


def test_close_keeps_the_handle_of_a_context_it_could_not_free(monkeypatch):
    log = []
    busy = _FakeLib(log, destroy_rc=capi.CK_ERR_STATE if hasattr(capi, "CK_ERR_STATE") else 5)
    monkeypatch.setattr(capi, "lib", lambda: busy)
    ctx = capi.Context.__new__(capi.Context)
    ctx._h, ctx.device = C.c_void_p(7), 0
    with pytest.raises(capi.CkError, match="not freed"):
        ctx.close()
    assert ctx._h.value == 7                                              # still there: a later close() can retry
    busy.destroy_rc = 0
    ctx.close()
    assert not ctx._h and log == ["ck_ctx_destroy2", "ck_ctx_destroy2"]

"""Stand-ins for checking camkifu_amd.capi without a GPU: a torch.cuda stream, a device tensor and a libck_hip.so that only
record what is done to them.  The log is a list of strings; `calls` of the library holds (name, args) of every ck_* call."""
import ctypes as C

import numpy as np


class FakeStream:
    def __init__(self, log, handle=0x5157):
        self.log, self.cuda_stream = log, handle

    def synchronize(self):
        self.log.append("stream.synchronize")


class FakeTensor:
    """what capi reads of a tensor in HBM; `dtype` prints like torch's"""
    is_cuda, device = True, "cuda:0"

    def __init__(self, log, shape=(2, 4, 4, 3), name="tensor", dtype=np.uint8, contiguous=True, ptr=0x1000):
        self.log, self.shape, self.name, self.ptr = log, tuple(shape), name, ptr
        self.dtype, self._contiguous = "torch." + np.dtype(dtype).name, contiguous

    def is_contiguous(self):
        return self._contiguous

    def contiguous(self):
        return self

    def data_ptr(self):
        return self.ptr

    def __del__(self):
        self.log.append("free " + self.name)


FakeTensor.__module__ = "torch"


class FakeLib:
    """every ck_* entry point succeeds and is recorded; nothing is computed"""
    QUIET = ("ck_stream_wait", "ck_last_error", "ck_ctx_destroy2", "ck_jpeg_probe")          # not compute calls

    def __init__(self, log, destroy_rc=0):
        self.log, self.destroy_rc, self.calls = log, destroy_rc, []

    def ck_stream_wait(self, h, stream):
        self.log.append("ck_stream_wait(0x%x)" % stream.value)
        return 0

    def ck_ctx_destroy2(self, h):
        self.log.append("ck_ctx_destroy2")
        return self.destroy_rc

    def ck_last_error(self, h):
        return b""

    def ck_jpeg_probe(self, data, size, info):
        """every stream is a 16 x 16 frame, 4:2:0"""
        info._obj.h, info._obj.w, info._obj.sampling, info._obj.blocks = 16, 16, 3, 6
        return 0

    def __getattr__(self, name):
        if not name.startswith("ck_"):
            raise AttributeError(name)

        def call(*args):
            self.log.append(name)
            self.calls.append((name, args))
            return 0
        return call


def stub_context(monkeypatch, log, lib=None):
    """a Context that was never created, over a FakeLib, with torch.cuda's stream and torch.empty replaced -> (ctx, lib);
    the caller clears ctx._h when it is done (the finaliser would otherwise free handle 1)"""
    import torch
    from camkifu_amd import capi
    lib = FakeLib(log) if lib is None else lib
    monkeypatch.setattr(capi, "lib", lambda: lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: FakeStream(log))

    def empty(shape, dtype=None, device=None):
        log.append("torch.empty")
        return FakeTensor(log, shape, "output", dtype=str(dtype).replace("torch.", ""))
    monkeypatch.setattr(torch, "empty", empty)
    ctx = capi.Context.__new__(capi.Context)
    ctx._h, ctx.device, ctx._mog2_shape = C.c_void_p(1), 0, {}
    return ctx, lib

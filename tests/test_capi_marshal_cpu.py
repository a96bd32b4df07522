"""What capi.py lets across the C-ABI, checked without a GPU over a recording stand-in for the library (tests/capi_fakes.py):
an array whose size or element type the library would take on trust is refused BEFORE any compute call, a caller's `out`
is handed over as it lies (its own pointer, never a converted copy), and device memory is ordered behind torch's stream
first.  A lost check costs a failed assertion here; on a GPU it would cost an out-of-bounds access by a kernel."""
import ast
import ctypes as C
import inspect

import numpy as np
import pytest

from camkifu_amd import capi
from tests.capi_fakes import FakeTensor, stub_context

REFUSED = (capi.CkError, ValueError)


@pytest.fixture
def stub(monkeypatch):
    log = []
    ctx, lib = stub_context(monkeypatch, log)
    ctx._mog2_shape[3] = (40, 60)                       # a 40 x 60 background model under handle 3
    yield ctx, lib, log
    ctx._h = C.c_void_p()


def _arr(shape, dtype=np.uint8, device=None, **kw):
    """zeros in host memory, or (device = the log) a fake tensor in HBM"""
    return np.zeros(shape, dtype) if device is None else FakeTensor(device, shape, dtype=dtype, ptr=0x3000, **kw)


def _refused(lib, call):
    with pytest.raises(REFUSED):
        call()
    assert lib.calls == []                              # nothing reached the library


# ---- refusals: inputs ------------------------------------------------------------------------------------------------
def test_a_device_tensor_of_another_element_type_or_layout_is_refused(stub):
    ctx, lib, log = stub
    _refused(lib, lambda: ctx.median15(_arr((2, 8, 8, 3), np.float32, log)))
    _refused(lib, lambda: ctx.median15(_arr((2, 8, 8, 3), np.uint8, log, contiguous=False)))
    half = {k: _arr(capi.WEIGHT_SHAPES[k], np.float16, log) for k in capi.WEIGHT_ORDER}
    _refused(lib, lambda: ctx.train_create(half))
    _refused(lib, lambda: ctx.cnn_set_weights(half))
    counts = _arr((1, 19, 19), np.int64, log)           # torch's default for counts: the library would read int32 pairs
    _refused(lib, lambda: ctx.harvest_patches(_arr((1, 380, 380, 3)), counts, [0], _arr((1, 19, 19))))


@pytest.mark.parametrize("space", ["host", "device"])
def test_a_goban_image_or_mask_of_another_size_is_refused(stub, space):
    ctx, lib, log = stub
    dev = log if space == "device" else None
    goban = _arr((1, 379, 380, 3), device=dev)
    _refused(lib, lambda: ctx.cnn_predict(goban))
    _refused(lib, lambda: ctx.cnn_regions(goban))
    _refused(lib, lambda: ctx.cnn_maps(goban))
    _refused(lib, lambda: ctx.cnn_regions_records(goban, np.zeros(1, capi.REC_DTYPE)))
    _refused(lib, lambda: ctx.zone_counts(_arr((2, 380, 379), device=dev)))
    _refused(lib, lambda: ctx.i420_to_bgr(_arr((2, 16 * 24 * 3 // 2 - 1), device=dev), 16, 24))


@pytest.mark.parametrize("space", ["host", "device"])
def test_the_background_model_sets_the_size_of_what_it_is_given(stub, space):
    ctx, lib, log = stub
    dev = log if space == "device" else None
    _refused(lib, lambda: ctx.mog2_apply(3, _arr((40, 61, 3), device=dev), 0.01))
    _refused(lib, lambda: ctx.mog2_band_run(3, _arr((2, 39, 60, 3), device=dev), [0.01, 0.01], False))
    # a handle the context never created: no size is known, so none is taken on trust
    with pytest.raises(capi.CkError, match="bad mog2 handle 9"):
        ctx.mog2_apply(9, _arr((40, 60, 3), device=dev), 0.01)
    with pytest.raises(capi.CkError, match="bad mog2 handle 9"):
        ctx.mog2_band_run(9, _arr((2, 40, 60, 3), device=dev), [0.01, 0.01], False)
    assert lib.calls == []
    ctx.mog2_apply(3, _arr((40, 60, 3), device=dev), 0.01)
    out = ctx.mog2_band_run(3, _arr((2, 40, 60, 3), device=dev), [0.01, 0.01], False)
    assert [c[0] for c in lib.calls] == ["ck_mog2_apply", "ck_mog2_band_run"] and tuple(out.shape) == (2, 2, 19)


# ---- the seven methods that fill a caller's `out` ------------------------------------------------------------------------
M = [[1.0, 0.1, 0.5], [0.0, 1.2, 0.25], [0.0, 0.001, 1.0]]


def _out_methods():
    """name -> (entry point, shape and dtype of a valid out, call(ctx, out, device or None))"""
    f = lambda shape, dtype=np.uint8: (lambda dev: _arr(shape, dtype, dev))
    frames, patches, small = f((2, 16, 24, 3)), f((3, 40, 40, 3)), f((2, 16, 16, 3))
    quant1 = np.ones((3, 64), np.uint16)
    return {
        "i420_to_bgr": ("ck_i420_to_bgr", (2, 16, 24, 3), np.uint8,
                        lambda ctx, out, dev: ctx.i420_to_bgr(_arr((2, 16 * 24 * 3 // 2), device=dev), 16, 24, out=out)),
        "pyr_down": ("ck_pyr_down", (2, 8, 12, 3), np.uint8, lambda ctx, out, dev: ctx.pyr_down(frames(dev), 1, out=out)),
        "warp_perspective": ("ck_warp_perspective", (2, 8, 8, 3), np.uint8,
                             lambda ctx, out, dev: ctx.warp_perspective(frames(dev), M, dsize=8, out=out)),
        "augment_patches": ("ck_augment_patches", (3, 40, 40, 3), np.uint8,
                            lambda ctx, out, dev: ctx.augment_patches(patches(dev), [0, 1, 6], out=out)),
        "jpeg_forward": ("ck_jpeg_forward", (2, 6 * 64), np.int16,
                         lambda ctx, out, dev: ctx.jpeg_forward(small(dev), quant1, capi.CK_JPEG_420, out=out)),
        "jpeg_reconstruct": ("ck_jpeg_reconstruct", (2, 16, 16, 3), np.uint8,
                             lambda ctx, out, dev: ctx.jpeg_reconstruct(_arr((2, 6 * 64), np.int16, dev), _arr((2, 3, 64), np.uint16, dev),
                                                                        16, 16, capi.CK_JPEG_420, out=out)),
        "jpeg_decode": ("ck_jpeg_decode", (2, 16, 16, 3), np.uint8, lambda ctx, out, dev: ctx.jpeg_decode([b"\xff\xd8", b"\xff\xd8"], out=out)),
    }


OUT_METHODS = _out_methods()


def _bad_out(kind, shape, dtype, dev):
    other = np.int16 if dtype == np.uint8 else np.uint8
    if kind == "dtype":
        return _arr(shape, other, dev)
    if kind == "shape":
        return _arr((shape[0] + 1,) + shape[1:], dtype, dev)
    if kind == "strided":
        return _arr(shape, dtype, dev, contiguous=False) if dev is not None else np.zeros(shape[:-1] + (2 * shape[-1],), dtype)[..., ::2]
    out = np.zeros(shape, dtype)
    out.flags.writeable = False
    return out


@pytest.mark.parametrize("kind,space", [(k, s) for k in ("dtype", "strided", "shape", "readonly") for s in ("host", "device")
                                        if (k, s) != ("readonly", "device")])
@pytest.mark.parametrize("name", sorted(OUT_METHODS))
def test_an_out_the_library_could_not_fill_in_place_is_refused(stub, name, kind, space):
    """(each of these used to be converted into a temporary that took the result, or was guarded by an assert at best)"""
    ctx, lib, log = stub
    entry, shape, dtype, call = OUT_METHODS[name]
    dev = log if space == "device" else None
    bad = _bad_out(kind, shape, dtype, dev)
    _refused(lib, lambda: call(ctx, bad, dev))
    if dev is None:
        assert not bad.any()


def test_warp_refuses_an_out_in_the_other_memory_space(stub):
    ctx, lib, log = stub
    with pytest.raises(capi.CkError, match="where the frames live"):
        ctx.warp_perspective(_arr((2, 16, 24, 3)), M, dsize=8, out=_arr((2, 8, 8, 3), device=log))
    with pytest.raises(capi.CkError, match="where the frames live"):
        ctx.warp_perspective(_arr((2, 16, 24, 3), device=log), M, dsize=8, out=_arr((2, 8, 8, 3)))
    assert lib.calls == []


# ---- hand-over ---------------------------------------------------------------------------------------------------------
def _pointers(args):
    return [a.value for a in args if isinstance(a, C.c_void_p)]


@pytest.mark.parametrize("name", sorted(OUT_METHODS))
def test_a_numpy_out_is_handed_over_as_it_lies(stub, name):
    ctx, lib, log = stub
    entry, shape, dtype, call = OUT_METHODS[name]
    out = np.zeros(shape, dtype)
    assert call(ctx, out, None) is out
    (got, args), = lib.calls
    assert got == entry and out.ctypes.data in _pointers(args)
    assert "ck_stream_wait(0x5157)" not in log                              # host memory: nothing to order


@pytest.mark.parametrize("name", sorted(OUT_METHODS))
def test_a_device_out_is_its_own_pointer_ordered_behind_torch(stub, name):
    ctx, lib, log = stub
    entry, shape, dtype, call = OUT_METHODS[name]
    out = FakeTensor(log, shape, "out", dtype=dtype, ptr=0x7000)
    assert call(ctx, out, log) is out
    (got, args), = lib.calls
    assert got == entry and 0x7000 in _pointers(args)
    if name != "jpeg_decode":                                               # (its streams are host memory)
        assert 0x3000 in _pointers(args)
    waits = [i for i, line in enumerate(log) if line == "ck_stream_wait(0x5157)"]
    assert len(waits) == (1 if name == "jpeg_decode" else 3 if name == "jpeg_reconstruct" else 2) and max(waits) < log.index(entry)
    assert "torch.empty" not in log and "stream.synchronize" not in log


def test_a_fresh_device_output_follows_to_device(stub):
    ctx, lib, log = stub
    out = ctx.i420_to_bgr(np.zeros((2, 16 * 24 * 3 // 2), np.uint8), 16, 24, to_device="cuda:0")
    assert isinstance(out, FakeTensor) and out.shape == (2, 16, 24, 3) and out.dtype == "torch.uint8"
    assert log[:3] == ["torch.empty", "ck_stream_wait(0x5157)", "ck_i420_to_bgr"]


# ---- structure -----------------------------------------------------------------------------------------------------------
def test_no_assert_guards_an_argument_in_capi():
    """python -O strips asserts: what crosses the ABI is checked by statements that stay"""
    tree = ast.parse(inspect.getsource(capi))
    assert [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)] == []

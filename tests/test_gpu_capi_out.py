"""A caller's `out=` really takes the result: for the methods that fill a preallocated array, the object comes back, and
holds byte for byte what the call without `out` returns -- once with an ndarray, once with a tensor in HBM.  What capi.py
REFUSES is checked over a stand-in library (tests/test_capi_marshal_cpu.py), never here: a lost check would hand a kernel
a pointer to too little memory.  pyr_down, jpeg_decode, jpeg_forward and augment_patches have this comparison next to
their references (test_gpu_pyr.py, test_gpu_jpeg.py, test_gpu_jpeg_enc.py, test_gpu_harvest.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = np.array([[1.1, 0.2, -1.5], [-0.1, 0.9, 2.25], [0.002, -0.001, 1.0]])           # fixed, not the identity


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _calls(ck):
    """name -> (call(out=None) for host inputs, call for the same inputs in HBM)"""
    import torch
    from camkifu_amd import capi
    rng = np.random.default_rng(16)
    dev = lambda a: torch.from_numpy(a).cuda()
    i420 = rng.integers(0, 256, (2, 16 * 24 * 3 // 2), dtype=np.uint8)
    frames = rng.integers(0, 256, (2, 16, 24, 3), dtype=np.uint8)
    noise = rng.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8)
    info, coef, quant = capi.jpeg_coefficients(ck.jpeg_encode(noise, quality=90, sampling=capi.CK_JPEG_420))
    assert (info["h"], info["w"], info["sampling"]) == (16, 16, capi.CK_JPEG_420)
    quant = quant.view(np.int16) if not hasattr(torch, "uint16") else quant                # (the bits count)
    d_i420, d_frames, d_coef, d_quant = dev(i420), dev(frames), dev(coef), dev(quant)
    return {
        "i420_to_bgr": (lambda **kw: ck.i420_to_bgr(i420, 16, 24, **kw), lambda **kw: ck.i420_to_bgr(d_i420, 16, 24, **kw)),
        "i420_to_bgr_level_1": (lambda **kw: ck.i420_to_bgr(i420, 16, 24, levels=1, **kw),
                                lambda **kw: ck.i420_to_bgr(d_i420, 16, 24, levels=1, **kw)),
        "warp_perspective": (lambda **kw: ck.warp_perspective(frames, M, dsize=8, **kw),
                             lambda **kw: ck.warp_perspective(d_frames, M, dsize=8, **kw)),
        "jpeg_reconstruct": (lambda **kw: ck.jpeg_reconstruct(coef, quant, 16, 16, capi.CK_JPEG_420, **kw),
                             lambda **kw: ck.jpeg_reconstruct(d_coef, d_quant, 16, 16, capi.CK_JPEG_420, **kw)),
    }


@pytest.mark.parametrize("name", ["i420_to_bgr", "i420_to_bgr_level_1", "warp_perspective", "jpeg_reconstruct"])
def test_out_takes_what_the_call_without_it_returns(ck, name):
    import torch
    host, device = _calls(ck)[name]
    want = host()
    assert isinstance(want, np.ndarray) and want.any()
    out = np.zeros_like(want)
    assert host(out=out) is out and np.array_equal(out, want)
    plain = device()
    assert plain.is_cuda and np.array_equal(plain.cpu().numpy(), want)
    out = torch.zeros_like(plain)
    assert device(out=out) is out and np.array_equal(out.cpu().numpy(), want)
    if name.startswith("i420"):                                  # the one method whose out may lie where the input does not
        out = torch.zeros_like(plain)
        assert host(out=out) is out and np.array_equal(out.cpu().numpy(), want)

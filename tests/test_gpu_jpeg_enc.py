"""The JPEG encoder on the GPU: the forward kernel against the coefficients the decoder's reference reads out of Pillow's
bytes and against the numpy reference, every int16; whole streams against the committed Pillow bytes; the tools."""
import importlib.util
import os

import numpy as np
import pytest

from . import jpeg_cases
from . import jpeg_enc_cases as cases
from . import jpeg_enc_ref as ref
from . import jpeg_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _expect_forward(case):
    """the reference's coefficients, which are also what the decoder's reference reads out of the golden"""
    exp = cases.ref_forward(case)
    assert np.array_equal(jpeg_ref.coefficients(cases.golden(case))[1], exp)
    return exp


@pytest.mark.parametrize("shape", cases.SHAPES, ids=["%dx%d" % s for s in cases.SHAPES])
def test_forward_equals_the_goldens_coefficients(ck, shape):
    """all four samplings at quality 1, 50, 90 and 100; host memory and HBM in turn"""
    import torch
    dev = torch.device("cuda:0")
    for k, case in enumerate(c for c in cases.forward_cases() if c[1:3] == shape):
        img, q = cases.case_image(case), ref.quant_tables(case[4])
        exp = _expect_forward(case)
        if k & 1:
            got = ck.jpeg_forward(torch.from_numpy(np.array(img)).to(dev), q, case[3]).cpu().numpy()
        else:
            got = ck.jpeg_forward(img, q, case[3])
        assert got.dtype == np.int16 and got.shape == (1, exp.size)
        assert np.array_equal(got[0], exp), cases.name_of(case)


@pytest.mark.parametrize("s", cases.SAMPLINGS)
def test_forward_of_a_batch_from_host_memory_and_from_hbm(ck, s):
    """three frames of 17 x 33: frames 1 and 2 start off a dword (1683 bytes each); the call again after one of another size"""
    import torch
    frames = np.stack([cases.image(cases.CONTENTS[k], 17, 33, seed=k) for k in range(3)])
    q = ref.quant_tables(90)
    exp = np.stack([ref.forward(f, q, s) for f in frames])
    got = ck.jpeg_forward(frames, q, s)
    assert np.array_equal(got, exp)
    other = cases.forward_case(33, 70, s, 50)
    assert np.array_equal(ck.jpeg_forward(cases.case_image(other), ref.quant_tables(50), s)[0], cases.ref_forward(other))
    dev = torch.device("cuda:0")
    d = ck.jpeg_forward(torch.from_numpy(frames).to(dev), q, s)
    assert d.is_cuda and np.array_equal(d.cpu().numpy(), exp)
    assert np.array_equal(ck.jpeg_forward(frames, q, s), exp)
    # a batch in HBM that itself starts off a dword
    flat = torch.zeros(frames.size + 1, dtype=torch.uint8, device=dev)
    flat[1:] = torch.from_numpy(frames).to(dev).reshape(-1)
    assert np.array_equal(ck.jpeg_forward(flat[1:].view(3, 17, 33, 3), q, s).cpu().numpy(), exp)
    if s == ref.S420:                                         # rows on dwords (w % 4 == 0) in a batch that is not: the byte path
        wide = np.stack([cases.image("noise", 16, 32, seed=k) for k in range(2)])
        flat = torch.zeros(wide.size + 2, dtype=torch.uint8, device=dev)
        flat[2:] = torch.from_numpy(wide).to(dev).reshape(-1)
        assert np.array_equal(ck.jpeg_forward(flat[2:].view(2, 16, 32, 3), q, s).cpu().numpy(), np.stack([ref.forward(f, q, s) for f in wide]))
    # into a preallocated output
    out = np.empty_like(exp)
    assert ck.jpeg_forward(frames, q, s, out=out) is out and np.array_equal(out, exp)
    out = torch.zeros_like(d)
    assert ck.jpeg_forward(torch.from_numpy(frames).to(dev), q, s, out=out) is out and np.array_equal(out.cpu().numpy(), exp)


def test_a_batch_equals_per_frame_calls(ck):
    case = cases.BATCH[0]
    frames = np.stack([cases.case_image(case, seed) for seed in range(5)])
    q = ref.quant_tables(case[4])
    got = ck.jpeg_forward(frames, q, case[3])
    for f in range(5):
        assert np.array_equal(got[f], ck.jpeg_forward(frames[f], q, case[3])[0])
        assert np.array_equal(got[f], cases.ref_forward(case, f))
    assert ck.jpeg_encode(frames, quality=case[4], sampling=case[3]) == [cases.golden(case, seed) for seed in range(5)]


@pytest.mark.parametrize("part", range(4))
def test_encode_equals_pillows_bytes(ck, part):
    """every committed case, restart intervals included; host memory and HBM in turn"""
    import torch
    dev = torch.device("cuda:0")
    for k, case in enumerate(cases.all_cases()[part::4]):
        img = cases.case_image(case)
        src = torch.from_numpy(np.array(img)).to(dev) if k & 1 else img
        out = ck.jpeg_encode(src, quality=case[4], sampling=case[3], restart_interval=case[5])
        assert isinstance(out, list) and len(out) == 1 and isinstance(out[0], bytes)
        assert out[0] == cases.golden(case), cases.name_of(case)


def test_encode_in_several_passes(ck, monkeypatch):
    """the pass size as the decoder's tests set it: 5 frames of 136 x 200 take one frame per pass"""
    case = cases.BATCH[0]
    frames = np.stack([cases.case_image(case, seed) for seed in range(5)])
    monkeypatch.setenv("CK_JPEG_PASS_BYTES", "70000")
    assert ck.jpeg_encode(frames, quality=case[4], sampling=case[3]) == [cases.golden(case, seed) for seed in range(5)]


def test_decode_of_encode_equals_the_reference_decode(ck):
    for case in cases.all_cases()[3::11]:
        data = ck.jpeg_encode(cases.case_image(case), quality=case[4], sampling=case[3], restart_interval=case[5])
        assert np.array_equal(ck.jpeg_decode(data)[0], jpeg_ref.decode(cases.golden(case))), cases.name_of(case)


def test_argument_errors_name_the_cause(ck):
    import ctypes as C
    from camkifu_amd import capi
    img = np.zeros((1, 8, 8, 3), np.uint8)
    q = capi.jpeg_quant(90)
    with pytest.raises(capi.CkError, match="sampling") as e:
        ck.jpeg_forward(img, q, 4)
    with pytest.raises(capi.CkError, match="sampling") as e:
        ck.jpeg_encode(img, sampling=9)
    assert e.value.code == capi.CK_ERR_ARG
    with pytest.raises(capi.CkError, match="restart interval") as e:
        ck.jpeg_encode(img, restart_interval=65536)
    assert e.value.code == capi.CK_ERR_ARG
    bad = q.copy()
    bad[2, 63] = 256
    with pytest.raises(capi.CkError, match="quant entry 191") as e:
        ck.jpeg_forward(img, bad, capi.CK_JPEG_420)
    assert e.value.code == capi.CK_ERR_ARG
    with pytest.raises(capi.CkError, match="frames"):
        ck.jpeg_encode(np.zeros((1, 8, 8, 4), np.uint8))
    with pytest.raises(capi.CkError, match="frames"):
        ck.jpeg_forward(np.zeros((1, 8, 8, 3), np.float32), q)
    # sizes outside 1 .. 65535 and a buffer below the bound: refused by the library before anything is read
    L = capi.lib()
    out, ln = np.zeros(4096, np.uint8), (C.c_size_t * 1)()
    pimg, pout = img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for h, w in ((0, 8), (8, 65536), (65536, 8)):
        assert L.ck_jpeg_encode(ck._h, pimg, 1, h, w, capi.CK_HOST, 90, capi.CK_JPEG_420, 0, pout, 1 << 40, ln) == capi.CK_ERR_ARG
        assert b"frame size" in L.ck_last_error(ck._h)
    bound = capi.jpeg_encode_bound(8, 8, capi.CK_JPEG_420)
    assert L.ck_jpeg_encode(ck._h, pimg, 1, 8, 8, capi.CK_HOST, 90, capi.CK_JPEG_420, 0, pout, bound - 1, ln) == capi.CK_ERR_ARG
    assert b"smaller than the bound" in L.ck_last_error(ck._h) and not out.any()
    # and the context still works
    assert ck.jpeg_encode(img)[0] == ref.encode(img[0], 90, ref.S420)


def test_write_jpeg_and_jpg_snapshot_on_the_gpu(ck, tmp_path):
    import torch
    from camkifu_amd.core import capture
    img = cases.image("ramp", 380, 380)
    path = str(tmp_path / "goban.jpg")
    capture.write_jpeg(path, torch.from_numpy(img).to("cuda:0"), quality=95, sampling=ref.S444, encode=ck.jpeg_encode)
    with open(path, "rb") as f:
        data = f.read()
    assert data == ref.encode(img, 95, ref.S444)
    cap = capture.ImageCapture(path, decode=ck.jpeg_decode)
    assert cap.isOpened() and np.array_equal(cap.read()[1], jpeg_ref.decode(data))


# ---- tools/transcode.py -----------------------------------------------------------------------------------------------------
def test_transcode_of_an_avi_and_of_an_array(ck, tmp_path):
    from camkifu_amd.core import capture
    tr = _tool("transcode")
    # tests/golden/tiny.avi: every chunk's picture (a repeat shows the previous one), encoded again
    idx, frames = jpeg_cases.avi_reference()
    out = str(tmp_path / "again.avi")
    res = tr.transcode(jpeg_cases.AVI, out, quality=85, sampling=ref.S422, batch=3, ctx=ck)
    cap = capture.AviMjpegCapture(out, decode=ck.jpeg_decode)
    assert cap.isOpened() and len(cap) == res["frames"] == len(frames) and cap.damaged == 0 and cap.fps == idx["fps"]
    for k, fr in enumerate(frames):
        ok, img = cap.read()
        assert ok and np.array_equal(img, jpeg_ref.decode(ref.encode(fr, 85, ref.S422))), k
    # a 12-frame 64 x 48 array, batches of 5
    film = np.stack([cases.image(cases.CONTENTS[k % 4], 48, 64, seed=k) for k in range(12)])
    out2 = str(tmp_path / "array.avi")
    res = tr.transcode(film, out2, batch=5, ctx=ck)
    cap = capture.AviMjpegCapture(out2, decode=ck.jpeg_decode)
    assert (res["frames"], res["h"], res["w"]) == (12, 48, 64) and len(cap) == 12 and cap.fps == 30.0
    with open(out2, "rb") as f:
        chunks = jpeg_ref.avi_index(f.read())["chunks"]
    for k in range(12):
        assert chunks[k] == ref.encode(film[k], 90, ref.S420)
        assert np.array_equal(cap.read()[1], jpeg_ref.decode(chunks[k]))


def test_recording_the_gobans_leaves_the_game_record_alone(ck, tmp_path):
    """the 100-frame film of test_fast_file_pipeline_on_gpu: one 380 x 380 frame per processed frame, black until the board
    is found, the goban images after that; the record equals the one of a run that records nothing"""
    from camkifu_amd import pipeline, synth
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture
    from camkifu_amd.stone.nn_manager import NNManager
    tr = _tool("transcode")
    frames = synth.film(100, 480, 640, seed=8, quiet=8, move_every=30, hand_frames=12)[0].numpy()
    ck.cnn_set_weights(NNManager.init_net())
    plain = ControllerHeadless()
    with pipeline.FastFilePipeline(480, 640, plain, ctx=ck, bg_init_frames=6) as pipe:
        want = []
        for b0 in range(0, 100, 23):
            want += pipe.process_batch(frames[b0:b0 + 23], len(frames[b0:b0 + 23]))
    out = str(tmp_path / "gobans.avi")
    res = tr.record_gobans(frames, out, quality=90, batch=23, ctx=ck, bg_init_frames=6)
    assert res["requests"] == want and res["controller"].kifu.to_sgf() == plain.kifu.to_sgf() and len(plain.kifu.moves) > 0
    cap = capture.AviMjpegCapture(out, decode=ck.jpeg_decode)
    assert cap.isOpened() and len(cap) == res["frames"] == 100 and (cap.h, cap.w) == (380, 380) and cap.damaged == 0
    assert not cap.read()[1].any()                            # the first batch had no transform yet
    cap.set(capture.CAP_PROP_POS_FRAMES, 99)
    last = cap.read()[1]
    assert last.shape == (380, 380, 3) and last.std() > 10    # a picture of a board, not a flat frame

"""Baseline JPEG decode on the GPU (csrc/k_jpeg.hip behind ck_jpeg_decode / ck_jpeg_reconstruct) against Pillow's committed
decodes and the numpy reference (tests/jpeg_ref.py), bit for bit; the MJPEG capture and process_mjpeg end to end."""
import io

import numpy as np
import pytest

from . import jpeg_cases, jpeg_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("part", range(4))
def test_every_case_decodes_to_pillows_bytes(ck, part):
    """n = 1, host output and device output in turn"""
    import torch
    cases = jpeg_cases.file_cases()
    dev = torch.device("cuda:0")
    for k, name in enumerate(jpeg_cases.names(4, part)):
        data, exp = cases[name]
        if k & 1:
            got = ck.jpeg_decode([data], to_device=dev)
            assert got.is_cuda
            got = got.cpu().numpy()
        else:
            got = ck.jpeg_decode([data])
        assert got.shape == (1,) + exp.shape and np.array_equal(got[0], exp), name


def test_the_batch_of_five_decodes_in_one_call(ck):
    import torch
    streams, exp = jpeg_cases.batch_case()
    assert np.array_equal(ck.jpeg_decode(streams), exp)                                       # -> host
    dev = ck.jpeg_decode(streams, to_device=torch.device("cuda:0"))                          # -> HBM
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), exp)
    out = np.zeros_like(exp)
    assert ck.jpeg_decode([np.frombuffer(s, np.uint8) for s in streams], out=out) is out and np.array_equal(out, exp)
    out = torch.zeros_like(dev)
    assert ck.jpeg_decode(streams, out=out) is out and np.array_equal(out.cpu().numpy(), exp)
    ck.timing_enable(True)
    ck.timing_reset()
    ck.jpeg_decode(streams)
    ms, launches = ck.timing_get("jpeg")
    ck.timing_enable(False)
    assert launches == 1 and ms > 0


def test_a_batch_larger_than_one_pass_decodes_in_several(ck, monkeypatch):
    """ck_jpeg_decode stages the coefficients of about 256 MB of frames at a time; with the budget at two frames the batch
    of five goes through in three passes, and a damaged frame of the last pass keeps its number in the batch"""
    import torch
    from camkifu_amd import capi
    streams, exp = jpeg_cases.batch_case()
    info = capi.jpeg_probe(streams[0])
    monkeypatch.setenv("CK_JPEG_PASS_BYTES", str(2 * (info["blocks"] * 128 + 384) + 100))
    assert np.array_equal(ck.jpeg_decode(streams), exp)
    dev = ck.jpeg_decode(streams, to_device=torch.device("cuda:0"))
    assert np.array_equal(dev.cpu().numpy(), exp)
    with pytest.raises(capi.CkError, match=r"frame 4: ") as e:
        ck.jpeg_decode(streams[:4] + [streams[4][:len(streams[4]) // 2]])
    assert e.value.bad_frame == 4
    monkeypatch.setenv("CK_JPEG_PASS_BYTES", "1")                                             # one frame per pass
    assert np.array_equal(ck.jpeg_decode(streams), exp)


def test_a_damaged_frame_of_a_batch_is_named(ck):
    from camkifu_amd import capi
    streams, _ = jpeg_cases.batch_case()
    bad = streams[3][:len(streams[3]) // 2]
    with pytest.raises(capi.CkError, match=r"frame 3: .*ran past its end") as e:
        ck.jpeg_decode(streams[:3] + [bad] + streams[4:])
    assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 3
    with pytest.raises(capi.CkError, match=r"frame 0: .*SOF2") as e:
        ck.jpeg_decode([streams[0].replace(b"\xff\xc0", b"\xff\xc2", 1)])
    assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 0
    assert np.array_equal(ck.jpeg_decode(streams[:1])[0], jpeg_cases.batch_case()[1][0])         # the context works on


@pytest.mark.parametrize("kind", jpeg_cases.KINDS)
@pytest.mark.parametrize("shape", jpeg_cases.synthetic_shapes(), ids=lambda s: "%dx%d_s%d" % s)
def test_reconstruct_alone_on_synthetic_coefficients(ck, kind, shape):
    import torch
    h, w, sampling = shape
    coef, quant, exp = jpeg_cases.synthetic_case(kind, h, w, sampling)        # ("one_ac": several frames, all 63 positions)
    got = ck.jpeg_reconstruct(coef, quant, h, w, sampling)                                    # host -> host
    assert got.shape == exp.shape and np.array_equal(got, exp)
    # in HBM, with one frame more: the first frame's coefficients under doubled quant tables (another picture)
    coef2 = np.concatenate([coef, coef[:1]])
    quant2 = np.concatenate([quant, quant[:1] if kind == "range_ends" else np.minimum(quant[:1] * 2, 255).astype(np.uint16)])
    last = jpeg_ref.reconstruct(coef2[-1], quant2[-1], h, w, sampling)
    # (the tables travel as int16 bits: the call takes pointers)
    got2 = ck.jpeg_reconstruct(torch.from_numpy(coef2).cuda(), torch.from_numpy(quant2.view(np.int16)).cuda(), h, w, sampling)
    assert got2.is_cuda
    got2 = got2.cpu().numpy()
    assert np.array_equal(got2[:-1], exp) and np.array_equal(got2[-1], last)


def test_reconstruct_refuses_arrays_that_do_not_fit_the_geometry(ck):
    """the library cannot see how much memory lies behind a pointer: the binding holds sizes and element types"""
    import torch
    from camkifu_amd import capi
    coef, quant, _ = jpeg_cases.synthetic_case("sparse", 17, 33, jpeg_ref.S420)
    for bad_coef, bad_quant in [(coef[:, :-64], quant), (coef.astype(np.int32), quant), (coef, quant[:, :2]),
                                (torch.from_numpy(coef[:, :-64].copy()).cuda(), torch.from_numpy(quant.view(np.int16)).cuda()),
                                (torch.from_numpy(coef).cuda().to(torch.int32), torch.from_numpy(quant.view(np.int16)).cuda())]:
        with pytest.raises(capi.CkError, match="is needed"):
            ck.jpeg_reconstruct(bad_coef, bad_quant, 17, 33, jpeg_ref.S420)
    with pytest.raises(capi.CkError, match="out: .*is needed"):
        ck.jpeg_reconstruct(coef, quant, 17, 33, jpeg_ref.S420, out=np.zeros((1, 17, 33, 3), np.float32))
    streams, exp = jpeg_cases.batch_case()
    with pytest.raises(capi.CkError, match="out: .*is needed"):
        ck.jpeg_decode(streams, out=np.zeros(exp.shape, np.int32))


def test_reconstruct_equals_the_reference_on_the_decoded_cases(ck):
    """the two halves held apart: the reference's coefficients through the kernel, the library's through the reference"""
    from camkifu_amd import capi
    for name in jpeg_cases.names(24, 5):
        data, exp = jpeg_cases.file_cases()[name]
        info, coef, quant = jpeg_cases.ref_coefficients(name)
        got = ck.jpeg_reconstruct(coef[None], quant[None], info["h"], info["w"], info["sampling"])
        assert np.array_equal(got[0], exp), name
        _, coef2, quant2 = capi.jpeg_coefficients([data])
        assert np.array_equal(jpeg_ref.reconstruct(coef2[0], quant2[0], info["h"], info["w"], info["sampling"]), exp), name


def test_avi_capture_reads_the_references_frames(ck):
    from camkifu_amd.core import capture as cap
    _, frames = jpeg_cases.avi_reference()
    c = cap.AviMjpegCapture(jpeg_cases.AVI, decode=ck.jpeg_decode)
    got = []
    while True:
        ok, img = c.read()
        if not ok:
            break
        got.append(img)
    assert len(got) == 6 and c.damaged == 1
    for k in range(6):
        assert got[k].shape == (48, 64, 3) and np.array_equal(got[k], frames[k]), k


def test_image_capture_reads_a_still(ck, tmp_path):
    from camkifu_amd.core import capture as cap
    data, exp = jpeg_cases.file_cases()["noise_47x61_420_q90_r0"]
    path = tmp_path / "still.jpg"
    path.write_bytes(data)
    c = cap.ImageCapture(str(path), decode=ck.jpeg_decode)
    assert c.isOpened() and np.array_equal(c.read()[1], exp)


def test_process_mjpeg_on_tiny_avi_equals_process_batch_on_the_references_frames(ck):
    from camkifu_amd import pipeline
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture as cap
    from camkifu_amd.stone.nn_manager import NNManager
    ck.cnn_set_weights(NNManager.init_net())
    _, frames = jpeg_cases.avi_reference()
    c = cap.AviMjpegCapture(jpeg_cases.AVI, decode=ck.jpeg_decode)
    idx = cap.file_frame_indices(len(c), c.fps, 25)                    # every second frame: 1, 3 (the repeat), 5
    assert idx == [1, 3, 5]
    ctrl = ControllerHeadless()
    with pipeline.FastFilePipeline(48, 64, ctrl, ctx=ck, bg_init_frames=2) as pipe:
        out = pipe.process_mjpeg(c, batch=2, file_fps=25)
        done, mtx = pipe.frames_done, pipe.board.mtx
    ctrl2 = ControllerHeadless()
    with pipeline.FastFilePipeline(48, 64, ctrl2, ctx=ck, bg_init_frames=2) as pipe2:
        out2 = []
        dec = np.stack([frames[i] for i in idx])
        for b0 in range(0, len(idx), 2):
            out2.extend(pipe2.process_batch(dec[b0:b0 + 2], len(dec[b0:b0 + 2])))
        mtx2 = pipe2.board.mtx
    assert done == 3 and len(out) == len(out2) == 3
    assert repr(out) == repr(out2) and ctrl.kifu.to_sgf() == ctrl2.kifu.to_sgf()
    assert (mtx is None) == (mtx2 is None) and (mtx is None or np.array_equal(mtx, mtx2))


def test_process_mjpeg_names_the_damaged_frame_of_the_file(ck, tmp_path):
    from camkifu_amd import capi, pipeline
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture as cap
    good = jpeg_cases.file_cases()["ramp_48x64_420_q90_r0"][0]
    path = str(tmp_path / "damaged.avi")
    cap.write_mjpeg_avi(path, [good, good, good, good, good, good[:len(good) - 200], good, good], 48, 64, fps=(25, 1))
    c = cap.AviMjpegCapture(path, decode=ck.jpeg_decode)
    assert c.damaged == 0                                          # its headers are fine: only the decoder finds out
    with pipeline.FastFilePipeline(48, 64, ControllerHeadless(), ctx=ck, bg_init_frames=2) as pipe:
        with pytest.raises(capi.CkError, match=r"frame 5 of .*damaged\.avi: .*ran past its end") as e:
            pipe.process_mjpeg(c, batch=8, file_fps=25)              # frames 1, 3, 5, 7
        assert e.value.code == capi.CK_ERR_DATA and e.value.bad_frame == 5


def test_mjpeg_film_through_the_pipeline_gives_the_games_record(ck, tmp_path):
    """the clip of test_y4m_file_through_the_pipeline (640x480, 100 frames) encoded as Motion-JPEG at quality 95 and run
    through process_mjpeg: the record of the game equals the one the uncompressed frames give, and the frames the
    pipeline saw are Pillow's decodes bit for bit"""
    Image = pytest.importorskip("PIL.Image")
    from camkifu_amd import pipeline, synth
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import capture as cap
    from camkifu_amd.stone.nn_manager import NNManager
    rng = np.random.default_rng(5)
    corners = synth.random_corners(480, 640, rng)
    stones = synth.random_stones(rng, density=0.3)
    bgr = [synth.render(480, 640, stones, corners, seed=900 + f).numpy() for f in range(8)]
    jpegs = []
    for f in range(8):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(bgr[f][:, :, ::-1]), "RGB").save(buf, "JPEG", quality=95)
        jpegs.append(buf.getvalue())
    path = str(tmp_path / "game.avi")
    cap.write_mjpeg_avi(path, (jpegs[f % 8] for f in range(100)), 480, 640, fps=(30, 1))
    ck.cnn_set_weights(NNManager.init_net())
    c = cap.AviMjpegCapture(path, decode=ck.jpeg_decode)
    idx = cap.file_frame_indices(len(c), c.fps)
    assert len(c) == 100 and c.damaged == 0 and idx == list(range(6, 100, 7))
    c.set(cap.CAP_PROP_POS_FRAMES, 6)
    pil = np.asarray(Image.open(io.BytesIO(jpegs[6])))[:, :, ::-1]
    assert np.array_equal(c.read()[1], pil)
    ctrl = ControllerHeadless()
    with pipeline.FastFilePipeline(480, 640, ctrl, ctx=ck, bg_init_frames=2) as pipe:
        pipe.process_mjpeg(c, batch=7)
        done = pipe.frames_done
    ctrl2 = ControllerHeadless()
    with pipeline.FastFilePipeline(480, 640, ctrl2, ctx=ck, bg_init_frames=2) as pipe2:
        raw = np.stack([bgr[i % 8] for i in idx])
        for b0 in range(0, len(idx), 7):
            pipe2.process_batch(raw[b0:b0 + 7], len(raw[b0:b0 + 7]))
    assert done == len(idx) and len(ctrl2.kifu.moves) > 0
    assert ctrl.kifu.to_sgf() == ctrl2.kifu.to_sgf()

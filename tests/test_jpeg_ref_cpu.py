"""tests/jpeg_ref.py, the plain numpy JPEG decoder the library is held against, is itself held against Pillow (libjpeg):
every committed expected image, and -- where Pillow imports -- live decodes of freshly encoded images."""
import io

import numpy as np
import pytest

from . import jpeg_cases, jpeg_ref


@pytest.mark.parametrize("part", range(8))
def test_reference_equals_every_committed_image(part):
    cases = jpeg_cases.file_cases()
    assert len(cases) == 288 + 10
    for name in jpeg_cases.names(8, part):
        data, exp = cases[name]
        got = jpeg_ref.decode(data)
        assert got.shape == exp.shape and np.array_equal(got, exp), name
        info = jpeg_cases.ref_coefficients(name)[0]
        assert (info["restart_interval"] > 0) == name.endswith("_r3"), name


def test_reference_equals_the_batch_frames():
    streams, exp = jpeg_cases.batch_case()
    quants = set()
    for k, data in enumerate(streams):
        assert np.array_equal(jpeg_ref.decode(data), exp[k]), k
        quants.add(jpeg_ref.coefficients(data)[2].tobytes())
    assert len(quants) == 5                              # a quant table per frame


def test_reference_equals_a_live_pillow_decode():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    for h, w, sub, q in [(23, 41, 2, 85), (16, 16, 1, 30), (9, 70, 0, 97), (31, 18, 2, 100), (40, 40, None, 60),
                        (5, 2, 2, 95), (3, 4, 2, 95), (2, 3, 1, 95), (9, 4, 1, 95), (7, 5, 2, 95), (6, 5, 1, 95)]:
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rgb[: h // 2] = (np.arange(w)[None, :, None] * 3 + np.arange(h // 2)[:, None, None] * 5) % 256
        buf = io.BytesIO()
        if sub is None:
            Image.fromarray(np.ascontiguousarray(rgb[:, :, 0]), "L").save(buf, "JPEG", quality=q)
        else:
            Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=q, subsampling=sub)
        data = buf.getvalue()
        a = np.asarray(Image.open(io.BytesIO(data)))
        exp = np.repeat(a[:, :, None], 3, axis=2) if a.ndim == 2 else a[:, :, ::-1]
        assert np.array_equal(jpeg_ref.decode(data), exp), (h, w, sub, q)


def test_avi_walker_reads_the_fixture():
    idx, frames = jpeg_cases.avi_reference()
    assert (idx["h"], idx["w"], idx["fps"]) == (48, 64, 25.0)
    assert [len(c) > 0 for c in idx["chunks"]] == [True, True, True, False, True, True]
    assert frames[3] is frames[2] and frames[0].shape == (48, 64, 3)

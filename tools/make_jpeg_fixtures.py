#!/usr/bin/env python
"""Write the fixtures of the JPEG tests (needs Pillow; the tests themselves do not):

  tests/golden/jpeg_cases*.npz   JPEG byte strings ("j_<name>") and the BGR image Pillow decodes from each ("e_<name>"):
                                 every size x sampling x quality x restart setting below, on a noise image and on a smooth
                                 ramp, and a few pictures at most 4 pixels wide; split over several archives so that each stays well under the limit for a committed file
  tests/golden/jpeg_batch.npz    five 136x200 4:2:0 frames at qualities 50, 75, 90, 95, 100 (one batch, several tiles, a quant
                                 table per frame)
  tests/golden/tiny.avi          6 frames of 64x48, the fourth chunk zero-length

Deterministic for a given Pillow / libjpeg build; run from the repository root:  python tools/make_jpeg_fixtures.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIMIT = 700 * 1024                 # bytes of payload per archive

SIZES = [(48, 64), (47, 61), (17, 33), (8, 8), (1, 1), (50, 35)]                 # h, w
SAMPLINGS = [("444", 0), ("422", 1), ("420", 2), ("grey", None)]
QUALITIES = [5, 90, 100]
RESTARTS = [0, 3]                  # MCUs between restart markers (0: none)
# pictures at most 4 pixels wide: libjpeg replicates chroma samples there instead of filtering (noise, quality 90 only)
NARROW = [(5, 2), (3, 4), (2, 3), (9, 2), (12, 4)]


def picture(kind, h, w, seed=0):
    if kind == "noise":
        return np.random.default_rng(1000 + seed + 7 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 255 * x / max(1, w - 1)
    g = 255 * y / max(1, h - 1)
    b = 127.5 + 127.5 * np.sin((x + 2 * y + seed) / 9.0)
    return np.stack([r, g, b], axis=2).round().astype(np.uint8)           # RGB


def encode(rgb, quality, subsampling, restart=0):
    buf = io.BytesIO()
    if subsampling is None:
        img = Image.fromarray(np.ascontiguousarray(rgb[:, :, 1]), "L")
        kw = {}
    else:
        img = Image.fromarray(rgb, "RGB")
        kw = dict(subsampling=subsampling)
    if restart:
        kw["restart_marker_blocks"] = restart
    img.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pillow_bgr(data):
    img = Image.open(io.BytesIO(data))
    a = np.asarray(img)
    if a.ndim == 2:
        return np.repeat(a[:, :, None], 3, axis=2).copy()
    return a[:, :, ::-1].copy()


def main():
    for f in os.listdir(GOLDEN):
        if f.startswith("jpeg_cases") and f.endswith(".npz"):
            os.remove(os.path.join(GOLDEN, f))
    parts, cur, size = [], {}, 0
    for kind in ("noise", "ramp"):
        for h, w in SIZES:
            for sname, sub in SAMPLINGS:
                for q in QUALITIES:
                    for ri in RESTARTS:
                        name = "%s_%dx%d_%s_q%d_r%d" % (kind, h, w, sname, q, ri)
                        data = encode(picture(kind, h, w), q, sub, ri)
                        exp = pillow_bgr(data)
                        assert exp.shape == (h, w, 3), (name, exp.shape)
                        if size + len(data) + exp.size > LIMIT and cur:
                            parts.append(cur)
                            cur, size = {}, 0
                        cur["j_" + name] = np.frombuffer(data, np.uint8)
                        cur["e_" + name] = exp
                        size += len(data) + exp.size
    for h, w in NARROW:
        for sname, sub in SAMPLINGS[1:3]:
            name = "noise_%dx%d_%s_q90_r0" % (h, w, sname)
            data = encode(picture("noise", h, w), 90, sub)
            cur["j_" + name] = np.frombuffer(data, np.uint8)
            cur["e_" + name] = pillow_bgr(data)
    parts.append(cur)
    for k, part in enumerate(parts):
        path = os.path.join(GOLDEN, "jpeg_cases%s.npz" % ("" if k == 0 else "_%d" % k))
        np.savez_compressed(path, **part)
        print(path, os.path.getsize(path), len(part) // 2, "cases")

    batch = {}
    for k, q in enumerate((50, 75, 90, 95, 100)):
        rgb = picture("ramp", 136, 200, seed=k)
        rgb = np.clip(rgb.astype(np.int64) + np.random.default_rng(k).integers(-12, 13, rgb.shape), 0, 255).astype(np.uint8)
        data = encode(rgb, q, 2)
        batch["j_%d" % k] = np.frombuffer(data, np.uint8)
        batch["e_%d" % k] = pillow_bgr(data)
    path = os.path.join(GOLDEN, "jpeg_batch.npz")
    np.savez_compressed(path, **batch)
    print(path, os.path.getsize(path))

    from camkifu_amd.core.capture import write_mjpeg_avi
    frames = []
    for k in range(6):
        rgb = picture("ramp", 48, 64, seed=5 * k)
        rgb[8 + 4 * k:20 + 4 * k, 10 + 6 * k:26 + 6 * k] = picture("noise", 12, 16, seed=k)
        frames.append(b"" if k == 3 else encode(rgb, 90, 2))
    path = os.path.join(GOLDEN, "tiny.avi")
    write_mjpeg_avi(path, frames, 48, 64, fps=(25, 1))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()

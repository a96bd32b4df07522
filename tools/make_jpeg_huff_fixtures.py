#!/usr/bin/env python
"""Write tests/golden/jpeg_huff_cases.npz, the fixture of the custom-table test of the GPU Huffman stage (needs Pillow; the
test itself does not): two 48x64 4:2:0 frames at quality 90 coded with Pillow's optimize=True -- Huffman tables made for
each picture, so the two differ from each other and from the tables of Annex K.3 -- and a restart interval of 2 MCUs,
"j_<k>", with the BGR image Pillow decodes from each, "e_<k>".

Deterministic for a given Pillow / libjpeg build; run from the repository root:  python tools/make_jpeg_huff_fixtures.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_jpeg_fixtures import picture, pillow_bgr  # noqa: E402


def main():
    out = {}
    for k, kind in enumerate(("noise", "ramp")):
        buf = io.BytesIO()
        Image.fromarray(picture(kind, 48, 64, seed=40 + k), "RGB").save(buf, "JPEG", quality=90, subsampling=2, optimize=True,
                                                                       restart_marker_blocks=2)
        data = buf.getvalue()
        assert b"\xff\xc4" in data and b"\xff\xdd" in data
        out["j_%d" % k] = np.frombuffer(data, np.uint8)
        out["e_%d" % k] = pillow_bgr(data)
    assert out["j_0"].tobytes() != out["j_1"].tobytes()
    path = os.path.join(ROOT, "tests", "golden", "jpeg_huff_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()

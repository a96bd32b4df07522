"""Restart intervals through the writers and the tools, no GPU: MjpegWriter and write_jpeg hand `restart_interval` to their
encoder only when it is set (an encoder that does not know the word keeps working), tools/transcode.py turns --restart into
MCUs, and the bindings refuse an entropy mode they do not know before any library call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Encoder:
    """stands in for Context.jpeg_encode: records what it was asked, returns a stream per frame"""

    def __init__(self):
        self.calls = []

    def __call__(self, frames, **kw):
        self.calls.append(kw)
        return [b"\xff\xd8\xff\xd9"] * len(frames)


def test_writers_pass_a_restart_interval_through_only_when_set(tmp_path):
    from camkifu_amd.core import capture as cap
    frames = np.zeros((2, 16, 16, 3), np.uint8)
    enc = _Encoder()
    with cap.MjpegWriter(str(tmp_path / "a.avi"), 16, 16, encode=enc, restart_interval=7) as wr:
        wr.write(frames)
    assert enc.calls == [dict(quality=90, sampling=3, restart_interval=7)]
    enc = _Encoder()
    with cap.MjpegWriter(str(tmp_path / "b.avi"), 16, 16, encode=enc) as wr:
        wr.write(frames)
    assert enc.calls == [dict(quality=90, sampling=3)]
    enc = _Encoder()
    cap.write_jpeg(str(tmp_path / "c.jpg"), frames[0], encode=enc, restart_interval=2)
    cap.write_jpeg(str(tmp_path / "d.jpg"), frames[0], encode=enc)
    assert enc.calls == [dict(quality=90, sampling=3, restart_interval=2), dict(quality=90, sampling=3)]


def test_transcode_restart_option_in_mcus():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import transcode
    finally:
        sys.path.pop(0)
    assert transcode.restart_mcus("0", 1920, 3) == 0 and transcode.restart_mcus(None, 1920, 3) == 0
    assert transcode.restart_mcus("12", 1920, 3) == 12
    assert transcode.restart_mcus("row", 1920, 3) == 120 and transcode.restart_mcus("row", 1920, 2) == 120
    assert transcode.restart_mcus("row", 1920, 1) == 240 and transcode.restart_mcus("row", 33, 0) == 5
    with pytest.raises(SystemExit):
        transcode.restart_mcus("70000", 1920, 3)


def test_an_unknown_entropy_mode_is_refused_by_the_binding():
    from camkifu_amd import capi
    ctx = capi.Context.__new__(capi.Context)                          # (no device: the check comes before the library)
    ctx._h = None
    with pytest.raises(capi.CkError, match="'host' or 'device'"):
        ctx.jpeg_set_entropy("auto")
    assert (capi.CK_JPEG_ENTROPY_HOST, capi.CK_JPEG_ENTROPY_DEVICE) == (0, 1)

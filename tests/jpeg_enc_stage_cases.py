"""The cases of the staged JPEG entropy coder's tests (the host's stages and the GPU kernels): coefficient arrays built directly,
so that the coder's extremes do not depend on images.  References are computed once per process and shared (read-only).

A case is (content, h, w, sampling, restart interval in MCUs); its name spells the five out.  Contents:
  zeros  all 0: blocks of 6 bits (luma) and 4 bits (chroma), many to a dword
  ff     AC 1023 at zigzag 16, 32 and 48 (the code of symbol 0xFA, then ten 1-bits: stuffed bytes), DC 0 / 1000 by block
  full   every AC +-1023 by position, DC -+1023 by block: no EOB, DC differences of 11 bits, about 260 bytes a block
  seamN  a grey frame whose first restart interval is N unstuffed bytes long: AC 1 at the first zigzag positions (3 bits
         each) on top of `zeros`, as many as it takes
"""
import functools

import numpy as np

from . import jpeg_enc_ref as ref

SNAME = {ref.GREY: "grey", ref.S444: "444", ref.S422: "422", ref.S420: "420"}
CONTENTS = ("zeros", "ff", "full")
H, W = 64, 96
GEOMETRIES = [(H, W, ref.GREY), (H, W, ref.S444), (H, W, ref.S422), (H, W, ref.S420), (1, 1, ref.GREY), (1, 1, ref.S420),
              (17, 33, ref.S422), (17, 33, ref.S420)]
QUALITY = 90
SEAM_INTERVAL = 48               # of the 96 MCUs of a grey 64 x 96 frame


def restart_intervals(h, w, s):
    """none, every MCU, one that does not divide the MCUs of a row, one MCU row"""
    return (0, 1, 5, ref.geometry(h, w, s)[0])


def name_of(case):
    content, h, w, s, ri = case
    return "%s_%dx%d_%s_r%d" % (content, h, w, SNAME[s], ri)


@functools.lru_cache(maxsize=None)
def tiles():
    from camkifu_amd import capi
    return capi.jpeg_enc_tiles()


def seam_lengths():
    """first segments that end one byte short of, on, and one byte over the first byte-tile seam"""
    y = tiles()[1]
    return (y - 1, y, y + 1)


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for h, w, s in GEOMETRIES:
        for ri in dict.fromkeys(restart_intervals(h, w, s)):
            for content in CONTENTS:
                out.append((content, h, w, s, ri))
    out += [("seam%d" % n, H, W, ref.GREY, SEAM_INTERVAL) for n in seam_lengths()]
    return out


def quant():
    return ref.quant_tables(QUALITY)


@functools.lru_cache(maxsize=None)
def coef(case):
    """int16 flat, the layout of ck_jpeg_coefficients (read-only)"""
    content, h, w, s, ri = case
    nb = ref.n_blocks(h, w, s)
    c = np.zeros((nb, 64), np.int16)
    b = np.arange(nb)
    if content == "ff":
        for z in (16, 32, 48):
            c[:, ref.ZIGZAG[z]] = 1023
        c[:, 0] = np.where(b % 2 == 0, 0, 1000)
    elif content == "full":
        c[:] = np.where(np.arange(64) % 2 == 0, 1023, -1023)
        c[:, 0] = np.where(b % 2 == 0, -1023, 1023)
    elif content.startswith("seam"):
        assert s == ref.GREY and ri > 0
        want = int(content[4:])                          # bytes: 8 * (want - 1) < bits <= 8 * want
        extra = -(-(8 * (want - 1) + 1 - 6 * ri) // 3)   # ACs of 3 bits on top of ri blocks of 6
        assert 0 <= extra <= 62 * ri and 6 * ri + 3 * extra <= 8 * want, "the interval cannot be made %d bytes long" % want
        for blk in range(ri):                            # (grey: block = MCU = place)
            n = min(62, extra)
            c[blk, ref.ZIGZAG[1:1 + n]] = 1
            extra -= n
    else:
        assert content == "zeros", content
    c = c.reshape(-1)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ref_encode(case):
    """(the reference's bytes, its path statistics)"""
    content, h, w, s, ri = case
    stats = ref.new_stats()
    return ref.entropy_encode(coef(case), quant(), h, w, s, ri, stats), stats


def segments(case):
    """the unstuffed bytes of every restart interval of the reference's stream, padding included"""
    content, h, w, s, ri = case
    data = ref_encode(case)[0]
    scan = data[len(ref.headers(quant(), h, w, s, ri)):-2]
    out, cur, i = [], bytearray(), 0
    while i < len(scan):
        if scan[i] == 0xFF and scan[i + 1] == 0:
            cur.append(0xFF)
            i += 2
        elif scan[i] == 0xFF:
            assert 0xD0 <= scan[i + 1] <= 0xD7
            out.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            cur.append(scan[i])
            i += 1
    return out + [bytes(cur)]


def batch():
    """five frames of one geometry with different contents: (cases, h, w, sampling, restart interval)"""
    cs = [("zeros", H, W, ref.S420, 5), ("ff", H, W, ref.S420, 5), ("full", H, W, ref.S420, 5), ("ff", H, W, ref.S420, 5),
          ("zeros", H, W, ref.S420, 5)]
    return cs, H, W, ref.S420, 5


def check_coverage():
    """the cases cross at least three block tiles inside one segment and three byte tiles inside one frame, and a segment
    ends one byte short of, on, and one byte over a byte-tile seam"""
    tb, ty = tiles()
    assert H < 256 and W < 256
    seg_blocks, frame_bytes, ends = 0, 0, set()
    for case in all_cases():
        content, h, w, s, ri = case
        mx, my, grids = ref.geometry(h, w, s)
        per_mcu = ref.n_blocks(h, w, s) // (mx * my)
        seg_blocks = max(seg_blocks, (min(ri, mx * my) if ri else mx * my) * per_mcu)
        if content.startswith("seam") or content == "full":
            at = 0
            for seg in segments(case):
                at += len(seg)
                ends.add(at % ty if at >= ty - 1 else None)
            frame_bytes = max(frame_bytes, at)
    assert seg_blocks > 2 * tb, "no segment crosses three block tiles of %d" % tb
    assert frame_bytes > 2 * ty, "no frame crosses three byte tiles of %d" % ty
    assert {ty - 1, 0, 1} <= ends, "no segment ends around a byte-tile seam"
    assert [len(segments(("seam%d" % n, H, W, ref.GREY, SEAM_INTERVAL))[0]) for n in seam_lengths()] == list(seam_lengths())

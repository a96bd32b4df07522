"""The device inflate: the kernel of csrc/k_png_inflate.hip against the staged host form of the same steps
(capi.png_inflate_staged) stream by stream -- bytes, total, cause, produced -- and png_decode in device mode against the host
mode, byte for byte and message for message."""
import struct
import zlib

import numpy as np
import pytest

from . import png_cases, png_inflate_cases, png_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def geometry():
    from camkifu_amd import capi
    g = capi.png_inflate_geometry()
    assert g["window_bits"] in (64, 128, 256) and g["flush_bytes"] == 16384
    return g


def _staged(z, cap):
    from camkifu_amd import capi
    return capi.png_inflate_staged(z, cap=cap, verdict=True)


def _same(got, want, what):
    assert (got["cause"], got["produced"], got["total"]) == (want["cause"], want["produced"], want["total"]), what
    if want["cause"] == 0:
        assert got["data"] == want["data"], what


def test_good_and_seam_streams_in_one_call(ck, geometry):
    cases = [(k, z, p) for k, (z, p) in sorted(png_cases.inflate_streams().items())]
    cases += [(k, z, p) for k, (z, p, _) in sorted(png_inflate_cases.seam_streams(geometry["window_bits"]).items())]
    cases += [("%d bytes" % n, z, p) for n, (z, p) in sorted(png_inflate_cases.sized_streams(geometry["flush_bytes"]).items())]
    cap = 70000
    got = ck.png_inflate_device([z for _, z, _ in cases], cap=cap)
    for (name, z, payload), g in zip(cases, got):
        want = _staged(z, cap)
        assert (want["data"] if want["cause"] == 0 else None) == payload, name
        _same(g, want, name)
    # room for none, one, across a match, all but one byte: the verdict and the count do not depend on it
    z, payload = png_cases.inflate_streams()["a match at distance 32768"]
    caps = [0, 1, 100, 32768 + 100, 32768 + 259, len(payload) - 1]
    for cap, g in zip(caps, ck.png_inflate_device([z] * len(caps), cap=caps)):
        _same(g, _staged(z, cap), cap)
        assert g["data"] == payload[:cap] and g["total"] == len(payload)


def test_every_truncation_and_byte_change_in_one_call(ck):
    damaged = list(png_inflate_cases.damaged())
    assert len(damaged) > 4000 and max(len(z) for _, z in damaged) <= 620
    got = ck.png_inflate_device([z if z else b"" for _, z in damaged], cap=4096)
    refused = 0
    for (what, z), g in zip(damaged, got):
        _same(g, _staged(z, 4096), what)
        refused += g["cause"] != 0
    assert refused > len(damaged) // 2
    assert ck.png_inflate_stats()["streams"] == len(damaged)


def test_stats_count_the_tokens(ck, geometry):
    S = png_inflate_cases.seam_streams(geometry["window_bits"])
    for name, (z, payload, tokens) in sorted(S.items()):
        g = ck.png_inflate_device([z], cap=16)[0]
        st = ck.png_inflate_stats()
        assert st["streams"] == 1 and st["tokens"] == tokens and st["bytes"] == g["produced"], name
        assert st["steps"] >= 1 or tokens == 0
    # streams with zlib's own matches, against the counter of tests/png_inflate_cases.py: alone, and all in one call
    sized = png_inflate_cases.sized_streams(geometry["flush_bytes"])
    counts = {n: png_inflate_cases.count_tokens(z) for n, (z, _) in sized.items()}
    for n, (z, payload) in sized.items():
        assert counts[n][1] == len(payload) and counts[n][0] < len(payload) // 2       # (the counter reads the stream right; matches)
        ck.png_inflate_device([z], cap=16)
        st = ck.png_inflate_stats()
        assert (st["tokens"], st["bytes"]) == counts[n], n
    ck.png_inflate_device([z for z, _ in sized.values()], cap=16)
    st = ck.png_inflate_stats()
    assert (st["streams"], st["tokens"], st["bytes"]) == (len(sized), sum(c[0] for c in counts.values()), sum(c[1] for c in counts.values()))
    # a file deflated at level 9, through png_decode in device mode
    data, want = png_cases.image(120, 100, 2, 8, seed=12, smooth=True, flavour="best")
    assert np.array_equal(ck.png_decode([data], inflate="device")[0], want)
    st = ck.png_inflate_stats()
    assert (st["streams"], st["tokens"], st["bytes"]) == (1,) + png_inflate_cases.count_tokens(png_ref.walk(data)["idat"])
    # literals only: as many tokens as bytes, which png_cases.trace confirms to be the case (no match in the stream)
    z = png_cases.small_streams()["dynamic, literals only"]
    t = png_cases.trace(z)
    assert t["max_length"] == 0
    ck.png_inflate_device([z, z])
    st = ck.png_inflate_stats()
    assert st == dict(streams=2, steps=st["steps"], tokens=2 * len(t["payload"]), bytes=2 * len(t["payload"]))
    assert st["tokens"] / st["steps"] > 2                   # (the window pays: several tokens a step)


def _both(ck, files):
    host = ck.png_decode(files, inflate="host")
    up_host = ck.png_uploaded_bytes()
    dev = ck.png_decode(files, inflate="device")
    up_dev = ck.png_uploaded_bytes()
    assert np.array_equal(host, dev)
    return host, up_host, up_dev


def test_device_mode_decodes_what_the_host_mode_decodes(ck):
    for ct, depth in png_cases.TYPES:
        data, want = png_cases.image(37, 21, ct, depth, seed=3)
        assert np.array_equal(_both(ck, [data])[0][0], want), (ct, depth)
    golden = png_cases.golden()
    names = sorted(golden)
    out = _both(ck, [golden[k][0] for k in names])[0]
    for k, name in enumerate(names):
        assert np.array_equal(out[k], golden[name][1]), name
    rng = np.random.RandomState(4)
    for h, w in ((1, 1), (16, 64), (17, 65), (380, 380)):
        img = (np.cumsum(rng.randint(-3, 4, (h, w, 3)), 1) + 100).astype(np.uint8)
        img[h // 3:h // 2] = 200                            # flat rows: runs
        for runs in (False, True):
            data = ck.png_encode(img, runs=runs)[0]
            assert np.array_equal(_both(ck, [data])[0][0], img), (h, w, runs)
    data, want = png_cases.image(300, 260, 2, 8, seed=5, smooth=True, flavour="best")
    t = png_cases.trace(png_ref.walk(data)["idat"])          # zlib level 9: several blocks, matches at real distances
    assert len(t["types"]) >= 2 and t["max_distance"] > 1000 and t["max_length"] >= 3
    assert np.array_equal(_both(ck, [data])[0][0], want)
    data, want = png_cases.image(40, 30, 6, 8, seed=6, idat_split=7)
    assert np.array_equal(_both(ck, [data])[0][0], want)
    # bytes left over behind the image data: one row more than the header says
    flt = png_ref.filtered(rng.randint(0, 256, (9, 27)).astype(np.uint8), 2, 8, [1] * 9)
    more = png_ref.SIG + png_ref.chunk(b"IHDR", struct.pack(">IIBBBBB", 9, 8, 8, 2, 0, 0, 0)) + png_ref.chunk(b"IDAT", zlib.compress(flt)) + png_ref.chunk(b"IEND")
    _both(ck, [more])


def _refusal(ck, files, inflate):
    from camkifu_amd import capi
    with pytest.raises(capi.CkError) as e:
        ck.png_decode(files, inflate=inflate)
    return str(e.value), e.value.code, e.value.bad_frame


def test_a_batch_of_nine_with_two_damaged_files(ck):
    kinds = [(0, 1), (0, 16), (2, 8), (2, 16), (3, 2), (3, 8), (4, 8), (6, 8), (6, 16)]
    good = [png_cases.image(23, 19, ct, d, seed=20 + k, flavour=("best", "fixed", "stored", "rle", "huffman")[k % 5])[0] for k, (ct, d) in enumerate(kinds)]

    def damage(data, change):
        """the file with its inflated rows changed and deflated again (the CRCs hold: the inflate or the rows refuse it)"""
        c = png_ref.walk(data)
        z = change(bytearray(zlib.decompress(c["idat"])))
        head = data[:data.index(b"IDAT") - 4]
        return head + png_ref.chunk(b"IDAT", z) + png_ref.chunk(b"IEND")

    def filter_7(rows):
        rows[0] = 7
        return zlib.compress(bytes(rows))

    def cut_adler(rows):
        z = bytearray(zlib.compress(bytes(rows)))
        z[-1] ^= 0x55
        return bytes(z)

    files = list(good)
    files[4] = damage(good[4], cut_adler)
    files[8] = damage(good[8], filter_7)
    want = _refusal(ck, files, "host")
    assert want[2] == 4 and "frame 4: Adler-32" in want[0]
    assert _refusal(ck, files, "device") == want
    files[4] = good[4]
    want = _refusal(ck, files, "host")
    assert want[2] == 8 and "frame 8: row 0: filter type 7" in want[0]
    assert _refusal(ck, files, "device") == want
    short = damage(good[2], lambda rows: zlib.compress(bytes(rows[:-3])))
    want = _refusal(ck, [good[0], short], "host")
    assert "frame 1: IDAT data too short" in want[0] and _refusal(ck, [good[0], short], "device") == want
    _both(ck, good)                                         # the context decodes a good batch right afterwards


def test_only_the_streams_go_up(ck):
    """images that deflate well (the nine above are noise): the device mode uploads the zlib streams, a descriptor (32 bytes),
    a palette (768) and a job (48) a file, and padding to 16 bytes; the host mode uploads the inflated rows"""
    files = [png_cases.image(96, 64, ct, d, seed=60 + k, smooth=True, filters=[0] * 64, flavour="best")[0] for k, (ct, d) in enumerate([(2, 8), (0, 8), (6, 8), (3, 8), (2, 16)])]
    host, up_host, up_dev = _both(ck, files)
    zsum = sum(len(png_ref.walk(d)["idat"]) for d in files)
    rows = sum(64 * (1 + png_ref.rowbytes(96, ct, d)) for ct, d in [(2, 8), (0, 8), (6, 8), (3, 8), (2, 16)])
    assert up_host >= rows
    assert up_dev < up_host
    assert zsum <= up_dev <= zsum + len(files) * (32 + 768 + 48 + 16) + 3 * 16


def test_read_pngs_groups_by_size(ck, tmp_path, monkeypatch):
    from camkifu_amd import capi
    from camkifu_amd.core import capture
    monkeypatch.setattr(capi, "get_context", lambda device=0: ck)
    made = [png_cases.image(w, h, ct, d, seed=40 + k) for k, (w, h, ct, d) in
            enumerate([(12, 9, 2, 8), (30, 7, 0, 8), (12, 9, 6, 8), (30, 7, 3, 4), (12, 9, 0, 2)])]
    paths = []
    for k, (data, _) in enumerate(made):
        paths.append(str(tmp_path / ("snapshot-%d.png" % k)))
        with open(paths[-1], "wb") as f:
            f.write(data)
    for inflate in ("host", "device", None):
        images = capture.read_pngs(paths, inflate=inflate)
        assert len(images) == 5
        for img, (_, want) in zip(images, made):
            assert np.array_equal(img, want)
    bad = bytearray(made[3][0])
    bad[-20] ^= 0x40
    with open(paths[3], "wb") as f:
        f.write(bytes(bad))
    with pytest.raises(capi.CkError) as e:
        capture.read_pngs(paths, inflate="device")
    assert e.value.bad_frame == 3


def test_the_mode_is_set_and_taken_back(ck):
    from camkifu_amd import capi
    data, want = png_cases.image(50, 40, 2, 8, seed=9, smooth=True, filters=[0] * 40)
    fresh = ck.png_decode([data])
    assert np.array_equal(fresh[0], want)
    up = ck.png_uploaded_bytes()
    assert up >= 40 * 151                                    # the host mode uploads the inflated rows
    ck.png_set_inflate("device")
    assert np.array_equal(ck.png_decode([data])[0], want) and ck.png_uploaded_bytes() < up
    assert ck.png_inflate_stats()["bytes"] == 40 * 151
    ck.png_set_inflate("host")
    assert np.array_equal(ck.png_decode([data]), fresh) and ck.png_uploaded_bytes() == up
    for mode in ("gpu", 1, None):
        with pytest.raises(capi.CkError):
            ck.png_set_inflate(mode)
    rc = capi.lib().ck_png_set_inflate(ck._h, 2)
    assert rc == capi.CK_ERR_ARG
    assert np.array_equal(ck.png_decode([data])[0], want) and ck.png_uploaded_bytes() == up

"""The steps of the device inflate (csrc/ck_png_inflate_stage.h) run in plain loops on the host, capi.png_inflate_staged,
against the library's host inflate capi.png_inflate: the same bytes, and for a refused stream the same message, character
for character.  No GPU."""
import zlib

import pytest

from camkifu_amd import capi

from . import png_cases, png_inflate_cases


def _verdict(fn, *a, **kw):
    try:
        return ("ok", fn(*a, **kw))
    except capi.CkError as e:
        assert e.code == capi.CK_ERR_DATA
        return ("refused", str(e))


def _geometry():
    g = capi.png_inflate_geometry()
    assert g["window_bits"] in (64, 128, 256) and g["flush_bytes"] == 16384
    return g


@pytest.mark.parametrize("name", sorted(png_cases.inflate_streams()))
def test_staged_inflate_gives_the_payload(name):
    z, payload = png_cases.inflate_streams()[name]
    assert capi.png_inflate_staged(z) == payload


@pytest.mark.parametrize("name", sorted(png_cases.small_streams()))
def test_staged_verdict_is_the_hosts_on_every_truncation_and_mutation(name):
    z = png_cases.small_streams()[name]
    assert capi.png_inflate_staged(z) == zlib.decompress(z)
    refused = compared = 0
    for what, m in png_inflate_cases.damaged():
        if not what.startswith(name + " "):
            continue
        want = _verdict(capi.png_inflate, m)
        assert _verdict(capi.png_inflate_staged, m) == want, what
        refused += want[0] == "refused"
        compared += 1
    assert compared == 4 * len(z) and refused > len(z)      # every truncation and three changes of every byte: none left out


def test_seam_streams_around_the_window():
    W = _geometry()["window_bits"]
    S = png_inflate_cases.seam_streams(W)
    assert len(S) == 11
    for name, (z, payload, tokens) in S.items():
        want = _verdict(capi.png_inflate, z)
        assert (want[0] == "ok") == (payload is not None), name
        if payload is not None:
            assert want[1] == payload and zlib.decompress(z) == payload, name      # (the case is what it says)
        assert _verdict(capi.png_inflate_staged, z) == want, name
        v = capi.png_inflate_staged(z, verdict=True)
        assert v["message"] == ("" if payload is not None else want[1].split(": ", 1)[1]), name
    later = capi.png_inflate_staged(S["a distance one byte too far as a later token of a window"][0], verdict=True)
    assert later["produced"] == 1 and later["message"] == "a distance beyond the bytes produced so far (after 1 bytes)"
    first = capi.png_inflate_staged(S["a distance one byte too far as the first token of a window"][0], verdict=True)
    assert first["produced"] == 256 and first["message"] == "a distance beyond the bytes produced so far (after 256 bytes)"
    assert first["cause"] == later["cause"] != 0


def test_payload_lengths_around_the_flush_and_the_ring():
    F = _geometry()["flush_bytes"]
    sized = png_inflate_cases.sized_streams(F)
    assert sorted(sized) == [16383, 16384, 16385, 32767, 32768, 32769, 65537]
    for n, (z, payload) in sized.items():
        assert capi.png_inflate_staged(z) == payload, n
        for cap in (0, 1, F - 1, F, F + 1, n - 1):
            v = capi.png_inflate_staged(z, cap=cap, verdict=True)
            assert v["cause"] == 0 and v["total"] == n and v["produced"] == n and v["data"] == payload[:cap], (n, cap)


def test_the_room_does_not_change_the_verdict():
    """cap values of test_inflate_ignores_what_follows_the_stream..'s kind: none, one byte, across a match, all but one"""
    z, payload = png_cases.inflate_streams()["a match at distance 32768"]
    assert capi.png_inflate_staged(z + b"trailing") == payload
    for cap in (0, 1, 100, 24577, 32767, 32768, 32769, 32768 + 100, 32768 + 258, 32768 + 259, 33000, len(payload) - 1, len(payload)):
        v = capi.png_inflate_staged(z, cap=cap, verdict=True)
        assert v["cause"] == 0 and v["total"] == len(payload) and v["data"] == payload[:cap], cap
    bad = bytearray(z)
    bad[-1] ^= 1                                            # the Adler-32 covers the bytes that found no room
    for cap in (0, 100, len(payload)):
        assert _verdict(capi.png_inflate_staged, bytes(bad), cap=cap) == _verdict(capi.png_inflate, bytes(bad))


def test_the_two_checks_of_the_rows():
    h, rowbytes = 7, 12
    rows = bytearray(b"".join(bytes([y % 5]) + bytes(range(y, y + rowbytes)) for y in range(h)))
    z = zlib.compress(bytes(rows), 6)
    assert capi.png_inflate_staged(z, rows=(h, rowbytes)) == bytes(rows)
    short = capi.png_inflate_staged(zlib.compress(bytes(rows[:-1])), rows=(h, rowbytes), verdict=True)
    assert short["message"] == "IDAT data too short: %d bytes where %d rows of 1 + %d need %d" % (len(rows) - 1, h, rowbytes, len(rows))
    for y in (0, h - 1):
        r = bytearray(rows)
        r[y * (1 + rowbytes)] = 5
        v = capi.png_inflate_staged(zlib.compress(bytes(r)), rows=(h, rowbytes), verdict=True)
        assert v["data"] is None and v["message"] == "row %d: filter type 5" % y and v["cause"] != short["cause"]
    both = bytearray(rows[:-1])                             # the host's order: the length first
    both[0] = 5
    assert capi.png_inflate_staged(zlib.compress(bytes(both)), rows=(h, rowbytes), verdict=True)["message"].startswith("IDAT data too short")
    # rows that begin on either side of a flush, in a stream longer than the ring
    h, rowbytes = 300, 130
    big = bytearray(b"".join(bytes([y % 5]) + bytes((y * 7 + i) % 251 for i in range(rowbytes)) for y in range(h)))
    for y in (124, 125, 126, 250, 251, 299):
        r = bytearray(big)
        r[y * (1 + rowbytes)] = 9
        assert capi.png_inflate_staged(zlib.compress(bytes(r)), rows=(h, rowbytes), verdict=True)["message"] == "row %d: filter type 9" % y
    r = bytearray(big)
    r[10 * 131], r[200 * 131] = 6, 7
    assert capi.png_inflate_staged(zlib.compress(bytes(r)), rows=(h, rowbytes), verdict=True)["message"] == "row 10: filter type 6"

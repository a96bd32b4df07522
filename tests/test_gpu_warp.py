"""K8 (warp_kernel, k_warp.hip) on the GPU against the plain float64 warp of tests/warp_ref.py, and bit for bit against
ora.warp_perspective, at the shapes, sizes and transforms where the kernel's paths split: every dsize class (a
byte-store tail, unaligned rows, a single block when dsize < 16, partial 64-column blocks), sources too small for the
8-byte row load, coordinates that reach the int and short clamps, W < 0, W exactly 0, a singular M, quads cut by each
frame edge, transforms on which the block association moves a tap, and per-frame matrices (m_count == n) through
ck_warp_perspective, ck_stones_detect and ck_stones_run.

The kernel must equal the plain reference at every pixel whose 32.x and 32.y lie at least 1e-6 from a .5 boundary, and
one of the two neighbouring taps' results where they lie closer (the band; each check prints how many pixels fell in
it).  Transforms whose arithmetic is exact (dyadic entries) get no band: ties at (k + 1/2) / 32 px round to even."""
import math

import numpy as np
import pytest

from tests import mog2_scenes as S
from tests import warp_ref as R

pytestmark = pytest.mark.gpu
DST = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)
DSIZES = [1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 127, 379, 380, 381, 517]


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _noise(h, w, seed):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[0, 0] = (200, 100, 50)              # what W == 0 and a singular M map to: never zero
    return img


def _check(ck, ora, src, M, dsize, exact=False, what=""):
    """kernel == oracle bit for bit, and within the plain reference (no band when `exact`) -> the kernel's image"""
    M = np.asarray(M, np.float64).reshape(3, 3)
    out = _host(ck.warp_perspective(src, M, dsize))
    assert np.array_equal(out, ora.warp_perspective(src, M, (dsize, dsize))), "%s: kernel != oracle" % what
    cands, band = R.reference(src, M, dsize, band=0 if exact else 1e-6)
    bad = R.mismatch(out, cands)
    assert not bad.any(), "%s: %d pixels differ from the plain reference, first at %s" % (
        what, int(bad.sum()), tuple(int(v) for v in np.argwhere(bad)[0]))
    print("%s: dsize %d, %d pixels in the band" % (what, dsize, band))
    return out


def _shift(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)


def _about_center(h, w, scale, deg, dsize):
    """source centre -> destination centre, scaled and rotated"""
    a = math.radians(deg)
    c, s = scale * math.cos(a), scale * math.sin(a)
    cx, cy, d = (w - 1) / 2, (h - 1) / 2, (dsize - 1) / 2
    return np.array([[c, -s, d - c * cx + s * cy], [s, c, d - s * cx - c * cy], [0, 0, 1]], np.float64)


# ---------------------------------------------------------------- destination sizes
@pytest.mark.parametrize("dsize", DSIZES)
def test_every_dsize_class(ck, ora, dsize):
    """the board quad onto a dsize square, a rotation, and an exact sub-pixel shift, from a 480 x 640 board and from
    37 x 53 noise: 1 .. 3 pixels per row (all tail), 5 and 17 (a tail after whole quads), 15 / 16 / 17 around the
    bh0 = dsize rule, 63 .. 65 and 127 around bw0 = 64, 379 / 381 / 517 (rows not a multiple of 4 bytes apart)"""
    from camkifu_amd import synth
    sc = synth.scene(480, 640, seed=8)
    board = sc["frame"].numpy()
    noise = _noise(37, 53, dsize)
    d = np.array([(0, 0), (dsize, 0), (dsize, dsize), (0, dsize)], np.float32)
    _check(ck, ora, board, ora.get_perspective_transform(sc["corners"], d), dsize, what="board quad")
    _check(ck, ora, noise, _about_center(37, 53, dsize / 40.0, 23.0, dsize), dsize, what="rotation")
    _check(ck, ora, noise, _shift(-3 + 11 / 32, 2 - 7 / 32), dsize, exact=True, what="shift by k/32")


# ---------------------------------------------------------------- source shapes and transforms
SOURCES = [(1, 1), (1, 9), (7, 1), (2, 2), (3, 11), (5, 17), (33, 47), (1080, 1920)]


@pytest.mark.parametrize("hw", SOURCES, ids=["%dx%d" % s for s in SOURCES])
def test_source_shapes(ck, ora, hw):
    """sources narrower than 3 px or shorter than 2 rows take the bounds-checked path only; identity and integer
    shifts must copy, sub-pixel shifts and ties are exact, scale / rotation within the band"""
    h, w = hw
    src = _noise(h, w, h * 7 + w)
    dsize = 380 if h > 100 else 23

    def shifted(tx, ty):                      # out[y, x] = src[y - ty, x - tx] inside the frame, 0 outside
        e = np.zeros((dsize, dsize, 3), np.uint8)
        y0, y1, x0, x1 = max(0, ty), min(dsize, h + ty), max(0, tx), min(dsize, w + tx)
        if y1 > y0 and x1 > x0:
            e[y0:y1, x0:x1] = src[y0 - ty:y1 - ty, x0 - tx:x1 - tx]
        return e
    for tx, ty in ((0, 0), (3, -2), (-1, 1), (2, 5)):
        out = _check(ck, ora, src, _shift(tx, ty), dsize, exact=True, what="shift (%d, %d)" % (tx, ty))
        assert np.array_equal(out, shifted(tx, ty)), (tx, ty)
    for k in (5, 13, 27):
        _check(ck, ora, src, _shift(k / 32, -k / 32), dsize, exact=True, what="shift by %d/32" % k)
    for k in (4, 7, -1, -6):                 # (k + 1/2) / 32: every coordinate on a tie, half of them odd
        _check(ck, ora, src, _shift((k + 0.5) / 32, (2 * k + 0.5) / 32), dsize, exact=True, what="tie %d" % k)
    for scale, deg in ((2.5, 0.0), (0.4, 0.0), (1.0, 30.0), (3.0, -71.0)):
        _check(ck, ora, src, _about_center(h, w, scale, deg, dsize), dsize, what="scale %g rotate %g" % (scale, deg))


def test_everything_outside_and_the_clamps(ck, ora):
    """a quad wholly outside the frame warps to zeros; coordinates of 1e9 px reach the +-2^31 / 32 clamp (then the
    short clamp) and stay outside, except destination (0, 0), which maps to source (0, 0)"""
    src = _noise(48, 64, 5)
    for M in (_shift(5000, 0), _shift(-70, 3), _shift(0, 4000.5)):
        assert not _check(ck, ora, src, M, 67, what="outside").any()
    for sx, sy in ((1e-9, 1e-9), (-1e-9, 1e-9), (1e-9, -1e-9)):
        out = _check(ck, ora, src, np.diag([sx, sy, 1.0]), 67, what="clamp")
        assert np.array_equal(out[0, 0], src[0, 0]) and not out.reshape(-1, 3)[1:].any()


def test_strong_perspective_horizon_inside(ck, ora):
    """W = 1.505 - dy / 100 changes sign between rows 150 and 151 (not on a row: there W would be 0 or a rounding
    error of either sign, test_w_exactly_zero's case): rows beyond see the source through W < 0 (coordinates reflected
    through the horizon), and some of them land inside the frame"""
    from camkifu_amd import synth
    src = synth.scene(480, 640, seed=9)["frame"].numpy()
    minv = np.array([[1, 0.25, -300], [0, -1, 100], [0, -0.01, 1.505]], np.float64)
    out = _check(ck, ora, src, np.linalg.inv(minv), 380, what="horizon")
    assert out[160:].any() and out[:100].any()


def test_w_exactly_zero(ck, ora):
    """an integer M whose inverse the host computes exactly: W = dx - 100, zero on column 100 while both numerators
    are not.  `W ? 32 / W : 0` sends those pixels to source (0, 0): they must hold src[0, 0] (a plain 32 / W would
    send them to infinity, i.e. zero)"""
    e, c = 20, 100
    minv = np.array([[e, 1, -e * c], [1, 0, 1 - c], [1, 0, -c]], np.float64)       # det 1
    M = np.array([[0, c, 1 - c], [1, 0, -e], [0, 1, -1]], np.float64)
    assert np.array_equal(M @ minv, np.eye(3)) and np.array_equal(R.host_inverse(M), minv.reshape(9))
    src = _noise(48, 64, 11)
    out = _check(ck, ora, src, M, 160, what="W == 0")
    assert (out[1:, c] == src[0, 0]).all()                # dy >= 1: X = dy, Y = 1, W = 0
    assert out[:, c - 30:c].any() and out[:, c + 1:].any()       # W < 0 and W > 0 both reach the frame


def test_singular_matrix(ck, ora):
    """the host inverse of a singular M is zeros (as cv::invert leaves it), so every pixel is source (0, 0)"""
    src = _noise(31, 45, 12)
    for M in (np.zeros((3, 3)), np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1]], np.float64)):
        assert (R.host_inverse(M) == 0).all()
        for dsize in (7, 65):
            out = _check(ck, ora, src, M, dsize, exact=True, what="singular")
            assert (out == src[0, 0]).all()


def test_nearly_singular_matrix_from_collinear_corners(ck, ora):
    """three exactly collinear corners on a slanted line: the solve returns det(M) ~ 1e-29, not 0, and an inverse with
    entries up to ~1e19 (tests/test_perspective_cpu.py::test_exactly_collinear_corners).  No plain reference means
    anything there; the kernel must still equal the oracle and the restatement of its own arithmetic bit for bit"""
    src = _noise(400, 640, 13)
    for quad in R.COLLINEAR[3:]:
        M = ora.get_perspective_transform(np.array(quad, np.float32), DST)
        assert np.abs(R.host_inverse(M)).max() >= 1e15
        out = _host(ck.warp_perspective(src, M))
        assert np.array_equal(out, ora.warp_perspective(src, M)), quad
        assert np.array_equal(out, R.emulate(src, M, 380)), quad


def test_quads_cut_by_each_frame_edge(ck, ora):
    from camkifu_amd import synth
    sc = synth.scene(480, 640, seed=10)
    fr = sc["frame"].numpy()
    for dx, dy in ((-330, 0), (330, 0), (0, -260), (0, 260), (-300, -230)):
        c = sc["corners"] + np.array([dx, dy], np.float32)
        out = _check(ck, ora, fr, ora.get_perspective_transform(c, DST), 380, what="cut (%d, %d)" % (dx, dy))
        empty = ~out.any(-1)
        assert empty.sum() > 10000 and (~empty).sum() > 10000, (dx, dy)


def test_transforms_that_see_the_block_association(ck, ora):
    """the CPU search's transforms (tests/warp_ref.flip_search): the kernel equals the numpy restatement of its own
    block-associated arithmetic bit for bit, and that differs from the direct sum and from blocks all at bx = 0"""
    rng = np.random.default_rng(78)
    for M, nd, nz in R.flip_search():
        src = rng.integers(0, 256, (160, 160, 3), dtype=np.uint8)
        for dsize in (380, 517):
            out = _check(ck, ora, src, M, dsize, what="block association")
            want = R.emulate(src, M, dsize)
            assert np.array_equal(out, want), "%d pixels" % int((out != want).any(-1).sum())
        assert (want != R.emulate(src, M, 517, "direct")).any() and (want != R.emulate(src, M, 517, "bx0")).any()


# ---------------------------------------------------------------- per-frame matrices
def _frames_and_mats(n, seed):
    """n frames of one board, each with its own camera: distinct corners, distinct M"""
    from camkifu_amd import synth
    from oracle import oracle as ora
    rng = np.random.default_rng(seed)
    stones = synth.random_stones(rng, density=0.3)
    frames, mats = [], []
    for f in range(n):
        corners = synth.random_corners(240, 320, rng)
        frames.append(synth.render(240, 320, stones, corners, seed=seed * 100 + f).numpy())
        mats.append(ora.get_perspective_transform(corners, DST))
    mats = np.stack(mats)
    assert len({m.tobytes() for m in mats}) == n
    return np.stack(frames), mats


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n", [1, 3, 8])
def test_per_frame_matrices_warp(ck, ora, n):
    """m_count == n: frame k is warped with its own M, host frames and HBM frames with out= in HBM"""
    import torch
    frames, mats = _frames_and_mats(n, 40 + n)
    got = ck.warp_perspective(frames, mats)
    out = torch.zeros((n, 380, 380, 3), dtype=torch.uint8, device="cuda")
    ck.warp_perspective(_dev(frames), mats, out=out)
    got_d = _host(out)
    for k in range(n):
        one = ck.warp_perspective(frames[k], mats[k])
        assert np.array_equal(one, ora.warp_perspective(frames[k], mats[k])), k
        assert np.array_equal(got[k], one) and np.array_equal(got_d[k], one), k


@pytest.mark.parametrize("n", [1, 3, 8])
def test_per_frame_matrices_stones_detect(ck, n):
    from camkifu_amd.stone.nn_manager import NNManager
    ck.cnn_set_weights(NNManager.init_net())
    frames, mats = _frames_and_mats(n, 50 + n)
    for inp in (frames, _dev(frames)):
        labels, conf = ck.stones_detect(inp, mats)
        labels, conf = _host(labels), _host(conf)
        for k in range(n):
            l1, c1 = ck.stones_detect(frames[k], mats[k])
            assert np.array_equal(labels[k], l1[0]) and np.array_equal(conf[k], c1[0]), k


@pytest.mark.parametrize("n", [1, 3, 8])
def test_per_frame_matrices_stones_run(ck, ora, n):
    """ck_stones_run with one M per frame: the foreground counts equal the oracle chain (frame k warped with M_k,
    then MOG2 in frame order), the region answers equal the classifier's on those warps"""
    from camkifu_amd.stone.nn_manager import NNManager
    ck.cnn_set_weights(NNManager.init_net())
    frames, mats = _frames_and_mats(n, 60 + n)
    r = np.linspace(0.3, 0.05, n)
    for inp in (frames, _dev(frames)):
        hd, model = ck.mog2_create(380, 380), ora.MOG2(380, 380, 3)
        got = ck.stones_run(inp, mats, mog2=hd, learning_rates=r)
        fg, rl, rc = (_host(got[k]) for k in ("fgcount", "region_label", "region_conf"))
        gobans = np.stack([ora.warp_perspective(frames[k], mats[k]) for k in range(n)])
        rl2, rc2 = ck.cnn_regions(gobans)
        for k in range(n):
            assert np.array_equal(fg[k], S.zone_counts(model.apply(gobans[k], float(r[k])))), k
            assert np.array_equal(rl[k], rl2[k]) and np.array_equal(rc[k], rc2[k]), k
        ck.mog2_destroy(hd)


def test_m_count_other_than_1_or_n_is_refused(ck):
    from camkifu_amd import capi
    frames, mats = _frames_and_mats(3, 70)
    hd = ck.mog2_create(380, 380)
    for fr, M in ((frames, mats[:2]), (frames[0], mats), (frames[:2], mats)):
        with pytest.raises(capi.CkError):
            ck.warp_perspective(fr, M)
        with pytest.raises(capi.CkError):
            ck.stones_detect(fr, M)
        with pytest.raises(capi.CkError):
            ck.stones_run(fr, M, mog2=hd, learning_rates=np.full(len(fr) if fr.ndim == 4 else 1, 0.01))
    ck.mog2_destroy(hd)

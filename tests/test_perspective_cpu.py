"""K7 (ck_get_perspective_transform, the host Gauss-Jordan solve) against the 8 x 8 system solved exactly in rationals
from the same float32 corners, and the CPU side of the K8 references (tests/warp_ref.py): the oracle's warp against
the plain float64 warp and the kernel restatement, and the search for transforms that see the block association.

Error bar: per row i of M, sum_j |M_ij - E_ij| S_j / sum_j |E_ij| S_j with S = (max |x|, max |y|, 1) over the corners,
i.e. the error of each of the three numerator / denominator terms at the quad's extent against the terms themselves.
Board quads, 4K and negative coordinates: <= 1e-14 (measured <= 8e-16).  Three corners d px off a line: the solve
loses about log10(extent / d) digits, so the bar is 2^-50 * extent / d on top."""
import numpy as np
import pytest

from tests import warp_ref as R

DST = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)


def _row_err(M, corners, E):
    E = np.array([float(v) for v in E]).reshape(3, 3)
    M = np.asarray(M, np.float64).reshape(3, 3)
    c = np.asarray(corners, np.float32).astype(np.float64)
    S = np.array([np.abs(c[:, 0]).max(), np.abs(c[:, 1]).max(), 1.0])
    return ((np.abs(M - E) * S).sum(1) / (np.abs(E) * S).sum(1)).max()


def _both(corners, dst=DST):
    from camkifu_amd import capi
    from oracle import oracle as ora
    M = capi.get_perspective_transform(corners, dst)
    assert np.array_equal(M, ora.get_perspective_transform(corners, dst)), "host and oracle solves differ"
    return M


def _board_quads():
    from camkifu_amd import synth
    for seed in range(30):
        rng = np.random.default_rng(700 + seed)
        for h, w in ((480, 640), (1080, 1920), (2160, 3840)):
            yield synth.random_corners(h, w, rng)


def test_board_quads_against_the_exact_solve():
    worst = 0.0
    for c in _board_quads():
        worst = max(worst, _row_err(_both(c), c, R.exact_perspective(c, DST)))
    assert worst <= 1e-14, worst


@pytest.mark.parametrize("corners", [
    [(-500, -300), (3000, -200), (3800, 2100), (-100, 2000)],
    [(-3840, -2160), (-10, -2100), (-5, -3), (-3800, -20)],
    [(0.5, 0.25), (3839.5, 1.0), (3839, 2159.75), (2, 2159)],
    [(-0.375, 2159.5), (1919.25, -1.5), (3841, 1080.125), (1920, 2161)],
])
def test_4k_and_negative_coordinates(corners):
    c = np.array(corners, np.float32)
    E = R.exact_perspective(c, DST)
    assert _row_err(_both(c), c, E) <= 1e-14
    # and against a 4K square as the destination
    d4 = np.array([(0, 0), (3840, 0), (3840, 2160), (0, 2160)], np.float32)
    assert _row_err(_both(c, d4), c, R.exact_perspective(c, d4)) <= 1e-14


COLLINEAR = R.COLLINEAR


@pytest.mark.parametrize("quad,d", [(q, d) for q in (0, 1) for d in (1e-3, 1e-5, 1e-7, 1e-9)] +
                         [(2, d) for d in (1e-3, 1e-5, 1e-6)] +       # float32 holds -3 + d down to d = 2.4e-7
                         [(q, d) for q in (3, 4, 5) for d in (1e-3, 1e-4, 1e-5)])    # and 103 + d down to 7.6e-6
def test_nearly_collinear_corners(quad, d):
    c = np.array(COLLINEAR[quad], np.float32)
    c[1, 1] += np.float32(d)
    off = abs(float(c[1, 1]) - COLLINEAR[quad][1][1])
    assert off > 0
    E = R.exact_perspective(c, DST)
    assert E is not None
    M = _both(c)
    assert np.isfinite(M).all()
    extent = float(np.abs(c).max())
    assert _row_err(M, c, E) <= 1e-14 + 2.0 ** -50 * extent / off, (_row_err(M, c, E), off)


def test_exactly_collinear_corners():
    """the degenerate-quad behaviour.  |pivot| < 1e-300 fires only where elimination meets an exact zero: on the first
    two quads the exact 8 x 8 system is singular, and both solves refuse.  On y = -3 the exact system has a solution,
    a singular M with an all-zero first row, and elimination is exact there: both solves return that M, its inverse is
    zeros, and K8 maps every pixel to source (0, 0).  On a slanted line the exact solution is singular too, but the
    rounded one is not: det(M) ~ 1e-29 instead of 0, an inverse with entries up to ~1e19, and a warp that is an
    arbitrary image (reproducible: the kernel's arithmetic and the oracle's agree on it, tests/test_gpu_warp.py)"""
    from camkifu_amd import capi
    from oracle import oracle as ora
    for quad in COLLINEAR[:2]:
        c = np.array(quad, np.float32)
        assert R.exact_perspective(c, DST) is None
        with pytest.raises(capi.CkError):
            capi.get_perspective_transform(c, DST)
        with pytest.raises(ValueError):
            ora.get_perspective_transform(c, DST)
    c = np.array(COLLINEAR[2], np.float32)
    E = np.array([float(v) for v in R.exact_perspective(c, DST)]).reshape(3, 3)
    assert (E[0] == 0).all()
    M = _both(c)
    assert (M[0] == 0).all() and np.linalg.det(M) == 0
    assert np.abs(M - E).max() <= 1e-14 * np.abs(E).max()
    assert (R.host_inverse(M) == 0).all()
    rng = np.random.default_rng(84)
    for quad in COLLINEAR[3:]:
        c = np.array(quad, np.float32)
        E = R.exact_perspective(c, DST)
        assert E is not None and _det(E) == 0
        M = _both(c)
        assert np.isfinite(M).all()
        det = np.linalg.det(M)
        assert det != 0 and abs(det) <= 1e-25 * np.abs(M).max() ** 3, det
        inv = R.host_inverse(M)
        assert np.isfinite(inv).all() and np.abs(inv).max() >= 1e15, np.abs(inv).max()
        src = rng.integers(1, 256, (400, 640, 3), dtype=np.uint8)
        out = ora.warp_perspective(src, M)
        assert np.array_equal(out, R.emulate(src, M, 380))
        assert not (out == src[0, 0]).all(-1).all()            # not the singular-M fill


def _det(E):
    return (E[0] * (E[4] * E[8] - E[5] * E[7]) - E[1] * (E[3] * E[8] - E[5] * E[6]) +
            E[2] * (E[3] * E[7] - E[4] * E[6]))


def test_flipped_taps_on_the_bench_films():
    """the product's M against the exact M (each entry rounded once) through the kernel's own
    arithmetic on the bench films' transforms (1080p, seeds SEED .. SEED + 7 as --streams gives the ranks, and the 4K
    leg): 0 of 9 x 380 x 380 x 2 taps move by 1/32 px"""
    from camkifu_amd import capi, synth
    flipped = 0
    for h, w, seed in [(1080, 1920, synth.SEED + r) for r in range(8)] + [(2160, 3840, synth.SEED)]:
        c = synth.random_corners(h, w, np.random.default_rng(seed))
        Mp = capi.get_perspective_transform(c, DST)
        Me = np.array([float(v) for v in R.exact_perspective(c, DST)])
        a = R.kernel_taps(R.host_inverse(Mp), 380)
        b = R.kernel_taps(R.host_inverse(Me), 380)
        flipped += int((a[0] != b[0]).sum() + (a[1] != b[1]).sum())
    assert flipped == 0, flipped


# ---------------------------------------------------------------- K8 references on the CPU
DSIZES = [1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 127, 379, 380, 381, 517]


def test_kernel_restatement_equals_the_oracle(ora):
    """warp_ref.emulate (numpy) and ora.warp_perspective (C) restate the same arithmetic: bit-exact at every dsize, and
    both within the plain reference's band"""
    from camkifu_amd import synth
    sc = synth.scene(480, 640, seed=1)
    fr = sc["frame"].numpy()
    for d in DSIZES:
        dst = np.array([(0, 0), (d, 0), (d, d), (0, d)], np.float32)
        M = ora.get_perspective_transform(sc["corners"], dst)
        o = ora.warp_perspective(fr, M, (d, d))
        assert np.array_equal(R.emulate(fr, M, d), o), d
        cands, _ = R.reference(fr, M, d)
        assert not R.mismatch(o, cands).any(), d


def test_flip_search_finds_transforms_that_see_the_blocks(ora):
    """the searched transforms move taps between the three evaluation orders, and the image with them, so a kernel
    that dropped the block association (or evaluated the direct sum) differs from the oracle on them"""
    found = R.flip_search()
    assert len(found) == 3
    rng = np.random.default_rng(77)
    for M, nd, nz in found:
        src = rng.integers(0, 256, (160, 160, 3), dtype=np.uint8)
        e = R.emulate(src, M, 380)
        assert np.array_equal(e, ora.warp_perspective(src, M))
        assert (e != R.emulate(src, M, 380, "direct")).any(-1).sum() > 100, nd
        assert (e != R.emulate(src, M, 380, "bx0")).any(-1).sum() > 100, nz
        cands, band = R.reference(src, M, 380)
        assert band > 0 and not R.mismatch(e, cands).any()

"""ck_cluster_stones (camkifu_amd/csrc/k_cluster.hip: cv2.kmeans + SfClustering.find_stones, sf_clustering.py:48-168) against
the plain reference tests/cluster_ref.py, BIT FOR BIT: stones, trusted, ratios, centres (as bits), labels, passes per attempt,
the winning attempt, and the generator's state after the call -- on the inputs of tests/cluster_cases.py: the nine regions of
rendered boards at densities 0.1-0.7 and of a frame with a hand, uniform noise and smooth textures (several passes per
attempt, up to 23), flat colours (the empty-cluster rule, compactness 0), a learned zone table, pixel counts that are and
are not multiples of 1024 and 64, one-zone regions, the columns 6-13 job and the whole image (the streaming form of the
kernel; the whole image against the reference with integer sums rounded once).

Condition on the inputs, checked before a comparison is trusted: in the reference any two attempts' compactness values are
bit-equal or more than 1e-9 apart (relative), so the kernel's fixed-order double sum and the reference's sequential one rank
the attempts alike.  A job that violates it FAILS as a bad input.

Mutants of the kernel that must each fail this file.  Each was built as a library of its own and run against this file on
an MI355X (the tests that fail, of 21); the first five were also applied to the plain reference and compared with the
unmutated one on these very inputs (tests/test_cluster_ref_cpu.py::test_the_cases_tell_the_mutants_apart keeps that alive):
    first of equals (`<`) in the farthest-point rule    1: flat
    last minimum instead of first                      9: boards, noise, texture, flat, the sized and one-zone cases, ...
    15 passes instead of 100                           1: creep (the attempts that run 16 and 23 passes)
    the generator advanced by 20 per job               15: every case with more than one job, and the carried state
    rounding for truncation in the ratios              14: every case
    a float atomic in the compactness sum              1: whole (attempt 1 wins where the three attempts tie: 1 != 0).  Inside
                                                       one workgroup the LDS atomic's order happened to repeat on the smaller
                                                       jobs; test_results_repeat_bit_for_bit is there for the run it does not."""
import numpy as np
import pytest

from tests import cluster_cases as cc
from tests import cluster_ref as cr

pytestmark = pytest.mark.gpu
CASES = cc.cases()


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, rel_compact=1e-11):
    """got: (stones, trusted, extra) of the library; want: list of reference results"""
    stones, trusted, extra = got
    for j, w in enumerate(want):
        assert cr.attempts_separated(w["compactness"]), "bad input: job %d has attempts %r too close to rank" % (j, w["compactness"])
        tag = "job %d" % j
        assert list(extra["passes"][j]) == list(w["passes"]), tag
        assert int(extra["winner"][j]) == w["winner"], tag
        assert np.array_equal(extra["labels"][j], w["labels"]), tag
        assert np.array_equal(_bits(extra["centers"][j]), _bits(w["centers"])), tag
        assert np.array_equal(extra["ratios"][j], w["ratios"]), tag
        assert np.array_equal(stones[j], w["stones"]), tag
        assert bool(trusted[j]) == w["trusted"], tag
        # the compactness itself is a sum in another order: equal to rounding, and equal BITS between attempts where the
        # reference's are
        c, wc = extra["compactness"][j], np.array(w["compactness"])
        assert np.all(np.abs(c - wc) <= rel_compact * np.abs(wc)), tag
        for a in range(3):
            for b in range(a + 1, 3):
                assert (c[a] == c[b]) == (wc[a] == wc[b]), tag


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_output_equals_the_plain_reference(ck, case):
    name, imgs, rects, jobs, int_sums = case
    mask = cr.circle_mask(rects, cc.SIDE)
    ck.rng_state = 0xffffffff
    want, state = cc.reference(imgs, rects, mask, jobs, int_sums=int_sums)
    got = ck.cluster_stones(imgs, rects, mask, jobs=jobs, want_all=True)
    _same(got, want)
    assert ck.rng_state == state


def test_the_loop_and_the_shift_test_take_part():
    for name in ("noise", "texture", "creep"):
        _, imgs, rects, jobs, _ = next(c for c in CASES if c[0] == name)
        want, _ = cc.reference(imgs, rects, cr.circle_mask(rects, cc.SIDE), jobs)
        assert max(p for w in want for p in w["passes"]) > (15 if name == "creep" else 3)


def test_boards_are_read_correctly(ck):
    """the finder's point: in every region that holds two stones of each colour the stones equal the truth"""
    rects = cr.default_rects(cc.SIDE)
    mask = cr.circle_mask(rects, cc.SIDE)
    seen = 0
    for k, density in enumerate((0.3, 0.5, 0.7)):
        img, truth = cc.board(density, 90 + k)
        stones, trusted = ck.cluster_stones(img[None], rects, mask, jobs=cc.nine_jobs(1))
        for (a, b, c, d), st, ok in zip(cc.NINE, stones, trusted):
            part = truth[a:b, c:d]
            if (part == 1).sum() >= 2 and (part == 2).sum() >= 2:
                assert ok and np.array_equal(st[a:b, c:d], part), (density, a, c)
                seen += 1
    assert seen >= 20


def test_one_image_and_the_plain_call(ck):
    _, imgs, rects, jobs, _ = CASES[0]
    mask = cr.circle_mask(rects, cc.SIDE)
    ck.rng_state = 0xffffffff
    stones, trusted = ck.cluster_stones(imgs[3], rects, mask, rs=6, re=12, cs=12, ce=19)
    want = cr.find_stones(imgs[3], rects, mask, 6, 12, 12, 19, rng=cr.RNG())
    assert stones.shape == (19, 19) and np.array_equal(stones, want["stones"]) and trusted == want["trusted"]
    assert ck.rng_state == cr.RNG().advanced(21)
    # a batch without a job list: one job per image, same region
    ck.rng_state = 0xffffffff
    stones, trusted = ck.cluster_stones(imgs[:3], rects, mask, rs=6, re=12, cs=12, ce=19)
    want, state = cc.reference(imgs, rects, mask, [(f, 6, 12, 12, 19) for f in range(3)])
    assert np.array_equal(stones, np.stack([w["stones"] for w in want])) and list(trusted) == [w["trusted"] for w in want]
    assert ck.rng_state == state


def test_device_memory_gives_the_same(ck):
    import torch
    _, imgs, rects, jobs, _ = CASES[0]
    mask = cr.circle_mask(rects, cc.SIDE)
    ck.rng_state = 0xffffffff
    host = ck.cluster_stones(imgs, rects, mask, jobs=jobs, want_all=True)
    ck.rng_state = 0xffffffff
    dev = ck.cluster_stones(torch.from_numpy(imgs).cuda(), rects, mask, jobs=jobs, want_all=True)
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])
    for key in ("ratios", "centers", "passes", "compactness", "winner"):
        assert np.array_equal(host[2][key], dev[2][key]), key
    assert all(np.array_equal(a, b) for a, b in zip(host[2]["labels"], dev[2]["labels"]))


def test_two_calls_carry_the_generator(ck):
    _, imgs, rects, _, _ = next(c for c in CASES if c[0] == "texture")
    mask = cr.circle_mask(rects, cc.SIDE)
    jobs = cc.nine_jobs(1)
    ck.rng_state = 0xffffffff
    first = ck.cluster_stones(imgs, rects, mask, jobs=jobs[:4], want_all=True)
    mid = ck.rng_state
    second = ck.cluster_stones(imgs, rects, mask, jobs=jobs[4:], want_all=True)
    w1, s1 = cc.reference(imgs, rects, mask, jobs[:4])
    w2, s2 = cc.reference(imgs, rects, mask, jobs[4:], state=s1)
    assert mid == s1 and ck.rng_state == s2
    _same(first, w1)
    _same(second, w2)
    # setting the state reproduces a call
    ck.rng_state = s1
    again = ck.cluster_stones(imgs, rects, mask, jobs=jobs[4:], want_all=True)
    assert np.array_equal(again[2]["centers"].view(np.uint32), second[2]["centers"].view(np.uint32))
    assert np.array_equal(again[2]["passes"], second[2]["passes"]) and np.array_equal(again[0], second[0])
    # and a fresh context starts from the library's default seed
    from camkifu_amd import capi
    other = capi.Context(0)
    assert other.rng_state == 0xffffffff
    other.close()


def test_results_repeat_bit_for_bit(ck):
    """a fixed-order reduction: the same call gives the same bits, and attempts that reach the same partition tie exactly"""
    for name in ("boards", "columns"):
        _, imgs, rects, jobs, _ = next(c for c in CASES if c[0] == name)
        mask = cr.circle_mask(rects, cc.SIDE)
        runs = []
        for _ in range(3):
            ck.rng_state = 12345
            runs.append(ck.cluster_stones(imgs, rects, mask, jobs=jobs, want_all=True)[2])
        for r in runs[1:]:
            assert np.array_equal(r["compactness"].view(np.uint64), runs[0]["compactness"].view(np.uint64))
            assert np.array_equal(r["passes"], runs[0]["passes"]) and np.array_equal(r["winner"], runs[0]["winner"])
        ties = sum(1 for c in runs[0]["compactness"] if c[0] == c[1] or c[0] == c[2]) if name == "boards" else len(jobs)
        assert ties >= len(jobs) // 2, "the attempts of a rendered board usually tie: %d of %d" % (ties, len(jobs))


def _accumulated(seed):
    """what SfClustering._find builds: an f32 running average (weight 0.2) of a few noisy frames of one board"""
    stones = None
    accu = None
    for k in range(4):
        img, stones = cc.board(0.5, seed)
        from camkifu_amd import synth
        img = synth.render(cc.SIDE, cc.SIDE, stones, cc.CORNERS, seed=seed + 100 * k).numpy()
        accu = img.astype(np.float32) if accu is None else (np.float32(0.8) * accu + np.float32(0.2) * img.astype(np.float32))
    return np.ascontiguousarray(accu, np.float32)


def test_float_images(ck):
    _, imgs, rects, jobs, _ = CASES[0]
    mask = cr.circle_mask(rects, cc.SIDE)
    few = jobs[18:36]
    # floats that hold integers: bit-equal to the uint8 path (and so to the reference)
    ck.rng_state = 0xffffffff
    as_u8 = ck.cluster_stones(imgs, rects, mask, jobs=few, want_all=True)
    ck.rng_state = 0xffffffff
    as_f32 = ck.cluster_stones(imgs.astype(np.float32), rects, mask, jobs=few, want_all=True)
    assert np.array_equal(as_u8[0], as_f32[0]) and np.array_equal(as_u8[1], as_f32[1])
    for key in ("ratios", "passes", "winner"):
        assert np.array_equal(as_u8[2][key], as_f32[2][key]), key
    assert np.array_equal(_bits(as_u8[2]["centers"]), _bits(as_f32[2]["centers"]))
    assert np.array_equal(as_u8[2]["compactness"].view(np.uint64), as_f32[2]["compactness"].view(np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(as_u8[2]["labels"], as_f32[2]["labels"]))
    # non-integer floats: the same bits run to run; each centre within n_k * 2^-24 (relative) of the reference's, whose
    # sequential f32 sum over the n_k pixels of a cluster carries that much error
    accu = _accumulated(61)[None]
    cols = np.array([(0, 0, 19, 6, 13), (0, 6, 12, 6, 12)], np.int32)
    outs = []
    for _ in range(2):
        ck.rng_state = 0xffffffff
        outs.append(ck.cluster_stones(accu, rects, mask, jobs=cols, want_all=True))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(_bits(outs[0][2]["centers"]), _bits(outs[1][2]["centers"]))
    assert np.array_equal(outs[0][2]["compactness"].view(np.uint64), outs[1][2]["compactness"].view(np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(outs[0][2]["labels"], outs[1][2]["labels"]))
    want, _ = cc.reference(accu, rects, mask, cols)
    for j, w in enumerate(want):
        for k in range(3):
            n_k = int((w["labels"] == k).sum())
            err = np.abs(outs[0][2]["centers"][j, k].astype(np.float64) - w["centers"][k].astype(np.float64))
            print("f32 job %d cluster %d: n_k %d, centre error %r, bound %r" % (j, k, n_k, err.max(), (n_k * 2.0 ** -24 * np.abs(w["centers"][k])).min()))
            assert np.all(err <= n_k * 2.0 ** -24 * np.abs(w["centers"][k].astype(np.float64))), (j, k)


def test_argument_errors(ck):
    from camkifu_amd import capi
    _, imgs, rects, jobs, _ = CASES[0]
    mask = cr.circle_mask(rects, cc.SIDE)
    ck.rng_state = 77
    for bad in ([(0, 6, 6, 0, 6)], [(0, 0, 6, 12, 20)], [(0, -1, 6, 0, 6)], [(7, 0, 6, 0, 6)], [(0, 0, 6, 0, 6), (0, 8, 3, 0, 6)]):
        with pytest.raises(capi.CkError):
            ck.cluster_stones(imgs, rects, mask, jobs=bad)
    outside = rects.copy()
    outside[18, 18, 2] = cc.SIDE + 5
    with pytest.raises(capi.CkError):
        ck.cluster_stones(imgs, outside, mask, jobs=[(0, 12, 19, 12, 19)])
    tiny = cc.square_rects(1)
    tiny[0, 1] = (0, 1, 1, 3)                                    # a 1 x 2 view: fewer than 3 pixels
    with pytest.raises(capi.CkError):
        ck.cluster_stones(imgs, tiny, mask, jobs=[(0, 0, 1, 1, 2)])
    with pytest.raises(ValueError):
        ck.cluster_stones(imgs.astype(np.int32), rects, mask, jobs=jobs)
    assert ck.rng_state == 77                                    # a refused call draws nothing

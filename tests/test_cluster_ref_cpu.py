"""The plain reference of the k-means stones finder (tests/cluster_ref.py) on cases worked by hand, so that what the GPU file
compares the kernel with is itself pinned: the generator's first outputs, flat colours (centres known, compactness 0, the
empty-cluster rule), rendered boards read correctly, check_density; and the check that the GPU file's inputs tell its
listed mutants apart."""
import numpy as np
import pytest

from tests import cluster_cases as cc
from tests import cluster_ref as cr


def test_generator_first_outputs():
    # by hand: 0xffffffff * 4164903690 (0xf83f630a) + 0 = 0xf83f6309_07c09cf6 -> output 0x07c09cf6, carry 0xf83f6309
    assert 0xffffffff * 0xf83f630a == 0xf83f630907c09cf6
    rng = cr.RNG()
    assert [rng.next() for _ in range(3)] == [0x07c09cf6, 0xb302a6a5, 0xe6abd4e7]
    assert rng.state == 0xad96e457e6abd4e7
    assert cr.RNG().advanced(3) == 0xad96e457e6abd4e7 and cr.RNG(5).advanced(0) == 5
    assert cr.RNG().real() == 0x07c09cf6 / 2.0 ** 32


def test_a_call_draws_21_numbers_whatever_the_data():
    for img in (cc.flat_image([(90, 100, 110)]), cc.noise_image(1)):
        rng = cr.RNG()
        cr.find_stones(img, cr.default_rects(), np.ones((380, 380), np.uint8), 6, 12, 6, 12, rng=rng)
        assert rng.state == cr.RNG().advanced(21)


def _px(colours, counts):
    return np.concatenate([np.tile(np.array(c, np.float32), (n, 1)) for c, n in zip(colours, counts)])


def test_three_flat_colours():
    """k-means++ never seeds a colour twice while another is left (a pixel at distance 0 cannot end the walk), so every attempt
    starts on the three colours: the first assignment has compactness exactly 0, the centres computed after it are the
    colours up to the rounding of sum * (1.f / count), and the finder reports 'not trusted'"""
    cols = [(20, 30, 40), (120, 130, 140), (220, 230, 240)]
    for seed in (0xffffffff, 1, 2, 12345):
        km = cr.kmeans3(_px(cols, (50, 70, 30)), cr.RNG(seed))
        assert np.allclose(np.sort(km["centers"], axis=0), np.array(cols, float), rtol=0, atol=1e-4)
        assert km["compactness"] == [0.0, 0.0, 0.0] and km["winner"] == 0 and km["passes"] == [2, 2, 2]
    rects = cr.default_rects()
    out = cr.find_stones(cc.flat_image(cols), rects, cr.circle_mask(rects, 380), 6, 12, 6, 12)
    assert not out["trusted"] and not out["stones"].any()


def test_two_and_one_flat_colours_take_the_empty_cluster_rule():
    # two colours: some cluster is empty after the first assignment, and gets the LAST pixel (<=) of the most populous one
    px = _px([(10, 10, 10), (200, 200, 200)], (6, 4))
    km = cr.kmeans3(px, cr.RNG())
    assert min(km["compactness"]) == 0.0
    assert len(set(km["labels"][:6])) + len(set(km["labels"][6:])) == 3        # one colour split over two clusters
    # one colour: all three seeds are pixel 0 (p = 0 stops the walk at once), every pixel goes to cluster 0, then cluster 1
    # takes the last pixel and cluster 2 the one before
    km = cr.kmeans3(_px([(90, 100, 110)], (8,)), cr.RNG())
    assert km["labels"].tolist() == [0, 0, 0, 0, 0, 0, 2, 1] and km["passes"] == [2, 2, 2] and km["winner"] == 0
    assert np.array_equal(km["centers"], np.tile(np.float32([90, 100, 110]), (3, 1)))
    first = cr.kmeans3(_px([(90, 100, 110)], (8,)), cr.RNG(), farthest_last=False)
    assert first["labels"].tolist() == [1, 2, 0, 0, 0, 0, 0, 0]


def test_seeding_walk_by_hand():
    """four pixels on a line, first centre = pixel (0x07c09cf6 % 4) = 2; distances to it 400, 100, 0, 900 (sum 1400)"""
    px = np.float32([[0, 0, 0], [10, 0, 0], [20, 0, 0], [50, 0, 0]])
    rng = cr.RNG()
    seeds = cr.seed_pp(px, rng)
    assert seeds[0] == 0x07c09cf6 % 4 == 2
    # trial draws: 0xb302a6a5 / 2^32 = 0.699.. -> p = 978.9 -> 400, 100, 0 subtracted leave 478.9 > 0 -> pixel 3 (N - 1);
    # 0xe6abd4e7 / 2^32 = 0.901 -> pixel 3 again; the third by the reference's own arithmetic
    assert seeds[1] == 3
    assert rng.state == cr.RNG().advanced(7)


@pytest.mark.parametrize("density", [0.3, 0.5, 0.7])
def test_rendered_boards_are_read_correctly(density):
    rects = cr.default_rects()
    mask = cr.circle_mask(rects, 380)
    img, truth = cc.board(density, 90 + int(density * 10))
    seen = 0
    for a, b, c, d in cc.NINE:
        part = truth[a:b, c:d]
        if (part == 1).sum() >= 2 and (part == 2).sum() >= 2:
            out = cr.find_stones(img, rects, mask, a, b, c, d)
            assert out["trusted"] and np.array_equal(out["stones"][a:b, c:d], part)
            assert not out["stones"][:a].any() and not out["stones"][:, :c].any()
            seen += 1
    assert seen >= 5


def test_check_density():
    st = np.zeros((19, 19), np.uint8)
    assert not cr.check_density(st)
    st[0, :2] = 1
    assert not cr.check_density(st)                  # no white
    st[1, 0] = 2
    assert not cr.check_density(st)                  # white once
    st[1, 1] = 2
    assert cr.check_density(st)


def test_mask_and_default_rects():
    rects = cr.default_rects()
    assert tuple(rects[0, 0]) == (0, 0, 20, 20) and tuple(rects[18, 18]) == (360, 360, 379, 379) and tuple(rects[5, 7]) == (100, 140, 120, 160)
    mask = cr.circle_mask(rects, 380)
    assert mask[10, 10] == 1 and mask[0, 0] == 0 and mask[379, 5] == 0 and set(np.unique(mask)) == {0, 1}
    assert mask[100:120, 140:160].sum() == sum(1 for y in range(20) for x in range(20) if (x - 10) ** 2 + (y - 10) ** 2 <= 100)


MUTANTS = [("farthest_first", dict(farthest_last=False)), ("last_minimum", dict(first_min=False)), ("passes_15", dict(max_passes=15)),
           ("rounding", dict(rounding=True)), ("draws_20", dict(draws=20))]


def _differs(a, b):
    return not (np.array_equal(a["ratios"], b["ratios"]) and np.array_equal(a["labels"], b["labels"]) and a["passes"] == b["passes"]
                and np.array_equal(a["centers"].view(np.uint32), b["centers"].view(np.uint32)) and a["winner"] == b["winner"])


def test_the_cases_tell_the_mutants_apart():
    """each mutant of tests/test_gpu_cluster.py's list, applied to the reference, changes the result of some job of the GPU
    file's inputs; and every job meets the condition on its attempts' compactness"""
    caught = {name: 0 for name, _ in MUTANTS}
    for name, imgs, rects, jobs, int_sums in cc.cases():
        if name in ("columns", "whole", "learned", "hand"):
            continue                                  # (large or redundant for this purpose)
        mask = cr.circle_mask(rects, cc.SIDE)
        plain, _ = cc.reference(imgs, rects, mask, jobs, int_sums=int_sums)
        assert all(cr.attempts_separated(r["compactness"]) for r in plain), name
        for mutant, how in MUTANTS:
            other, _ = cc.reference(imgs, rects, mask, jobs, int_sums=int_sums, **how)
            caught[mutant] += sum(_differs(a, b) for a, b in zip(plain, other))
    assert all(n > 0 for n in caught.values()), caught

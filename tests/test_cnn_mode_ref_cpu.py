"""The rounding models of tests/cnn_mode_ref.py and the exact cases of tests/cnn_exact_cases.py held to what they claim,
on the CPU: the fp32 model is the float64 network the other classifier tests use; every (case, mode) pair the GPU test
runs passes the audit that makes "bit for bit" legitimate; on an exact case the models of all its modes agree; the cases
reach every weight of every layer; and every listed way of getting a mode wrong changes the bits of some case."""
import numpy as np
import pytest

from tests import cnn_exact_cases as ec
from tests import cnn_mode_ref as mr
from tests import cnn_pack_ref as pk

_runs = {}


def _run(name, mode):
    """the audit and the model's outputs of (case, mode), computed once"""
    if (name, mode) not in _runs:
        c, out = ec.case(name), {}
        _runs[name, mode] = (mr.audit(c["W"], c["gobans"], mode, outputs=out), out)
    return _runs[name, mode]


def test_e4m3_rounding_is_the_packers():
    """mr.e4m3_round (arithmetic) against the code table of tests/cnn_pack_ref.py, which test_cnn_pack_cpu.py holds to
    the bytes of ck_cnn_pack.cpp: every code's value, every midpoint between two codes, seeded values, the saturation"""
    vals = pk.e4m3_values()
    mags = vals[:0x7F]
    rng = np.random.default_rng(3)
    v = np.concatenate([mags, (mags[1:] + mags[:-1]) / 2, np.nextafter((mags[1:] + mags[:-1]) / 2, 0), [449.0, 1000.0, 2.0 ** -11],
                        rng.standard_normal(4000) * 10.0 ** rng.integers(-4, 3, 4000)])
    v = np.concatenate([v, -v])
    assert np.array_equal(mr.e4m3_round(v), vals[pk.e4m3(v)])


def test_splits_round_as_the_kernels_do():
    """split_act: both halves towards zero, hi + lo = x for values of up to 22 bits; an fp16-subnormal lo is kept"""
    x = np.array([2049.0, -2049.0, 1035.9375, 2.0 ** -3 + 2.0 ** -22, 65503.0, 1 + 2.0 ** -11 + 2.0 ** -21, 0.1])
    hi, lo = mr.split_act(x)
    assert np.array_equal(hi[:5], [2048.0, -2048.0, 1035.0, 2.0 ** -3, 65472.0]) and np.array_equal(lo[:4], [1.0, -1.0, 0.9375, 2.0 ** -22])
    assert np.array_equal((hi + lo)[:6], x[:6]) and abs(hi[6] + lo[6] - np.float32(0.1)) < 2.0 ** -22 * 0.1 * 4
    assert np.all(np.abs(hi) <= np.abs(x)) and np.all(np.abs(hi + lo) <= np.abs(mr.f32(x)))
    assert mr.split_act(x, ("flush_lo",))[1][3] == 0
    assert np.array_equal(mr.bf16_rne(np.array([257.0, 259.0, 257.25, -0.0, 1 + 2.0 ** -9])), [256.0, 260.0, 258.0, 0.0, 1.0])
    assert np.array_equal(mr.bf16_trunc(np.array([259.0, 257.25])), [258.0, 256.0])


@pytest.fixture(scope="module")
def torch64():
    from tests.test_gpu_parity import _torch_fp64_classifier, _torch_fp64_maps
    return _torch_fp64_maps, _torch_fp64_classifier


def _close(got, want):
    return np.abs(got - want).max() <= 1e-12 * max(1.0, float(np.abs(want).max()))


def test_fp32_model_is_the_float64_network_on_seeded_weights(torch64):
    from camkifu_amd import synth
    maps, classifier = torch64
    g = np.random.default_rng(23).integers(0, 256, (2, 380, 380, 3), dtype=np.uint8)
    for _, W in ec.realistic_weights(synth):
        o = mr.forward(W, g, "fp32")
        t2, t4 = maps(W, g)
        assert _close(o["pool2"], t2) and _close(o["pool4"], t4) and _close(o["y"], classifier(W, g))


@pytest.mark.parametrize("name", ec.NAMES)
def test_exact_case_passes_its_audits_and_its_models_agree(name, torch64):
    """what makes "bit for bit" legitimate, for every (case, mode) pair of the GPU test: operands unchanged by the mode's
    roundings, no lo * lo product, sums within 2^20 quanta, magnitudes inside the modes' limits.  Then the float64
    result is the one right answer: the models of all the case's modes return the same bits (agree), and mode fp32 is
    the float64 torch network."""
    c = ec.case(name)
    maps, classifier = torch64
    for mode in c["modes"]:
        a, _ = _run(name, mode)
        assert all(v["ok"] for v in a.values()), (name, mode, {k: v for k, v in a.items() if not v["ok"]})
    first = _run(name, c["modes"][0])[1]
    if c["agree"]:
        for mode in c["modes"][1:]:
            o = _run(name, mode)[1]
            for k in ("pool2", "pool4", "h1", "logits", "y"):
                assert np.array_equal(first[k], o[k]), (name, mode, k)
    if "fp32" in c["modes"]:
        o = _run(name, "fp32")[1]
        t2, t4 = maps(c["W"], c["gobans"])
        assert _close(o["pool2"].reshape(t2.shape), t2) and _close(o["pool4"].reshape(t4.shape), t4)
        assert _close(o["y"].reshape(-1, 100, 81), classifier(c["W"], c["gobans"]))
    assert first["pool2"].max() > 0 and first["pool4"].max() > 0          # the maps are alive


def test_cases_reach_every_weight():
    """every (kernel row, kernel column, input channel, output channel) of the four convolutions and every (k, output)
    of both dense layers is nonzero in some case; output channels 80 .. 89 of conv3 / conv4 and dense-2 outputs 64 .. 80
    are alive in the padding case, whose image is 255 everywhere"""
    for k in ("c1w", "c2w", "c3w", "c4w", "d1w", "d2w"):
        seen = np.zeros(ec.WEIGHT_SHAPES[k], bool)
        for name in ec.NAMES:
            seen |= ec.case(name)["W"][k] != 0
        assert seen.all(), k
    p = ec.case("padding")
    assert (p["gobans"] == 255).all()
    assert np.abs(p["W"]["c3w"][..., 80:]).sum() > 0 and np.abs(p["W"]["c4w"][..., 80:]).sum() > 0 and np.abs(p["W"]["d2w"][:, 64:]).sum((0,)).all()
    o = _run("padding", "fp32")[1]
    assert (o["pool4"][..., 80:] > 0).all() and len(np.unique(o["pool4"][..., 80:])) == 1


def _taps_with(mask):
    """the set of (kernel row, kernel column) at which a boolean HWIO array holds a True"""
    return {(int(i), int(j)) for i, j in zip(*np.nonzero(mask.any(axis=(2, 3))))}


def test_lo_cases_hold_what_they_are_for():
    """weight lo: 12 .. 22 significant bits in the weights of one layer, at EVERY kernel position of that convolution (the
    kernels have unrolled code per tap, per pair of tap columns and per vertical tap), and none elsewhere; activation lo:
    the mirror -- every kernel position of conv2, conv3 and conv4 carries a weight whose input channel has activation
    lo halves, and no weight has a lo; alo_sub: the lo halves are fp16 subnormals"""
    for layer in ("c1", "c2", "c3", "c4", "d1"):
        c = ec.case("wlo_" + layer)
        w = c["W"][layer + "w"]
        hi, lo = mr.split_weight(w[w != 0])
        assert (lo != 0).sum() >= lo.size - (layer == "d1")            # (dense 1: one unit without a lo, its twin's rival)
        if layer != "d1":
            kh, kw = w.shape[:2]
            assert _taps_with(mr.split_weight(w)[1] != 0) == {(i, j) for i in range(kh) for j in range(kw)}, layer
        for other in ("c1", "c2", "c3", "c4", "d1"):
            if other != layer:
                assert not mr.split_weight(c["W"][other + "w"])[1].any()
    c, keep = ec.case("alo"), {}
    p2 = mr.stage_a(c["W"], c["gobans"], "f16x2", keep=keep)
    p4 = mr.stage_b(c["W"], p2, "f16x2", keep=keep)
    for a in (keep["a1"], p2, keep["a3"], p4):
        assert (mr.split_act(a)[1] != 0).mean() > 0.2 and (mr.split_act_q8(a)[2] != 0).mean() > 0.2
    for k, a in (("c2w", keep["a1"]), ("c3w", p2), ("c4w", keep["a3"])):
        w = c["W"][k]
        for split in (lambda v: mr.split_act(v)[1], lambda v: mr.split_act_q8(v)[2]):
            has_lo = (split(a) != 0).any(axis=(0, 1, 2))                       # per input channel
            assert _taps_with((w != 0) & has_lo[None, None, :, None]) == {(i, j) for i in range(w.shape[0]) for j in range(w.shape[1])}, k
    for k in ("c2w", "c3w", "c4w", "d1w"):
        assert not mr.split_weight(c["W"][k])[1].any()
    c, keep = ec.case("alo_sub"), {}
    mr.stage_a(c["W"], c["gobans"], "f16x2", keep=keep)
    lo = mr.split_act(keep["a1"])[1]
    assert set(np.unique(lo)) == {0.0, 2.0 ** -22} and 2.0 ** -22 < 2.0 ** -14 and keep["a1"].max() <= 2.0 ** -3 * (1 + 2.0 ** -19)
    for k in ("c2w", "c3w", "c4w"):                                            # the subnormal lo meets every kernel position too
        w = c["W"][k]
        assert _taps_with(w != 0) == {(i, j) for i in range(w.shape[0]) for j in range(w.shape[1])}, k


def test_bf16_round_case_has_ties_on_both_sides_and_a_minus_zero():
    c = ec.case("bf16_round")
    W = c["W"]
    x = mr.gather(c["gobans"])
    s = mr._layer(x, W["c1w"], W["c1b"], "bf16", "c1", (), np.float64, first=True)
    down, ulp = mr.bf16_trunc(s), mr.bf16_ulp(s)
    tie = (s > 0) & (s - down == ulp / 2)
    up = mr.bf16_rne(s) > s
    assert (tie & up).sum() > 1000 and (tie & ~up).sum() > 1000              # halfway, the even neighbour above / below
    near = (s > 0) & ~tie & (np.abs(s - down - ulp / 2) <= ulp / 4) & (s != down)
    assert near.sum() > 1000                                                 # just off the tie
    assert (s < 0).sum() > 1000                                              # negatives before the relu
    for k in ("c1b", "c2b", "c3b", "c4b"):
        assert (mr.bf16_rne(W[k]) != W[k]).any()                             # biases that are no bf16 numbers
    # a real -0 before the relu: conv2's channel 31 and conv3's channel 89 (all weights -0.0 or negative, bias -0.0) sum
    # nothing but -0 over the blacked-out rectangle and are negative elsewhere; the pool hands the -0 on, the rounding
    # keeps it (0x8000), the relu has to return +0 bits
    keep = {}
    p2 = mr.stage_a(W, c["gobans"], "bf16", keep=keep)
    s2 = mr._layer(keep["a1"], W["c2w"], W["c2b"], "bf16", "c2", (), np.float64)
    s3 = mr._layer(p2, W["c3w"], W["c3b"], "bf16", "c3", (), np.float64)
    for s, ch in ((s2, 31), (s3, 89)):
        zero = s[..., ch] == 0
        assert zero.sum() > 1000 and np.signbit(s[..., ch][zero]).all() and (s[..., ch] < 0).sum() > 1000
        assert not np.signbit(np.delete(s, ch, axis=-1)[np.delete(s, ch, axis=-1) == 0]).any()
    pooled = mr.pool(s2)[..., 31]
    assert np.signbit(pooled[pooled == 0]).all() and np.signbit(mr.bf16_rne(pooled)[pooled == 0]).all() and (pooled == 0).sum() > 100
    o = _run("bf16_round", "bf16")[1]
    assert not np.signbit(o["pool2"]).any() and not np.signbit(o["pool4"]).any()
    assert not o["pool2"][..., 31].any() and o["pool2"][..., 4].any()


def test_ties_case_has_equal_best_logits():
    o = _run("ties", "fp32")[1]
    lg = o["logits"]
    best = lg == lg.max(axis=1, keepdims=True)
    sets = {tuple(np.nonzero(b)[0]) for b in best}
    assert {(15, 16), (79, 80), (0, 80), (15, 16, 79, 80), (0, 15, 16, 80), tuple(range(81))} <= sets
    lab = mr.decode(o["y"].reshape(1, 100, 81))[0][0]
    assert np.array_equal(lab, [np.nonzero(b)[0][0] for b in best])
    assert (mr.decode(o["y"].reshape(1, 100, 81), last=True)[0][0] != lab).sum() >= 6


# what a wrong kernel could do -> (mode it would be wrong in, the case that has to see it)
MUTANTS = [("drop_hilo_" + L, m, "wlo_" + L) for L in ("c1", "c2", "c3", "c4", "d1") for m in ("f16x2", "f16q8")] + \
          [("near_hilo_" + L, m, "wlo_" + L) for L in ("c1", "c2", "c3", "c4", "d1") for m in ("f16x2", "f16q8")] + \
          [(k + "_lohi_" + L, m, "alo") for k in ("drop", "near") for L in ("c2", "c3", "c4", "d1") for m in ("f16x2", "f16q8")] + \
          [("flush_lo", "f16x2", "alo_sub"), ("bf16_trunc", "bf16", "bf16_round"), ("bf16_skip_c1", "bf16", "bf16_round"),
           ("bf16_skip_c3", "bf16", "bf16_round"), ("bf16_bias", "bf16", "bf16_round")] + \
          [(k + L, "fp32", "taps_" + L) for k in ("shift_", "noflip_") for L in ("c1", "c2", "c3", "c4")] + \
          [(k + L, "fp32", "gather") for k in ("shift_", "noflip_") for L in ("c1", "c2", "c3", "c4")] + \
          [("origin9_320", "fp32", "gather"), ("origin9_339", "fp32", "gather"), ("argmax_last", "fp32", "ties"),
           ("pad_tap6", "fp32", "taps_c1"), ("pad_tap6", "bf16", "gather"), ("pad_d2", "fp32", "padding")]


@pytest.mark.parametrize("mutant, mode, name", MUTANTS)
def test_cases_tell_the_mutants_apart(mutant, mode, name):
    """every listed mistake changes the bits of pool2 or pool4 or a label of the case named for it.  Dense 1 reaches no
    map: its a_hi * w_lo term decides a label of wlo_d1 (dropped; read from the neighbouring k it keeps its sign and the
    label), and every dense-1 cross-term mutant and dense 2's pad column move y by more than the GPU test's bound on it.
    (The issue's "origin 340 replaced by 360 - 40 + 20" IS 340; the two wrong origins tried are 320, region 8 again,
    and 339.)"""
    c = ec.case(name)
    good = _run(name, mode)[1]
    lab = mr.decode(good["y"].reshape(-1, 100, 81))[0]
    if mutant == "argmax_last":
        assert not np.array_equal(mr.decode(good["y"].reshape(-1, 100, 81), last=True)[0], lab)
        return
    bad = dict(good)                               # the layers before the mutated one are the good run's
    if mutant[-2:] in ("c3", "c4"):
        bad["pool4"] = mr.stage_b(c["W"], good["pool2"], mode, (mutant,))
    elif mutant[-2:] != "d1" and mutant != "pad_d2":
        bad = mr.forward(c["W"], c["gobans"], mode, mut=(mutant,))
    if bad.get("y") is good["y"]:
        bad["h1"], bad["logits"], bad["y"] = mr.stage_c(c["W"], bad["pool4"], mode, (mutant,))
    seen = [k for k in ("pool2", "pool4") if not np.array_equal(bad[k].reshape(good[k].shape), good[k])]
    if not np.array_equal(mr.decode(bad["y"].reshape(-1, 100, 81))[0], lab):
        seen.append("labels")
    if mutant == "drop_hilo_d1":
        assert "labels" in seen, (mutant, mode)    # (logits 3 and 5 of wlo_d1 differ by a_hi * w_lo alone)
    if mutant.endswith("_d1") or mutant == "pad_d2":
        assert np.abs(bad["y"].reshape(good["y"].shape) - good["y"]).max() > 4 * ec.Y_EXACT, (mutant, mode)
    else:
        assert seen, (mutant, mode, name)
    expect = {"c1": "pool2", "c2": "pool2", "c3": "pool4", "c4": "pool4"}.get(mutant[-2:])
    if expect and not mutant.startswith("bf16_skip"):
        assert expect in seen, (mutant, seen)


def test_bf16_model_against_itself_at_realistic_magnitudes(ora):
    """the yardsticks of the GPU test's realistic tier: float32 against float64 accumulation of the SAME roundings, staged
    as the GPU test stages them, on its inputs.  The model alone differs in under 1 % of a stage's elements (chained
    through all four convolutions too) and stays within half of each bound the GPU test allows (ec.A_REAL, ec.Y_REAL
    are 4 x what this measured when they were set; float32 sums depend on the BLAS's blocking, so the figures -- printed --
    may move a little between machines)."""
    from camkifu_amd import synth
    g = ec.realistic_gobans(ora, synth)
    R = list(ec.REAL_REGIONS)
    for wname, W in ec.realistic_weights(synth):
        for k in range(2):
            x = mr.gather(g[k])[R]
            p2 = mr.stage_a(W, None, "bf16", patches=x)
            p2f = mr.stage_a(W, None, "bf16", patches=x, acc=np.float32)
            p4 = mr.stage_b(W, p2, "bf16")
            p4f = mr.stage_b(W, p2, "bf16", acc=np.float32)
            p4c = mr.stage_b(W, p2f, "bf16", acc=np.float32)
            y = mr.stage_c(W, p4, "bf16")[2]
            yf = mr.stage_c(W, p4, "bf16", acc=np.float32)[2]
            fig = dict(A=mr.compare_maps(p2f, p2), B=mr.compare_maps(p4f, p4), chained=mr.compare_maps(p4c, p4), C=float(np.abs(y - yf).max()))
            print(wname, ("scene", "noise")[k], fig)
            for s in ("A", "B", "chained"):
                assert fig[s][0] < 0.01, (wname, k, s, fig)
            assert max(fig["A"][1], fig["B"][1]) <= ec.A_REAL / 2 and fig["C"] <= ec.Y_REAL / 2, (wname, k, fig)


def test_softmax_bound_of_the_exact_tier():
    """ec.Y_EXACT is 4 x the largest gap between fc2_softmax_kernel's arithmetic in numpy float32 and the float64 softmax
    over the exact cases' logits"""
    worst = 0.0
    for name in ec.NAMES:
        lg = _run(name, ec.case(name)["modes"][0])[1]["logits"]
        worst = max(worst, float(np.abs(mr.softmax32_kernel_order(lg).astype(np.float64) - mr.softmax64(lg)).max()))
    print("largest |softmax32 - softmax64| over the exact cases: %.3g" % worst)
    assert worst <= ec.Y_EXACT / 2

"""K10..K12 in all four CK_CNN_* modes, bit for bit.

Exact tier.  tests/cnn_exact_cases.py holds networks and images on which the classifier's arithmetic is exact in the
modes listed for each (tests/test_cnn_mode_ref_cpu.py asserts the audit of every (case, mode) pair on the CPU: operands
unchanged by the mode's roundings, no lo * lo product, every sum within 2^20 quanta).  The float64 evaluation of
tests/cnn_mode_ref.py is then the one right answer and the kernels owe its bits: pool2 and pool4 as float32 bit
patterns, every label, tie or not, region_conf as y[label] / sum of y in double from the GPU's own y.  Only y itself
goes through expf and a division: it is held to ec.Y_EXACT = 4 x 1.03e-7 = 4.12e-7, four times the largest gap between
numpy float32 exp / sum / divide in fc2_softmax_kernel's order and the float64 softmax over these cases' logits
(1.03e-7, case taps_d2; the factor 4 is for the device's expf and the DPP sum order).

Which case sees which mistake (tests/test_cnn_mode_ref_cpu.py: MUTANTS, each shown to change the model's bits there):
  wlo_c1 .. wlo_d1   a dropped a_hi * w_lo term of that layer, or one read from the neighbouring tap (f16x2, f16q8), at
                     every kernel position of the convolution
  alo                a dropped a_lo * w_hi term of conv2, conv3, conv4 or dense 1, or one read from the neighbouring tap,
                     at every kernel position
  alo_sub            activation lo halves flushed where they are fp16 subnormals (f16x2)
  wlo_d1             dense 1's a_hi * w_lo term alone separates logits 3 and 5: dropped, the label falls to 3
  bf16_round         bf16 rounding by truncation; no rounding after conv1 or after conv3; a rounded bias; conv2's channel
                     31 and conv3's channel 89 sum to a real -0 (0x8000 into the relu's integer clamp): +0 bits are owed
  taps_c1 .. taps_c4 one tap shifted, the kernel not flipped (gather sees both too); taps_d1 / taps_d2: the dense layers
  gather             region origin 340 replaced by 320 or 339; the sixth tap of a conv1 kernel row given weight (also taps_c1)
  ties               argmax keeping the last maximum (15 = 16, 79 = 80, 0 = 80, four-way ties, an all-equal row -> 0)
  padding            a zero pad column of dense 2 given weight (in y); conv3 / conv4 channels 80 .. 89 next to the pads

bf16 at realistic magnitudes.  Seeded and trained weights, one scene and one noise goban, 34 of the 100 regions each,
staged so that one flipped rounding does not propagate: A goban -> pool2; B the model's conv3 + conv4 + pool on the
GPU's pool2; C the model's dense layers on the GPU's pool4.  Yardstick: the model against itself, float32 against
float64 accumulation of the same roundings (measured by test_bf16_model_against_itself_at_realistic_magnitudes):
  (a) at most 2 % of a stage's elements differ from the float64 model at all (the model alone: 0.05 % staged, 0.42 % chained);
  (b) every one that differs is within one bf16 ulp of the model's value or within ec.A_REAL = 4 x 3.14e-4 = 1.26e-3 of
      the map's largest value (3.14e-4: the largest excess of the float32 model, pool4, seeded weights, noise goban);
  (C) y within ec.Y_REAL = 4 x 1.67e-7 = 6.7e-7 (1.67e-7: the float32 against the float64 dense layers of the model)."""
import numpy as np
import pytest

from tests import cnn_exact_cases as ec
from tests import cnn_mode_ref as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _mode(name):
    from camkifu_amd import capi
    return {"f16x2": capi.CK_CNN_F16X2, "fp32": capi.CK_CNN_FP32, "bf16": capi.CK_CNN_BF16, "f16q8": capi.CK_CNN_F16Q8}[name]


_refs = {}


def _reference(name, mode):
    """the model's answer for (case, mode), computed once per case where the models of all its modes agree (asserted
    on the CPU), left unchanged"""
    c = ec.case(name)
    key = (name, c["modes"][0] if c["agree"] else mode)
    if key not in _refs:
        o = mr.forward(c["W"], c["gobans"], key[1])
        lab, _, stones, _ = mr.decode(o["y"])
        assert np.array_equal(lab, o["logits"].argmax(-1))
        _refs[key] = dict(o, labels=lab, stones=stones)
        for v in _refs[key].values():
            v.setflags(write=False)
    return _refs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _all(ck, gobans):
    p2, p4 = ck.cnn_maps(gobans)
    y, stones, conf = ck.cnn_predict(gobans)
    rl, rc = ck.cnn_regions(gobans)
    return dict(pool2=p2, pool4=p4, y=y, stones=stones, conf=conf, rl=rl.reshape(len(gobans), 100), rc=rc.reshape(len(gobans), 100))


@pytest.mark.parametrize("name, mode", ec.pairs())
def test_exact_case_bit_for_bit(ck, name, mode):
    """ck_cnn_maps refuses a batch that raised the overflow flag, so its clean return on the very batch cnn_predict and
    cnn_regions then classify shows that the mode's own kernels ran and not the f32 fallback of cnn_run."""
    from camkifu_amd import capi
    c, ref = ec.case(name), _reference(name, mode)
    g = c["gobans"]
    ck.cnn_set_weights(c["W"])
    ck.cnn_set_mode(_mode(mode))
    try:
        one = _all(ck, g)
        three = _all(ck, np.stack([g[0], ec.noise(), g[0]]))
    finally:
        ck.cnn_set_mode(capi.CK_CNN_DEFAULT)
    for k in ("pool2", "pool4"):
        want = _bits(ref[k])
        bad = one[k].view(np.uint32) != want
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            pytest.fail("%s %s %s: %d of %d elements differ, first at %r: got %r, want %r" % (
                name, mode, k, bad.sum(), bad.size, i, float(one[k][i]), float(ref[k][i])))
    assert np.array_equal(one["rl"], ref["labels"]), (name, mode)
    assert np.array_equal(one["stones"], ref["stones"])
    lab, conf, _, conf19 = mr.decode(one["y"])                      # from the GPU's own y: float64, index order
    assert np.array_equal(lab, one["rl"])
    assert np.array_equal(one["rc"].view(np.uint64), conf.view(np.uint64))
    assert np.array_equal(one["conf"].view(np.uint64), np.ascontiguousarray(conf19).view(np.uint64))
    gap = float(np.abs(one["y"] - ref["y"]).max())
    print("%s %s: |y - y64| max %.3g (bound %.3g)" % (name, mode, gap, ec.Y_EXACT))
    assert gap <= ec.Y_EXACT, (name, mode, gap)
    for k, v in one.items():                                           # (case, noise, case): both copies are the single run
        for copy in (0, 2):
            assert np.array_equal(three[k][copy].view(np.uint8), v[0].view(np.uint8)), (name, mode, k, copy)


@pytest.mark.parametrize("wname", ["random", "trained"])
def test_bf16_against_its_rounding_model_at_realistic_magnitudes(ck, ora, wname):
    from camkifu_amd import capi, synth
    g = ec.realistic_gobans(ora, synth)
    W = dict(ec.realistic_weights(synth))[wname]
    ck.cnn_set_weights(W)
    ck.cnn_set_mode(capi.CK_CNN_BF16)
    try:
        p2, p4 = ck.cnn_maps(g)
        y, _, _ = ck.cnn_predict(g)
    finally:
        ck.cnn_set_mode(capi.CK_CNN_DEFAULT)
        ck.cnn_set_weights(synth.cnn_weights())
    R = list(ec.REAL_REGIONS)
    for k in range(2):
        x = mr.gather(g[k])[R]
        stages = (("A", p2[k][R], mr.stage_a(W, None, "bf16", patches=x)),
                  ("B", p4[k][R], mr.stage_b(W, p2[k][R], "bf16")))
        for s, got, want in stages:
            share, excess = mr.compare_maps(got, want.reshape(got.shape))
            print("%s %s stage %s: %.4f %% differ, excess %.3g (bound %.3g)" % (wname, ("scene", "noise")[k], s, 100 * share, excess, ec.A_REAL))
            assert float(np.abs(want).max()) > 0.1
            assert share <= ec.SHARE and excess <= ec.A_REAL, (wname, k, s, share, excess)
        gap = float(np.abs(y[k][R] - mr.stage_c(W, p4[k][R], "bf16")[2]).max())
        print("%s %s stage C: |y - model| max %.3g (bound %.3g)" % (wname, ("scene", "noise")[k], gap, ec.Y_REAL))
        assert gap <= ec.Y_REAL, (wname, k, gap)

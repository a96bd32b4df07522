"""Networks and goban images on which the stone classifier's arithmetic is exact, for tests/test_cnn_mode_ref_cpu.py and
tests/test_gpu_cnn_exact.py: every operand survives the rounding its mode applies and every sum is short enough for f32
accumulation in any order (tests/cnn_mode_ref.py: audit), so the float64 result is the one right answer and a kernel
has to return its bits.

A case is a dict: name, W (the twelve float32 arrays), gobans (n, 380, 380, 3) uint8, modes (the CK_CNN_* modes whose
audit it passes) and agree (the models of all its modes give the same bits; False where bf16's roundings are the
point).  Most cases start from one "chain" of single-tap layers that hands pixel values through the network --
  conv1  channel o reads pixel channel o % 3 at a tap that depends on o
  conv2  channel o reads conv1's channel o            conv3  channel o reads pool2's channel o % 32
  conv4  channel o reads conv3's channel o            dense 1  unit k reads one pool4 element, dense 2 adds units c, c + 81
-- and replace the layer they are about."""
import numpy as np

from camkifu_amd.capi import WEIGHT_SHAPES

ALL = ("fp32", "f16x2", "f16q8", "bf16")
SPLIT = ("fp32", "f16x2", "f16q8")


def _tap(o, kh, kw, salt=0):
    """the kernel position output channel o reads in a single-tap layer: the channels walk through ALL kh * kw positions
    (32 channels over conv1's and conv2's 25, 90 over conv3's and conv4's 9); `salt` sets two layers apart"""
    t = (o + 7 * salt) % (kh * kw)
    return t // kw, t % kw


def chain(scale1=1.0):
    W = {k: np.zeros(s, np.float32) for k, s in WEIGHT_SHAPES.items()}
    for o in range(32):
        i, j = _tap(o, 5, 5)
        W["c1w"][i, j, o % 3, o] = scale1
        i, j = _tap(o, 5, 5, 1)
        W["c2w"][i, j, o, o] = 1
    for o in range(90):
        i, j = _tap(o, 3, 3)
        W["c3w"][i, j, o % 32, o] = 1
        i, j = _tap(o, 3, 3, 1)
        W["c4w"][i, j, o, o] = 1
    for k in range(160):
        W["d1w"][(k * 20 + 7) % 3240, k] = 1
        W["d2w"][k, k % 81] = 2.0 ** -6
    return W


def _pm12(rng, shape):
    return (rng.choice([-2.0, -1.0, 1.0, 2.0], size=shape)).astype(np.float32)


def _bits(rng, p):
    """a goban image whose pixels are 1 with probability p, else 0"""
    return (rng.random((1, 380, 380, 3)) < p).astype(np.uint8)


def _case(name, W, gobans, modes=ALL, agree=True):
    return dict(name=name, W=W, gobans=np.ascontiguousarray(gobans, np.uint8), modes=tuple(modes), agree=agree)


# ---- taps: every weight of one layer alive, small integers, different in every output channel -----------------------
def taps_c1():
    rng = np.random.default_rng(101)
    W = chain()
    W["c1w"] = _pm12(rng, WEIGHT_SHAPES["c1w"])
    W["c1b"][:] = 64                              # |sum| <= 75 * 2: the maps stay within 0 .. 214
    return _case("taps_c1", W, _bits(rng, 0.5))


def taps_c2():
    rng = np.random.default_rng(102)
    W = chain()
    W["c2w"] = _pm12(rng, WEIGHT_SHAPES["c2w"])
    return _case("taps_c2", W, _bits(rng, 0.25))


def taps_c3():
    rng = np.random.default_rng(103)
    W = chain()
    W["c3w"] = _pm12(rng, WEIGHT_SHAPES["c3w"])
    W["c3b"] = rng.integers(-3, 4, 90).astype(np.float32)
    return _case("taps_c3", W, _bits(rng, 0.1))


def taps_c4():
    rng = np.random.default_rng(104)
    W = chain()
    W["c4w"] = _pm12(rng, WEIGHT_SHAPES["c4w"])
    W["c4b"] = rng.integers(-3, 4, 90).astype(np.float32)
    return _case("taps_c4", W, _bits(rng, 0.1))


def taps_d1():
    rng = np.random.default_rng(105)
    W = chain()
    W["d1w"] = _pm12(rng, WEIGHT_SHAPES["d1w"])
    W["d1b"] = rng.integers(-3, 4, 160).astype(np.float32)
    return _case("taps_d1", W, _bits(rng, 0.03))


def taps_d2():
    rng = np.random.default_rng(106)
    W = chain()
    W["d2w"] = _pm12(rng, WEIGHT_SHAPES["d2w"]) * np.float32(2.0 ** -6)
    W["d2b"] = (rng.integers(-8, 9, 81) * 2.0 ** -6).astype(np.float32)
    return _case("taps_d2", W, rng.integers(0, 16, (1, 380, 380, 3)))


# ---- gather: the pixel says where it is ----------------------------------------------------------------------------------
def gather():
    y, x = np.mgrid[:380, :380]
    g = np.stack([x // 2, y // 2, (x & 1) | ((y & 1) << 1) | (((x // 40 + 3 * (y // 40)) & 7) << 2)], -1)
    return _case("gather", chain(), g[None])


# ---- weight lo: one layer's weights carry 12 .. 14 significant bits, every activation that meets them has 4 -----------
_WLO = (1 + 2.0 ** -12, 0.5 + 2.0 ** -13, 2 + 2.0 ** -10)


def wlo(layer):
    rng = np.random.default_rng(110 + "c1 c2 c3 c4 d1".split().index(layer))
    W = chain()
    k = W[layer + "w"]
    nz = np.nonzero(k)
    k[nz] = np.asarray(_WLO, np.float32)[nz[-1] % 3]
    if layer == "d1":
        W["d2w"] *= np.float32(16)                # dense 1 shows in y alone: logits steep enough for 2^-12 of a unit to move it
        # ... and in a label: units 158 and 159 read the same pool4 element p, 158 with weight 1 (no lo), 159 with
        # 1 + 2^-12; they alone feed logits 3 and 5, twice as steeply as anything else.  Where p >= 8 the best logit is 5,
        # by p * 2^-11 = a_hi * w_lo alone: without that term 3 and 5 tie and the first maximum, 3, wins.
        e = int(np.nonzero(W["d1w"][:, 159])[0][0])
        W["d1w"][:, 158] = 0
        W["d1w"][e, 158] = 1
        W["d2w"][[3, 84, 5, 86, 158, 159]] = 0
        W["d2w"][158, 3] = W["d2w"][159, 5] = 2
    return _case("wlo_" + layer, W, rng.integers(0, 16, (1, 380, 380, 3)), SPLIT)


# ---- activation lo: conv1 builds 14-bit values, every later weight is a power of two ------------------------------------
def alo():
    rng = np.random.default_rng(120)
    W = chain()
    for o in range(32):
        i, j = _tap(o, 5, 5)
        W["c1w"][i, j, o % 3, o] = 4
        W["c1w"][(i + 2) % 5, (j + 1) % 5, (o + 1) % 3, o] = 2.0 ** -4
        i, j = _tap(o, 5, 5, 1)
        W["c2w"][i, j, o, o] = 0.5
        W["c2w"][(i + 1) % 5, (j + 3) % 5, (o + 5) % 32, o] = 0.25
    W["c4w"] *= np.float32(0.5)
    return _case("alo", W, rng.integers(0, 256, (1, 380, 380, 3)), SPLIT)


def alo_sub():
    """conv1's output is 2^-3 (1 + 2^-19) wherever the pixel is 1: hi = 2^-3 and lo = 2^-22, an fp16 SUBNORMAL (the
    weights are pre-scaled by 2^8, the activations are not)"""
    rng = np.random.default_rng(121)
    W = chain(2.0 ** -3 + 2.0 ** -22)
    W["d2w"][81:] = 0                             # one term per logit: its sum stays within 2^20 quanta of 2^-28
    return _case("alo_sub", W, _bits(rng, 0.3), ("fp32", "f16x2"))


# ---- bf16 rounding: ties on both sides, values just off a tie, -0, biases that are no bf16 numbers --------------------
def bf16_round():
    rng = np.random.default_rng(130)
    W = chain()
    nb = np.float32(1 + 2.0 ** -9)                # not a bf16 number
    for o in range(32):
        i, j = _tap(o, 5, 5)
        s = -1.0 if o % 4 == 3 else 1.0          # every fourth channel: negative sums, and -0 where the pixels are 0
        W["c1w"][i, j, o % 3, o] = s
        W["c1w"][(i + 1) % 5, (j + 2) % 5, (o + 1) % 3, o] = s
        W["c1w"][(i + 3) % 5, (j + 1) % 5, (o + 2) % 3, o] = s * 0.25
        W["c1b"][o] = (0.0, nb, 0.5, -0.0)[o % 4]
        i, j = _tap(o, 5, 5, 1)
        W["c2w"][(i + 2) % 5, (j + 2) % 5, (o + 4) % 32, o] = 0.5
        W["c2b"][o] = (nb, 0.0)[o % 2]
    for o in range(90):
        i, j = _tap(o, 3, 3)
        W["c3w"][(i + 1) % 3, (j + 1) % 3, (o + 8) % 32, o] = 1
        W["c3b"][o] = (0.0, nb, -nb)[o % 3]
        i, j = _tap(o, 3, 3, 1)
        W["c4w"][(i + 2) % 3, (j + 1) % 3, (o + 2) % 90, o] = 0.5
        W["c4b"][o] = (nb, 0.0, 0.25)[o % 3]
    # a real -0 before the relu.  k_cnn_bf16.hip starts every accumulator at the bias and conv2 (K = 25 x 32) and conv3
    # (K = 9 x 32) have no padding slot, and Bf16Rne keeps the sign of a -0.0 weight: an output channel whose weights are
    # ALL -0.0 or negative and whose bias is -0.0 sums nothing but -0 wherever its inputs are 0 -- over the blacked-out
    # rectangle below -- and that -0 goes through the pool's fmaxf into pk_bf16_relu's integer clamp as 0x8000.
    W["c2b"][4] = 0                               # pool2 channel 4: conv1's channels 4 and 8, zero over the rectangle
    W["c2w"][..., 31] = -0.0
    W["c2w"][1, 3, 0, 31], W["c2w"][4, 0, 8, 31], W["c2b"][31] = -1, -0.5, -0.0
    W["c3w"][..., 89] = -0.0
    W["c3w"][0, 2, 4, 89], W["c3w"][2, 1, 31, 89], W["c3b"][89] = -1, -0.5, -0.0
    g = rng.integers(0, 64, (1, 380, 380, 3))
    g[0, 100:180, 60:300] = 0
    return _case("bf16_round", W, g, ("bf16",), agree=False)


# ---- padding: the channels and columns next to the zero pads alive, the image 255 everywhere -------------------------
def padding():
    W = chain()
    W["c3b"][80:] = 0.5
    W["c4b"][80:] = 1
    W["c3w"][..., 80:] *= np.float32(0.5)
    W["d2b"][64:] = 2.0 ** -5
    return _case("padding", W, np.full((1, 380, 380, 3), 255))


# ---- ties: equal best logits at different index pairs, an all-equal row -----------------------------------------------
def ties():
    rng = np.random.default_rng(140)
    W = chain()
    W["d1w"][:] = 0
    W["d2w"][:] = 0
    for c in range(3):
        W["d1w"][c, c] = 1                        # unit c = pool4[0, 0, c] = the colour of the block the patch starts in
    for k, cols in ((0, (15, 16)), (1, (79, 80)), (2, (0, 80))):
        for c in cols:
            W["d2w"][k, c] = 0.25
    col = rng.choice([0, 2, 4, 8], size=(10, 10, 3))
    col[0, 0] = col[5, 5] = (0, 0, 0)             # every logit equal: label 0
    col[0, 1] = (4, 0, 0)                         # 15 = 16
    col[0, 2] = (0, 4, 0)                         # 79 = 80
    col[0, 3] = (0, 0, 4)                         # 0 = 80
    col[0, 4] = (4, 4, 0)                         # 15 = 16 = 79 = 80
    col[0, 5] = (4, 0, 4)                         # 0 = 15 = 16 = 80
    g = np.repeat(np.repeat(col, 40, 0), 40, 1)[:380, :380]
    return _case("ties", W, g[None])


_BUILDERS = [taps_c1, taps_c2, taps_c3, taps_c4, taps_d1, taps_d2, gather] + \
    [(lambda L=L: wlo(L)) for L in ("c1", "c2", "c3", "c4", "d1")] + [alo, alo_sub, bf16_round, padding, ties]
NAMES = ["taps_c1", "taps_c2", "taps_c3", "taps_c4", "taps_d1", "taps_d2", "gather", "wlo_c1", "wlo_c2", "wlo_c3", "wlo_c4",
         "wlo_d1", "alo", "alo_sub", "bf16_round", "padding", "ties"]
MODES_OF = dict(zip(NAMES, [ALL] * 7 + [SPLIT] * 5 + [SPLIT, ("fp32", "f16x2"), ("bf16",), ALL, ALL]))
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = _BUILDERS[NAMES.index(name)]()
        assert _cache[name]["name"] == name and _cache[name]["modes"] == tuple(MODES_OF[name])
    return _cache[name]


def pairs():
    """every (case name, mode) the GPU test runs"""
    return [(n, m) for n in NAMES for m in MODES_OF[n]]


def noise():
    return np.random.default_rng(7).integers(0, 4, (380, 380, 3), dtype=np.uint8)


# ---- bf16 at realistic magnitudes ------------------------------------------------------------------------------------------
REAL_REGIONS = tuple(range(0, 100, 3))            # 34 of a goban's 100 regions, 9, 39, 69, 90 .. 99 at origin 340 among them


def realistic_gobans(ora, synth):
    """one scene goban and one noise goban (those of test_cnn_filter_maps_below_the_softmax)"""
    sc = synth.scene(480, 640, seed=31, density=0.45)
    dst = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)
    goban = ora.warp_perspective(sc["frame"].numpy(), ora.get_perspective_transform(sc["corners"], dst))
    return np.stack([goban, np.random.default_rng(17).integers(0, 256, (380, 380, 3), dtype=np.uint8)])


def realistic_weights(synth):
    from camkifu_amd.stone.nn_manager import NNManager
    return (("random", synth.cnn_weights()), ("trained", NNManager.init_net()))


# The yardsticks of tests/test_gpu_cnn_exact.py, each 4 x what the float64 model shows against ITSELF on the CPU
# (tests/test_cnn_mode_ref_cpu.py measures them again and holds the model alone to half of each):
#   Y_EXACT   y of an exact case against the float64 softmax of the exact logits.  numpy float32 exp / sum / divide in
#             fc2_softmax_kernel's order against float64, the largest gap over all cases: 1.03e-7 (taps_d2)
#   A_REAL    bf16, realistic weights, staged: the largest excess of the float32-accumulating model over one bf16 ulp
#             of the float64-accumulating one, relative to the map's largest value: 3.14e-4 (random weights, noise
#             goban, pool4; pool2: 7.8e-5; trained weights: 0)
#   Y_REAL    the same models' dense layers fed with the same pool4: the largest gap in y, 1.67e-7
#   SHARE     at most 2 % of a stage's elements differ at all (the model alone, staged: 0.05 %; chained: 0.42 %)
Y_EXACT = 4 * 1.03e-7
A_REAL = 4 * 3.14e-4
Y_REAL = 4 * 1.67e-7
SHARE = 0.02

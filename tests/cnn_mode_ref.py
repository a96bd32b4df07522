"""The stone classifier (NNManager.create_net) evaluated in float64 with the operand roundings of each CK_CNN_* mode,
for tests/test_cnn_mode_ref_cpu.py and tests/test_gpu_cnn_exact.py.  Plain numpy: no code shared with oracle/ or with
the kernels.  Convolutions are true ("flipped") valid convolutions over HWIO weights, pools are 2x2, the flatten is
channels-last, the 100 patches of a 380x380 goban image start at 0, 40 .. 320 and 340 in both axes.

Where every rounding point was read (csrc = camkifu_amd/csrc):

fp32   no operand is rounded.  csrc/k_cnn.hip conv1_mfma16_kernel / conv_mfma16_f32_kernel / fc1_mfma16_kernel:
       f32 operands, v_mfma_f32_16x16x4_f32, bias added to the f32 sum, relu; the pool takes the maximum first
       ("max commutes with the bias add and relu").
f16x2  csrc/k_cnn.hip.  Weights: Split of csrc/ck_cnn_pack.cpp -- hi = the NEAREST fp16 of w * 2^8, lo = the nearest
       fp16 of (w * 2^8 - hi).  Activations: split_h2x2 -- hi = fp16 of x TOWARDS ZERO (v_cvt_pkrtz), lo = fp16 towards
       zero of the f32 residual x - hi.  conv1: the u8 pixels are exact fp16 and have no lo (conv_h2_body, FUSE1: two
       MFMAs per product).  Per product lo*hi + hi*lo + hi*hi (k_loop of conv_h2_body, fc1_h2_kernel), the accumulator
       starts at bias * 2^8 (convolutions) and is scaled by 2^-8 at the end; dense 1 adds its bias after the scaling.
       An activation above 65000 raises the overflow flag.
f16q8  csrc/k_cnn_q8.hip:1-23 and split4.  conv1 as in f16x2 (pack c1w_q8 = both Split planes).  conv2 .. conv4: the
       main term is fp16(x) to NEAREST times the weight's hi plane; the cross terms' operands are e4m3 under the block
       scale 4: e4m3(hi / 4) against e4m3(w_lo * 2^11 / 4) and e4m3((x - hi) * 2^11 / 4) against e4m3(w_hi / 4) (Cross
       of csrc/ck_cnn_pack.cpp), the 2^-11 in the blocks' scales.  Dense 1 is fc1_h2_kernel, i.e. f16x2's
       (k_cnn_predict: `h2` holds for both split modes).  An activation above 1700 raises the overflow flag; weights
       beyond +-7 (448 * 4 / 2^8) switch the whole mode to the f16x2 kernels (q8_ok).
bf16   csrc/k_cnn_bf16.hip.  conv1: fp16 weights (pack c1w_f16, F16 = nearest) times the exact u8 pixels on the fp16
       MFMA; conv2 .. conv4 and dense 1: bf16 weights (Bf16Rne / Bf16Cast: nearest even) times bf16 activations.  Every
       accumulator starts at the f32 bias (dense 1 adds it at the end), pk_bf16_relu / bf16_relu round the f32 sum --
       after the pool's maximum where there is one -- to bf16, nearest even, and clamp the packed bits at zero (so a
       -0 becomes +0).  Dense 1 leaves f32 (relu, no rounding).
all    dense 2, the softmax (fc2_softmax_kernel) and the decode (decode_kernel) are f32 / f64 in every mode: logits =
       f32 sum + bias, y = expf(v - max) / sum; label = the FIRST maximum of y, conf = y[label] / sum of y in double,
       index order.

The kernels accumulate in f32 and store f32 (bf16 in bf16 mode); the model accumulates in float64 and rounds only where
a mode rounds an OPERAND, so mode fp32 is the float64 network itself.  On an exact case (audit) every f32 sum is exact
and the two are the same numbers.

Observed on the MI355X (tests/test_gpu_cnn_exact.py holds the kernels to it):
  * the fp16, bf16 and block-scaled f8 MFMAs with f32 accumulation returned the exact sum on every case, the widest of
    which put 0.6 .. 0.9 x 2^20 quanta into one sum next to its smallest term: the audit's span limit stands at 2^20,
    nothing had to be narrowed;
  * an activation lo that is an fp16 SUBNORMAL (case alo_sub: 2^-22 beside hi = 2^-3) is kept by v_cvt_pkrtz_f16_f32 and
    multiplied exactly by the fp16 MFMA, so split_act flushes nothing ("flush_lo" is a mutant, not the model)."""
import numpy as np

from tests import cnn_pack_ref as pk

MODES = ("fp32", "f16x2", "f16q8", "bf16")
ORIGINS = (0, 40, 80, 120, 160, 200, 240, 280, 320, 340)
WS = 256.0                       # CK_CNN_WSCALE: the split packs hold w * 2^8
SPAN = 2.0 ** 20                 # audit: sum of |terms| below SPAN quanta
LIMIT = {"f16x2": 65000.0, "f16q8": 1700.0}


# ---- roundings (float64 in, float64 out) ------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def fp16_rne(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


def fp16_rtz(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        h = x.astype(np.float32).astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)


def bf16_rne(x):
    bits = pk.bf16(np.asarray(x, np.float64).astype(np.float32)).astype(np.uint32) << 16
    return bits.view(np.float32).astype(np.float64).reshape(np.shape(x))


def bf16_trunc(x):
    bits = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32) & np.uint32(0xFFFF0000)
    return bits.view(np.float32).astype(np.float64).reshape(np.shape(x))


def e4m3_round(x):
    """x rounded to the nearest OCP e4m3 value, ties to the even code, saturating at 448 -- what Cross of
    ck_cnn_pack.cpp and v_cvt_scalef32_pk_fp8 give (the CPU test holds this to tests/cnn_pack_ref.py: e4m3).  Three
    mantissa bits: the quantum is 2^(exponent - 3), 2^-9 at and below the smallest normal 2^-6."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                               # |x| = m 2^e, m in [0.5, 1)
    q = np.ldexp(1.0, np.maximum(e - 4, -9))
    return np.clip(np.round(x / q) * q, -448.0, 448.0)


def split_weight(w):
    """(hi, lo) of w * 2^8 as ck_cnn_pack.cpp's Split writes them"""
    hi, lo = pk.split(np.asarray(w, np.float32))
    return hi.astype(np.float64), lo.astype(np.float64)


def split_act(x, mut=()):
    """split_h2x2 of k_cnn.hip: both halves rounded towards zero"""
    hi = fp16_rtz(x)
    lo = fp16_rtz(f32(x - hi))
    if "flush_lo" in mut:
        lo = np.where(np.abs(lo) < 2.0 ** -14, 0.0, lo)
    return hi, lo


def split_act_q8(x):
    """split4 of k_cnn_q8.hip -> (hi, e4m3 image of hi, e4m3 image of the residual), as values"""
    hi = fp16_rne(x)
    lo = f32(x - hi)
    return hi, 4.0 * e4m3_round(hi / 4.0), e4m3_round(lo * 512.0) / 512.0


def cross_weight(w):
    """Cross of ck_cnn_pack.cpp -> (e4m3 image of w_lo, e4m3 image of w_hi), as values of w * 2^8"""
    hi, lo = split_weight(w)
    return e4m3_round(lo * 512.0) / 512.0, 4.0 * e4m3_round(hi / 4.0)


# ---- the layers ----------------------------------------------------------------------------------------------------------
def gather(gobans, origins=ORIGINS):
    g = np.asarray(gobans)
    if g.ndim == 3:
        g = g[None]
    return np.stack([g[n, a:a + 40, b:b + 40] for n in range(len(g)) for a in origins for b in origins]).astype(np.float64)


def conv(x, k, acc=np.float64, flip=True):
    """valid convolution of x (N, H, W, CI) with the Keras kernel k (KH, KW, CI, CO): out[y, x] = sum x[y + i, x + j] *
    k[KH - 1 - i, KW - 1 - j]; one matrix product per tap that has a weight, over the channels that have one, accumulated in `acc`"""
    kf = (k[::-1, ::-1] if flip else k).astype(acc)
    x = x.astype(acc)
    kh, kw = k.shape[:2]
    oh, ow = x.shape[1] - kh + 1, x.shape[2] - kw + 1
    out = np.zeros((x.shape[0], oh, ow, k.shape[3]), acc)
    if not x.any():                              # (a lo plane that is all zero)
        return out.astype(np.float64)
    for i in range(kh):
        for j in range(kw):
            ci, co = kf[i, j].any(axis=1), kf[i, j].any(axis=0)
            if ci.all() and co.all():
                out += x[:, i:i + oh, j:j + ow] @ kf[i, j]
            elif ci.any():                       # a sparse tap: only the channels that carry a weight
                out[..., co] += x[:, i:i + oh, j:j + ow][..., ci] @ kf[i, j][ci][:, co]
    return out.astype(np.float64)


def pool(x):
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))


def relu(x):
    return np.where(x > 0, x, 0.0)               # (-0 and negatives -> +0)


def _shift_tap(k):
    """one tap shifted: what kernel column 0 holds moves to column 1 and back"""
    k = k.copy()
    k[:, [0, 1]] = k[:, [1, 0]]
    return k


def _neighbour(k):
    """the weights as the neighbouring tap column would see them (a term read from the wrong tap)"""
    return np.roll(k, 1, axis=1)


def _terms(a, k, mode, layer, mut, first):
    """the operand pairs (activation part, weight part) whose products a mode sums for one layer, and the scale the
    sum is divided by; `first`: the layer reads u8 pixels (conv1)"""
    if mode == "fp32":
        return [(a, k)], 1.0
    if mode == "bf16":
        return [(a, fp16_rne(k) if first else bf16_rne(k))], 1.0
    whi, wlo = split_weight(k)
    if first:                                    # pixels are exact fp16: hi*hi + hi*lo
        pairs = [(a, whi), (a, wlo, "hilo")]
    elif mode == "f16x2" or layer == "d1":
        ahi, alo = split_act(a, mut)
        pairs = [(ahi, whi), (ahi, wlo, "hilo"), (alo, whi, "lohi")]
    else:
        ahi, qh, ql = split_act_q8(a)
        wloq, whiq = cross_weight(k)
        pairs = [(ahi, whi), (qh, wloq, "hilo"), (ql, whiq, "lohi")]
    out = []
    for p in pairs:
        name = p[2] if len(p) > 2 else "main"
        if "drop_%s_%s" % (name, layer) in mut:
            continue
        w = p[1]
        if "near_%s_%s" % (name, layer) in mut:
            w = _neighbour(w) if w.ndim == 4 else np.roll(w, 1, axis=0)
        out.append((p[0], w))
    return out, WS


def _layer(a, k, b, mode, layer, mut, acc, first=False):
    """one convolution or dense layer before its relu: the sum of the mode's terms plus the f32 bias"""
    if "shift_" + layer in mut:
        k = _shift_tap(k)
    flip = ("noflip_" + layer) not in mut
    pairs, scale = _terms(a, np.asarray(k, np.float64), mode, layer, mut, first)
    s = 0.0
    for x, w in pairs:
        s = s + (conv(x, w, acc, flip) if w.ndim == 4 else (x.astype(acc) @ w.astype(acc)).astype(np.float64))
    b = np.asarray(b, np.float64)
    s = s / scale + (bf16_rne(b) if "bf16_bias" in mut else b)
    if mode == "bf16" and layer in ("c2", "c3"):
        # The sign of a zero.  numpy's products start from +0, the kernel's accumulator starts at the bias and these two
        # layers have no padding slot (K = 25 x 32 and 9 x 32): where the bias is -0.0 and EVERY weight of the output
        # channel carries the sign bit (-0.0 included), every addend over non-negative activations is -0 or negative, and a
        # sum that comes out zero is -0.  Nowhere else can a -0 sum arise: conv1, conv4 and dense 1 have +0 padding
        # slots in their packs, the fp32 kernels start at +0 and add the bias last, and the lo plane of a split -0.0
        # weight is +0.
        k = np.asarray(k)
        minus = np.signbit(b) & (b == 0) & np.signbit(k).all(axis=(0, 1, 2))
        s = np.where(minus & (s == 0), -0.0, s)
    return s


def _store(x, mode, mut, layer):
    """what the next layer reads of a layer's sum: in bf16 mode its bf16 image (the relu is applied by the caller AFTER
    the rounding, as pk_bf16_relu does; the two commute for every value but -0)"""
    if mode != "bf16" or ("bf16_skip_" + layer) in mut:
        return x
    return bf16_trunc(x) if "bf16_trunc" in mut else bf16_rne(x)


def stage_a(W, gobans, mode, mut=(), acc=np.float64, keep=None, patches=None):
    """goban images (or `patches` (N, 40, 40, 3) gathered already) -> pool2 (patches, 16, 16, 32); `keep`: a dict that
    receives the patches and conv1's output"""
    moved = [int(m[8:]) for m in mut if m.startswith("origin9_")]
    org = ORIGINS[:9] + (moved[0],) if moved else ORIGINS
    x = gather(gobans, org) if patches is None else np.asarray(patches, np.float64)
    k1 = np.asarray(W["c1w"], np.float64)
    s = _layer(x, k1, W["c1b"], mode, "c1", mut, acc, first=True)
    if "pad_tap6" in mut:                        # the zero sixth tap of a conv1 kernel row given its neighbour's weight
        kf = k1[::-1, ::-1]
        xp = np.concatenate([x, x[:, :, -1:]], axis=2)
        for i in range(5):
            s = s + xp[:, i:i + 36, 5:41] @ kf[i, 4]
    a1 = relu(_store(s, mode, mut, "c1"))
    if keep is not None:
        keep.update(x=x, a1=a1)
    s = _layer(a1, W["c2w"], W["c2b"], mode, "c2", mut, acc)
    return relu(_store(pool(s), mode, mut, "c2"))


def stage_b(W, pool2, mode, mut=(), acc=np.float64, keep=None):
    """pool2 -> pool4 (patches, 6, 6, 90); `keep`: a dict that receives conv3's output"""
    s = _layer(np.asarray(pool2, np.float64), W["c3w"], W["c3b"], mode, "c3", mut, acc)
    a3 = relu(_store(s, mode, mut, "c3"))
    if keep is not None:
        keep.update(a3=a3)
    s = _layer(a3, W["c4w"], W["c4b"], mode, "c4", mut, acc)
    return relu(_store(pool(s), mode, mut, "c4"))


def softmax64(logits):
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softmax32_kernel_order(logits):
    """fc2_softmax_kernel's arithmetic in numpy float32: expf(v - max), a lane's six tiles summed in order, then the
    four DPP butterflies over the 16 lanes of a row (xor 1, xor 2, half mirror, mirror), the division"""
    v = np.full((len(logits), 96), -np.inf, np.float32)
    v[:, :81] = np.asarray(logits, np.float64).astype(np.float32)
    e = np.exp(v - v.max(axis=1, keepdims=True)).astype(np.float32)
    s = np.zeros((len(v), 16), np.float32)
    for t in range(6):
        s = s + e[:, 16 * t:16 * t + 16]
    lane = np.arange(16)
    for perm in (lane ^ 1, lane ^ 2, (lane & 8) | (7 - (lane & 7)), 15 - lane):
        s = s + s[:, perm]
    return (e / s[:, :1])[:, :81]


def stage_c(W, pool4, mode, mut=(), acc=np.float64):
    """pool4 -> (h1, logits, y)"""
    x = np.asarray(pool4, np.float64).reshape(len(pool4), -1)
    h1 = relu(_layer(x, np.asarray(W["d1w"], np.float64), W["d1b"], mode, "d1", mut, acc))
    d2 = np.asarray(W["d2w"], np.float64)
    logits = (h1.astype(acc) @ d2.astype(acc)).astype(np.float64) + np.asarray(W["d2b"], np.float64)
    if "pad_d2" in mut:                          # a zero pad column of dense 2 (81 .. 95) given column 80's weights
        lg = np.concatenate([logits, logits[:, 80:81]], axis=1)
        return h1, logits, softmax64(lg)[:, :81]
    return h1, logits, softmax64(logits)


def forward(W, gobans, mode, mut=(), acc=np.float64):
    """-> dict pool2 (n, 100, 16, 16, 32), pool4 (n, 100, 6, 6, 90), h1 (n, 100, 160), logits and y (n, 100, 81)"""
    assert mode in MODES
    n = 1 if np.ndim(gobans) == 3 else len(gobans)
    p2 = stage_a(W, gobans, mode, mut, acc)
    p4 = stage_b(W, p2, mode, mut, acc)
    h1, logits, y = stage_c(W, p4, mode, mut, acc)
    return dict(pool2=p2.reshape(n, 100, 16, 16, 32), pool4=p4.reshape(n, 100, 6, 6, 90), h1=h1.reshape(n, 100, 160),
                logits=logits.reshape(n, 100, 81), y=y.reshape(n, 100, 81))


def decode(y, last=False):
    """decode_kernel: y (n, 100, 81) -> region labels (n, 100), region conf (n, 100) float64, stones (n, 19, 19), conf
    (n, 19, 19).  The first maximum wins; conf = y[label] / sum of y in double, index order.  `last`: the mutant that
    keeps the last maximum."""
    y = np.asarray(y)
    lab = (80 - y[..., ::-1].argmax(-1)) if last else y.argmax(-1)
    s = np.zeros(y.shape[:-1], np.float64)
    for k in range(81):
        s = s + y[..., k].astype(np.float64)
    conf = np.take_along_axis(y, lab[..., None], -1)[..., 0].astype(np.float64) / s
    r = np.arange(19)
    reg = np.where(r >= 17, 9, r // 2)
    start = np.where(reg == 9, 17, 2 * reg)
    idx = reg[:, None] * 10 + reg[None, :]
    digit = (r - start)[:, None] * 2 + (r - start)[None, :]
    stones = (lab[:, idx] // 3 ** digit) % 3
    return lab.astype(np.uint8), conf, stones.astype(np.uint8), conf[:, idx]


# ---- the proof obligations of an exact case -----------------------------------------------------------------------------
def quantum(x):
    """the largest power of two that divides every nonzero element of x (inf for an all-zero array)"""
    x = np.abs(np.asarray(x, np.float64).ravel())
    x = x[x != 0]
    if not x.size:
        return np.inf
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)
    return float(np.min(np.ldexp((mi & -mi).astype(np.float64), e - 53)))


def _audit_layer(a, k, b, mode, layer, first):
    k = np.asarray(k, np.float64)
    b = np.asarray(b, np.float64)
    ok = {}
    if mode == "fp32":
        parts_a, parts_w = [a], [k]
        ok["operands"] = bool(np.array_equal(f32(a), a))
    elif mode == "bf16":
        kr = fp16_rne(k) if first else bf16_rne(k)
        parts_a, parts_w = [a], [k]
        ok["operands"] = bool(np.array_equal(kr, k) and (first or np.array_equal(bf16_rne(a), a)))
    else:
        whi, wlo = split_weight(k)
        q8 = mode == "f16q8" and layer in ("c2", "c3", "c4")
        if first:
            ahi, alo = a, np.zeros_like(a)
            fine = np.array_equal(fp16_rne(a), a)
        elif q8:
            ahi, qh, ql = split_act_q8(a)
            alo = a - ahi
            wloq, whiq = cross_weight(k)
            fine = np.array_equal(ql, alo) and np.array_equal(wloq, wlo)
            if wlo.any():
                fine = fine and np.array_equal(qh, ahi)           # e4m3(hi / 4) meets a weight lo: it has to be hi
            if alo.any():
                fine = fine and np.array_equal(whiq, whi)
        else:
            ahi, alo = split_act(a)
            fine = np.array_equal(ahi + alo, a)
        ok["operands"] = bool(fine and np.array_equal(whi + wlo, k * WS))
        ok["no_lo_lo"] = not (alo.any() and wlo.any())
        ok["range"] = bool(np.abs(a).max() < LIMIT[mode] and (mode != "f16q8" or np.abs(k).max() <= 7.0))
        parts_a, parts_w = [ahi, alo], [whi / WS, wlo / WS]
    q = min(min(quantum(p) for p in parts_a) * min(quantum(p) for p in parts_w), quantum(b))
    absum = (conv(np.abs(a), np.abs(k)) if k.ndim == 4 else np.abs(a) @ np.abs(k)) + np.abs(b)
    ok["span"] = bool(absum.max() < SPAN * q) if np.isfinite(q) else True
    ok["q"], ok["sum"] = q, float(absum.max())
    ok["ok"] = all(v for n, v in ok.items() if n in ("operands", "no_lo_lo", "range", "span"))
    return ok


def audit(W, gobans, mode, outputs=None):
    """Per layer, what makes "bit for bit" legitimate for (W, gobans) in `mode`:
      operands  every operand is unchanged by the mode's rounding of it (for f16q8's e4m3 images: wherever the term they
                enter has a nonzero partner in the layer);
      no_lo_lo  split modes: no layer has both a weight lo and an activation lo (the dropped lo*lo term is then zero);
      range     split modes: every activation below the overflow flag's limit (65000 / 1700), q8 weights within +-7;
      span      every term of every output sum, the bias included, is a multiple of one quantum q and the sum of the
                terms' magnitudes is below 2^20 q -- then f32 accumulation is exact in any order and with any
                internal alignment of the addends that keeps 24 bits below the largest.
    The activations are the float64 model's own (mode `mode`), so a bf16 case may round between layers: the rounding is
    then applied to an exact sum and is itself well defined.  `outputs`: a dict that receives the model's flat pool2, pool4,
    h1, logits and y of this run.  -> dict layer -> dict of the checks, "ok" their conjunction."""
    out, k = {}, {}
    p2 = stage_a(W, gobans, mode, keep=k)
    p4 = stage_b(W, p2, mode, keep=k)
    h1, logits, y = stage_c(W, p4, mode)
    out["c1"] = _audit_layer(k["x"], W["c1w"], W["c1b"], mode, "c1", True)
    out["c2"] = _audit_layer(k["a1"], W["c2w"], W["c2b"], mode, "c2", False)
    out["c3"] = _audit_layer(p2, W["c3w"], W["c3b"], mode, "c3", False)
    out["c4"] = _audit_layer(k["a3"], W["c4w"], W["c4b"], mode, "c4", False)
    out["d1"] = _audit_layer(p4.reshape(len(p4), -1), W["d1w"], W["d1b"], mode, "d1", False)
    out["d2"] = _audit_layer(h1, W["d2w"], W["d2b"], "fp32", "d2", False)
    if outputs is not None:
        outputs.update(pool2=p2, pool4=p4, h1=h1, logits=logits, y=y)
    return out


def audit_ok(W, gobans, mode):
    return all(v["ok"] for v in audit(W, gobans, mode).values())


# ---- bf16 at realistic magnitudes: how far two evaluations of the same roundings may lie apart -----------------------
def bf16_ulp(v):
    """the spacing of bf16 numbers at |v| (0 at 0)"""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)
    return np.where(v > 0, np.ldexp(1.0, e - 8), 0.0)


def compare_maps(got, want):
    """-> (share of elements that differ at all, the largest excess of |got - want| over one bf16 ulp of `want`,
    relative to max |want|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = np.abs(got - want)
    excess = np.maximum(d - bf16_ulp(want), 0.0).max() / np.abs(want).max()
    return float((d != 0).mean()), float(excess)

"""Deterministic scenes and rate schedules for K9 (MOG2), shared by the CPU and GPU tests (numpy only, no GPU).

Each scene is built to drive one rarely taken branch of the mixture update (tests/test_mog2_cpu.py holds every scene to
a floor on the oracle's event counters, so a scene that is made trivial fails loudly):

    cycle   flat colours in a cycle longer than the 5 mode slots     new modes, replacement at NMIX, bubbles; with a
                                                                     0.6 .. 0.95 segment: updates that prune every mode
    noise   zero-noise, +-3 and +-40 pixels                          varMin (zero noise), varMax (+-40)
    ghost   a colour held 12 frames, >= 30 quiet frames, then again  prune of a transient mode, its return
    hand    a constant-colour blob that leaves and comes back        prune, bubble, replacement
    tie     two colours, two modes of equal weight, rate 0            a match that bubbles up on an exact weight tie

A scene is a function (h, w, frames, seed) -> uint8 (len(frames), h, w, 3) of frame indices, so a long sequence can be
made in slices.  Pixels of the mixture never interact: `mosaic` deals the four scenes over the pixels of one image.

`reference` is a second, structurally different statement of the update (lists of modes that are re-sorted, instead
of in-place bubbling over fixed arrays), the one tests/test_oracle_properties.py holds the C oracle against.
"""
import numpy as np

NMIX = 5
PALETTE = np.array([(20, 20, 20), (235, 235, 235), (235, 20, 20), (20, 235, 20), (20, 20, 235),
                    (235, 235, 20), (20, 235, 235), (235, 20, 235), (128, 128, 128)], np.int16)
HAND = np.array((60, 90, 140), np.int16)         # the blob colour of tests/test_gpu_ordered.py::_clip


def _pixel_rng(seed, salt):
    return np.random.default_rng([int(seed), salt])


def _frame_rng(seed, salt, t):
    return np.random.default_rng([int(seed), salt, int(t)])


def _frames(frames):
    return np.atleast_1d(np.asarray(frames, np.int64))


def cycle(h, w, frames, seed=0, ncol=7, hold=3):
    """each pixel cycles through `ncol` (>= 6) flat, well separated colours, each held `hold` frames, from its own
    phase: more colours than mode slots, so modes are opened, the weakest replaced and the rest bubble up"""
    assert 6 <= ncol <= len(PALETTE)
    rng = _pixel_rng(seed, 1)
    phase = rng.integers(0, ncol * hold, (h, w))
    offset = rng.integers(-8, 9, (h, w, 3)).astype(np.int16)
    out = np.empty((len(_frames(frames)), h, w, 3), np.uint8)
    for i, t in enumerate(_frames(frames)):
        out[i] = np.clip(PALETTE[((t + phase) // hold) % ncol] + offset, 0, 255)
    return out


def noise(h, w, frames, seed=0):
    """a fixed colour per pixel with uniform sensor noise of amplitude 0 (varMin), 3, or 40 (varMax) by pixel"""
    rng = _pixel_rng(seed, 2)
    base = rng.integers(60, 196, (h, w, 3)).astype(np.int16)
    yy, xx = np.mgrid[:h, :w]
    amp = np.array([0, 3, 40], np.int16)[(xx + 2 * yy) % 3][..., None]
    out = np.empty((len(_frames(frames)), h, w, 3), np.uint8)
    for i, t in enumerate(_frames(frames)):
        r = _frame_rng(seed, 2, t).integers(-40, 41, (h, w, 3)).astype(np.int16)
        out[i] = np.clip(base + np.clip(r, -amp, amp), 0, 255)
    return out


def ghost(h, w, frames, seed=0, start=8, hold=12, gap=32):
    """a quiet background; from frame start (+0..2 by pixel) a transient colour held `hold` frames, `gap` quiet frames,
    then the same colour again for `hold` frames (a mode that was pruned in the gap -- at a rate high enough to prune
    it -- comes back: the "ghost mode" case)"""
    rng = _pixel_rng(seed, 3)
    base = rng.integers(40, 110, (h, w, 3)).astype(np.int16)
    trans = 255 - base
    shift = rng.integers(0, 3, (h, w))
    out = np.empty((len(_frames(frames)), h, w, 3), np.uint8)
    for i, t in enumerate(_frames(frames)):
        s = t - start - shift
        on = ((s >= 0) & (s < hold)) | ((s >= hold + gap) & (s < 2 * hold + gap))
        out[i] = np.where(on[..., None], trans, base).astype(np.uint8)
    return out


def hand(h, w, frames, seed=0, period=25):
    """a textured, slightly noisy table and a constant-colour blob (a hand) over a third of the image that is there for
    8 frames of every `period`, moving while it is, then leaves and comes back (as _clip of test_gpu_ordered does)"""
    rng = _pixel_rng(seed, 4)
    base = rng.integers(30, 220, (h, w, 3)).astype(np.int16)
    bh, bw = max(1, (h + 2) // 3), max(1, (w + 2) // 3)
    out = np.empty((len(_frames(frames)), h, w, 3), np.uint8)
    for i, t in enumerate(_frames(frames)):
        fr = base + _frame_rng(seed, 4, t).integers(-2, 3, (h, w, 3)).astype(np.int16)
        p = int(t) % period
        if 10 <= p < 18:
            y0 = (h - bh) * (p - 10) // 7
            x0 = (w - bw) * (p - 10) // 14
            fr[y0:y0 + bh, x0:x0 + bw] = HAND
        out[i] = np.clip(fr, 0, 255)
    return out


def tie(h, w, frames, seed=0):
    """two colours per pixel: A on frame 0, B on frame 1, then A and B alternating (from a phase by pixel).  With the
    `tie` schedule (the automatic rate 0.5 on frame 0, 0.5 on frame 1) both modes hold exactly 0.5; at rate 0 a match
    changes no weight, so every match at mode 1 is an exact tie with mode 0 -- and a tie bubbles up
    (`!(weight < gw[i-1])`), which random scenes never reach"""
    rng = _pixel_rng(seed, 5)
    a = rng.integers(20, 100, (h, w, 3)).astype(np.uint8)
    b = (255 - a).astype(np.uint8)
    phase = rng.integers(0, 2, (h, w))
    out = np.empty((len(_frames(frames)), h, w, 3), np.uint8)
    for i, t in enumerate(_frames(frames)):
        use_b = np.full((h, w), t == 1) if t < 2 else (t + phase) % 2 == 1
        out[i] = np.where(use_b[..., None], b, a)
    return out


SCENES = dict(cycle=cycle, noise=noise, ghost=ghost, hand=hand)


def mosaic(h, w, frames, seed=0):
    """the four scenes dealt over the pixels in 4x4 tiles (a 1x1 image is all `cycle`)"""
    yy, xx = np.mgrid[:h, :w]
    kind = (yy // 4 + xx // 4) % len(SCENES)
    out = np.empty((len(_frames(frames)), h, w, 3), np.uint8)
    for k, fn in enumerate(SCENES.values()):
        sel = kind == k
        if sel.any():
            out[:, sel] = fn(h, w, frames, seed)[:, sel]
    return out


# ---------------------------------------------------------------- learning-rate schedules
def rates(name, n):
    """float64 (n,) learning rates.  `-1` is the library's automatic rate 1 / min(2 * nframes, 500) (capped from frame
    250 on); 0 opens no mode; >= 1 resets the model (the frame form only: an ordered run refuses it)."""
    r = np.full(n, 0.01)
    if name == "auto":                                   # the automatic rate through its cap
        r[:] = -1
    elif name == "product":                              # what the product uses (stonesfinder.py: 0.01, then 0.005)
        r[n // 2:] = 0.005
    elif name == "zero":                                 # spans of exact 0 between spans of 0.01
        r[n // 4:n // 4 + 10] = 0
        r[n // 2:n // 2 + 5] = 0
        r[-3:] = 0
    elif name == "reset":                                # one reset in the middle, then the automatic rate for a while
        r[n // 2] = 1.0
        r[n // 2 + 1:n // 2 + 11] = -1
    elif name == "high":                                 # after saturation, a segment at 0.6 .. 0.95 (its first frame
        k = max(n // 2, n - 20)                          # prunes every mode of a saturated pixel it does not match)
        r[k:k + 6] = (0.95, 0.6, 0.7, 0.95, 0.8, 0.67)[:len(r[k:k + 6])]
    elif name == "tie":                                  # two modes of exactly 0.5, then rate 0 (see `tie`), then 0.01
        r[0], r[1] = -1, 0.5
        r[2:n - 10] = 0
    elif name == "mixed":                                # all of the above in one sequence of >= 100 frames
        assert n >= 100
        r[40:50] = 0.005
        r[50:56] = 0
        r[56:60] = (0.95, 0.6, 0.8, 0.7)
        r[70] = 1.0
        r[71:100] = -1
        r[100:] = 0.005
    else:
        raise KeyError(name)
    return r


SCHEDULES = ("auto", "product", "zero", "reset", "high", "mixed")


# ---------------------------------------------------------------- state comparison
def zone_counts(mask):
    """ora.zone_counts as one block sum (20 x 20 zones, pixel row and column 379 not counted): the oracle's loop over
    the 361 zones costs ~0.1 s a frame.  tests/test_gpu_mog2.py::test_band_run_lengths_against_the_oracle checks the
    two agree."""
    m = (np.asarray(mask) != 0).astype(np.int32)
    m[379, :] = 0
    m[:, 379] = 0
    return m.reshape(19, 20, 19, 20).sum((1, 3), dtype=np.int32)


def state_mismatch(a, b):
    """None if two mixtures (Context.mog2_state / oracle MOG2.state layout) agree -- nmodes equal, and for every slot
    k < nmodes the weight, variance and mean bit-equal, NaN counting equal to NaN of any payload; slots at or above
    nmodes are don't-care -- else a short description of the first difference"""
    if not np.array_equal(a["nmodes"], b["nmodes"]):
        px = int(np.flatnonzero(a["nmodes"] != b["nmodes"])[0])
        return "nmodes differ at px %d: %d vs %d" % (px, a["nmodes"][px], b["nmodes"][px])
    live = np.arange(NMIX)[:, None] < a["nmodes"][None, :].astype(np.int64)          # (5, npx)
    for key in ("weight", "variance", "mean"):
        x, y = np.asarray(a[key], np.float32), np.asarray(b[key], np.float32)
        same = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        bad = ~same & (live[:, None, :] if x.ndim == 3 else live)
        if bad.any():
            idx = tuple(int(i[0]) for i in np.nonzero(bad))
            return "%s differs at %s: %r vs %r" % (key, idx, x[idx], y[idx])
    return None


def live_values(s):
    """the weights, variances and means of the live slots only (flat float32)"""
    live = np.arange(NMIX)[:, None] < s["nmodes"][None, :].astype(np.int64)
    return np.concatenate([s["weight"][live], s["variance"][live], s["mean"].transpose(1, 0, 2)[:, live].ravel()])


# ---------------------------------------------------------------- the second restatement
def reference(frames, rates_, return_state=False):
    """Zivkovic's adaptive mixture written out pixel by pixel in numpy float32 scalars (library defaults: 5 modes, Tb 16,
    Tg 9, TB 0.9, initial variance 15 clipped to [4, 75], complexity reduction 0.05, no shadows) -- a second, structurally
    different statement of K9 (lists of modes that are re-sorted, instead of in-place bubbling over fixed arrays).
    A rate >= 1 resets the model; an update that prunes every live mode skips the renormalisation.
    -> list of masks (and, with return_state, the final mixture in the MOG2.state layout)"""
    f32 = np.float32
    h, w = frames[0].shape[:2]
    modes = [[[] for _ in range(w)] for _ in range(h)]           # each mode: [weight, variance, mean(3)]
    masks = []
    nframes = 0
    for img, rate in zip(frames, rates_):
        if rate >= 1:
            modes = [[[] for _ in range(w)] for _ in range(h)]
            nframes = 0
        nframes += 1
        lr = rate if (rate >= 0 and nframes > 1) else 1.0 / min(2 * nframes, 500)
        alpha = f32(lr)
        one_minus = f32(1.0) - alpha
        prune = f32(-lr * f32(0.05))
        mask = np.zeros((h, w), np.uint8)
        for y in range(h):
            for x in range(w):
                px = img[y, x].astype(np.float32)
                ms = modes[y][x]
                background, fits, total = False, False, f32(0)
                k = 0
                while k < len(ms):
                    wgt = one_minus * ms[k][0] + prune
                    moved_to = k
                    if not fits:
                        var = ms[k][1]
                        d = ms[k][2] - px
                        dist2 = f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                        if total < f32(0.9) and dist2 < f32(16) * var:
                            background = True
                        if dist2 < f32(9) * var:
                            fits = True
                            wgt = wgt + alpha
                            kk = alpha / wgt
                            ms[k][2] = ms[k][2] - kk * d
                            nv = var + kk * (dist2 - var)
                            ms[k][1] = min(max(nv, f32(4)), f32(75))
                            while moved_to > 0 and not (wgt < ms[moved_to - 1][0]):     # keep the modes sorted by weight
                                ms[moved_to], ms[moved_to - 1] = ms[moved_to - 1], ms[moved_to]
                                moved_to -= 1
                    if wgt < -prune:
                        wgt = f32(0)
                        ms[moved_to][0] = wgt
                        ms.pop()                                   # sorted: the mode that falls away is the last one
                        if moved_to >= len(ms):
                            continue
                    else:
                        ms[moved_to][0] = wgt
                    total = total + wgt
                    k += 1
                if total != 0:                                     # all pruned: no renormalisation (no 0 * inf)
                    inv = f32(1) / total
                    for m in ms:
                        m[0] = m[0] * inv
                if not fits and alpha > 0:
                    if len(ms) == NMIX:
                        ms.pop()
                    if not ms:
                        ms.append([f32(1), f32(15), px.copy()])
                    else:
                        for m in ms:
                            m[0] = m[0] * one_minus
                        ms.append([alpha, f32(15), px.copy()])
                        j = len(ms) - 1
                        while j > 0 and not (alpha < ms[j - 1][0]):
                            ms[j], ms[j - 1] = ms[j - 1], ms[j]
                            j -= 1
                mask[y, x] = 0 if background else 255
        masks.append(mask)
    if not return_state:
        return masks
    npx = h * w
    st = dict(weight=np.zeros((NMIX, npx), np.float32), variance=np.zeros((NMIX, npx), np.float32),
              mean=np.zeros((NMIX, 3, npx), np.float32), nmodes=np.zeros(npx, np.uint8))
    for y in range(h):
        for x in range(w):
            p = y * w + x
            st["nmodes"][p] = len(modes[y][x])
            for k, (wt, var, mu) in enumerate(modes[y][x]):
                st["weight"][k, p], st["variance"][k, p], st["mean"][k, :, p] = wt, var, mu
    return masks, st

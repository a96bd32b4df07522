"""Inputs of the training tests: 40 x 40 patches cut from boards that synth.render draws straight into the canonical
380 x 380 frame (densities 0.1 - 0.6, noise 3), labelled with the base-3 code of their 2 x 2 intersections, and the seeded
He-normal weights of synth.cnn_weights() -- what NNManager.create_net returns and what training starts from.

Batches (cases()):
    n1, n3      the smallest; nothing is near a ReLU or pool decision in float32
    n65         one past a 64-wide tile (and past two 32-row MFMA tiles of the dense layers)
    n257        one past CHUNK = 256, the number of patches the trainer takes through forward and backward at once:
                the second chunk holds ONE patch and its gradient sums are added onto the first chunk's
    empty       label 0 only: patches of an empty board (wood and lines) and two of flat wood (one colour, no noise), in
                which all four values of every pool window are equal and mostly above 0: where the tie rule shows
    white       labels include 80 (four white stones), the last class
    ties        the patches of n3 under weights_of("ties"): eight filters of conv 2 and sixteen of conv 4 are zero with a
                positive bias, so their maps are constant above 0 and all four values of every pool window tie while the
                layer's input varies.  Under the seeded weights a tie happens at 0 only (behind ReLU), where relu'(0) = 0
                routes nothing whichever maximum is chosen -- and in flat patches, where the input does not vary and the
                choice changes no sum: the pool's tie rule is invisible on the other cases.
Everything is computed once per process and must be left unchanged by its users."""
import functools

import numpy as np

CHUNK = 256
ORIGIN = (0, 40, 80, 120, 160, 200, 240, 280, 320, 340)
START = (0, 2, 4, 6, 8, 10, 12, 14, 16, 17)
SQUARE = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)


def board(seed, density, stones=None):
    """-> (100 patches uint8 (100, 40, 40, 3), 100 labels uint8, the 380 x 380 image)"""
    from camkifu_amd import synth
    rng = np.random.default_rng(seed)
    if stones is None:
        stones = synth.random_stones(rng, density=density, keep_first_line_empty=False)
    img = synth.render(380, 380, stones, SQUARE, seed=seed, noise=3.0).numpy()
    X, Y = [], []
    for i in range(10):
        for j in range(10):
            X.append(img[ORIGIN[i]:ORIGIN[i] + 40, ORIGIN[j]:ORIGIN[j] + 40])
            s = stones[START[i]:START[i] + 2, START[j]:START[j] + 2].reshape(-1).astype(int)
            Y.append(s[0] + 3 * s[1] + 9 * s[2] + 27 * s[3])
    return np.stack(X), np.array(Y, np.uint8), img


@functools.lru_cache(maxsize=None)
def pool():
    """300 patches of three boards at densities 0.1, 0.35, 0.6"""
    parts = [board(900 + k, d) for k, d in enumerate((0.1, 0.35, 0.6))]
    X, Y = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def weights():
    from camkifu_amd import synth
    W = synth.cnn_weights()
    for a in W.values():
        a.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def weights_of(name):
    """the weights a case is run with: the seeded set, except for "ties" """
    if name != "ties":
        return weights()
    W = {k: v.copy() for k, v in weights().items()}
    W["c2w"][..., :8], W["c2b"][:8] = 0, np.linspace(0.05, 0.4, 8, dtype=np.float32)
    W["c4w"][..., :16], W["c4b"][:16] = 0, np.linspace(0.05, 0.8, 16, dtype=np.float32)
    for a in W.values():
        a.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def cases():
    """-> dict name -> (x uint8 (n, 40, 40, 3), labels uint8 (n,))"""
    X, Y = pool()
    pick = np.random.default_rng(77).permutation(len(X))
    out = {"n1": (X[pick[:1]], Y[pick[:1]]), "n3": (X[pick[1:4]], Y[pick[1:4]]), "n65": (X[pick[4:69]], Y[pick[4:69]]),
           "n%d" % (CHUNK + 1): (X[pick[:CHUNK + 1]], Y[pick[:CHUNK + 1]])}
    ex, ey, _ = board(950, 0.0, stones=np.zeros((19, 19), np.uint8))
    flat = np.empty((2, 40, 40, 3), np.uint8)          # flat wood, no noise: every 2 x 2 window of every map ties, above 0 too
    flat[0], flat[1] = (65, 100, 128), (60, 95, 121)
    out["empty"] = (np.concatenate([ex[[0, 37, 55, 99]], flat]), np.zeros(6, np.uint8))
    st = np.zeros((19, 19), np.uint8)
    st[4:6, 6:8] = 2                        # region (2, 3): four white stones = label 80
    st[10, 10], st[17, 18] = 1, 2
    wx, wy, _ = board(960, 0.0, stones=st)
    out["white"] = (wx[[23, 55, 99, 0]], wy[[23, 55, 99, 0]])
    out["ties"] = out["n3"]
    assert out["white"][1][0] == 80 and set(out["empty"][1]) == {0}
    for x, y in out.values():
        x.setflags(write=False)
        y.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 (loss, gradients) of case `name`, dropout off"""
    from tests import train_ref
    x, y = cases()[name]
    return train_ref.loss_and_grads(weights_of(name), x, y)


def learn_set():
    """32 patches of one board, 24 non-empty and 8 empty, for the 'it learns' test"""
    X, Y, _ = board(970, 0.3)
    full, empty = np.flatnonzero(Y > 0)[:24], np.flatnonzero(Y == 0)[:8]
    assert len(full) == 24 and len(empty) == 8
    idx = np.concatenate([full, empty])
    return X[idx], Y[idx]

"""NNManager: region geometry, the base-3 label codec, the classifier's weights and their training -- the reference's
stone/nn_manager.py (29-131, 133-214, 216-298, 360-382) under the same method names, built on small lookup
tables instead of per-call loops.  The Keras model is a dictionary of twelve float32 arrays handed to the HIP
library (K10..K12, ck_cnn_set_weights); train() fits them on the GPU (ck_train_*: forward, backward and Adam in
csrc/k_cnn_train.hip) and writes checkpoints as .npz files of those twelve arrays.  The labelling GUI is out of scope.

Tables (gsize 19, 10 x 10 regions of 2 x 2 intersections, the last region pulled back onto rows 17-18):
    REGION_START[i]  first row (or column) of region i            0, 2, ..., 16, 17
    DIGITS[label]    the four base-3 digits of a label, least significant first = intersections
                     (0,0) (0,1) (1,0) (1,1) of the region         nn_manager.py:236-254
    PATCH_ORIGIN[i]  first pixel of region i's 40-pixel window     0, 40, ..., 320, 340
    AUG_LABEL[t, l]  the label of a region labelled l after transform t of its window: numpy.rot90 by t & 3 quarter
                     turns, then the columns mirrored when t & 4 (Context.augment_patches does the same to the pixels)
"""
import os
import re
from threading import RLock

import numpy as np

from .. import cvconf
from ..golib_shim import gsize, E, B, W

SPLIT = 10
STEP = (gsize + 1) // SPLIT
NB_CLASSES = 3 ** (STEP * STEP)
REGION_START = np.minimum(np.arange(SPLIT) * STEP, gsize - STEP)
DIGITS = ((np.arange(NB_CLASSES)[:, None] // 3 ** np.arange(STEP * STEP)[None, :]) % 3).astype(np.uint8)
SYMBOLS = np.array([E, B, W], dtype=object)
CODE = {E: 0, B: 1, W: 2}
CELL_PX = cvconf.canonical_size // gsize
PATCH_ORIGIN = REGION_START * CELL_PX
PATCH_SIDE = STEP * CELL_PX


def _aug_label_table():
    table = np.empty((8, NB_CLASSES), np.uint8)
    for t in range(8):
        for label in range(NB_CLASSES):
            block = np.rot90(DIGITS[label].reshape(STEP, STEP), t & 3)
            block = block[:, ::-1] if t & 4 else block
            table[t, label] = int((block.reshape(-1).astype(np.int64) * 3 ** np.arange(STEP * STEP)).sum())
    return table


AUG_LABEL = _aug_label_table()
SNAPSHOT_SUFFIXES = (".npy", ".jpg", ".jpeg", ".png")      # an array, or a still read through open_capture (.png: the reference's own snapshots)

# The trained model file.  The reference downloads the author's keras.h5 into its training directory
# (stone/nn_manager.py:22, 65-90); that file cannot be fetched here, so the package ships a classifier trained on the
# synthetic renderer (tools/train_cnn.py) in the same Keras-1 HDF5 layout.  $CAMKIFU_KERAS_MODEL overrides the path.
PACKAGED_MODEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "keras.h5")
KERAS_MODEL_FILE = os.environ.get("CAMKIFU_KERAS_MODEL") or PACKAGED_MODEL
GOLDEN_WEIGHTS = KERAS_MODEL_FILE


class ModelMissing(FileNotFoundError):
    pass


def _seeded_weights():
    from .. import synth
    return synth.cnn_weights()


class NNManager:
    _network, _guard = None, RLock()      # the weights, loaded once per process like the reference's lazily built model

    def __init__(self):
        self.canonical_shape = (cvconf.canonical_size,) * 2
        self.split, self.step, self.nb_classes = SPLIT, STEP, NB_CLASSES
        self.r_width = self.c_width = PATCH_SIDE
        self.c_indices = self._class_table = None

    # ---- model ---------------------------------------------------------------------------------
    @classmethod
    def get_net(cls, download=False):
        with cls._guard:
            if cls._network is None:
                cls._network = cls.init_net()
            return cls._network

    def init_net(download=False, allow_random=False):
        """the twelve weight arrays (Keras-1 'tf' layout) from KERAS_MODEL_FILE.  A missing file is an error -- a
        classifier with random weights reads garbage -- unless seeded random weights are asked for explicitly
        (numerics tests use them)."""
        if os.path.isfile(KERAS_MODEL_FILE):
            return NNManager.load_model(KERAS_MODEL_FILE)
        if allow_random:
            return _seeded_weights()
        raise ModelMissing("stone classifier model not found: %s (set CAMKIFU_KERAS_MODEL)" % KERAS_MODEL_FILE)

    def load_model(path):
        """the twelve arrays of a Keras-1 HDF5 model, or of an .npz checkpoint (save_model, tools/train_cnn.py)"""
        if str(path).endswith(".npz"):
            from ..capi import WEIGHT_ORDER, WEIGHT_SHAPES
            with np.load(path) as z:
                net = {k: np.ascontiguousarray(z[k], np.float32) for k in WEIGHT_ORDER}
            for k, a in net.items():
                if a.shape != WEIGHT_SHAPES[k]:
                    raise ValueError("%s: %s has shape %r, expected %r" % (path, k, a.shape, WEIGHT_SHAPES[k]))
            return net
        from . import keras1
        return keras1.load_model(path)

    def save_model(net, path):
        """the checkpoint format: an .npz of the twelve arrays under their WEIGHT_ORDER names"""
        from ..capi import WEIGHT_ORDER
        with open(path, "wb") as f:
            np.savez(f, **{k: np.ascontiguousarray(net[k], np.float32) for k in WEIGHT_ORDER})

    def get_nb_weights(net=None):
        net = _seeded_weights() if net is None else net
        return int(sum(int(np.prod(a.shape)) for a in net.values()))

    def create_net():
        """the architecture of nn_manager.py:277-298 with seeded He-normal weights (untrained)"""
        return _seeded_weights()

    init_net, load_model, create_net = staticmethod(init_net), staticmethod(load_model), staticmethod(create_net)
    save_model, get_nb_weights = staticmethod(save_model), staticmethod(get_nb_weights)

    # ---- geometry --------------------------------------------------------------------------------
    def _subregion(self, ri, cj):
        """(row start, row end, col start, col end) of region (ri, cj), ends exclusive"""
        r0, c0 = int(REGION_START[ri]), int(REGION_START[cj])
        return r0, r0 + STEP, c0, c0 + STEP

    def get_region_indices(self, row, col):
        return row // STEP, col // STEP

    def getrect(self, row, col, re=0, ce=0):
        """pixel box (x0, y0, x1, y1) of intersections row..re, col..ce (inclusive; 0 = just row / col), canonical image"""
        last_r, last_c = (re if re > 0 else row), (ce if ce > 0 else col)
        return row * CELL_PX, col * CELL_PX, (last_r + 1) * CELL_PX, (last_c + 1) * CELL_PX

    def _get_rect_nn(self, r0, r1, c0, c1):
        """(x0, x1, y0, y1) of the classifier's window for a block of intersections: always PATCH_SIDE wide,
        anchored at the block's far edge"""
        x1, y1 = r1 * CELL_PX, c1 * CELL_PX
        return x1 - PATCH_SIDE, x1, y1 - PATCH_SIDE, y1

    def _get_x(self, ri, cj, image):
        a, b = int(PATCH_ORIGIN[ri]), int(PATCH_ORIGIN[cj])
        return image[a:a + PATCH_SIDE, b:b + PATCH_SIDE]

    # ---- codec -----------------------------------------------------------------------------------
    def compute_label(r0, r1, c0, c1, stones):
        block = np.asarray(stones)[r0:r1, c0:c1].reshape(-1)
        return int(sum(CODE[s] * 3 ** k for k, s in enumerate(block)))

    def compute_stones(label, dimension=STEP * STEP):
        if dimension == STEP * STEP:
            return SYMBOLS[DIGITS[int(label)]]
        return SYMBOLS[(int(label) // 3 ** np.arange(dimension)) % 3]

    compute_label, compute_stones = staticmethod(compute_label), staticmethod(compute_stones)

    def class_indices(self):
        """[intersection k, colour, :] = the labels that put that colour on that intersection (27 each)"""
        table = self._class_table
        if table is None:
            per_colour = [[np.flatnonzero(DIGITS[:, k] == col) for col in range(3)] for k in range(STEP * STEP)]
            table = self.c_indices = self._class_table = np.array(per_colour, np.uint8)
        return table

    # ---- datasets (.npz: X uint8 N x 40 x 40 x 3, Y bool N x 81) ----------------------------------
    def generate_xs(self, img):
        """the 100 classifier windows of a canonical image, region (i, j) at i * 10 + j"""
        if tuple(img.shape[:2]) != self.canonical_shape:
            raise ValueError("canonical image expected, got %r" % (tuple(img.shape),))
        rows = PATCH_ORIGIN[:, None] + np.arange(PATCH_SIDE)[None, :]
        cut = np.asarray(img)[rows[:, None, :, None], rows[None, :, None, :]]
        return np.ascontiguousarray(cut.reshape((SPLIT * SPLIT, PATCH_SIDE, PATCH_SIDE) + tuple(img.shape[2:])), np.uint8)

    def generate_ys(self, stones):
        """one-hot labels (100, 81) of the regions of a 19 x 19 grid of E / B / W"""
        ys = np.zeros((SPLIT * SPLIT, NB_CLASSES), bool)
        for i, r0 in enumerate(REGION_START):
            for j, c0 in enumerate(REGION_START):
                ys[i * SPLIT + j, NNManager.compute_label(r0, r0 + STEP, c0, c0 + STEP, stones)] = True
        return ys

    # ---- datasets from snapshots (nn_manager.py:133-176) -------------------------------------------------------
    @staticmethod
    def _stem(path):
        for suffix in SNAPSHOT_SUFFIXES:
            if str(path).lower().endswith(suffix):
                return str(path)[:-len(suffix)]
        raise ValueError("a snapshot is a .npy, .jpg or .png file: %s" % (path,))

    @staticmethod
    def get_ref_game(img_path):
        """snapshot-N.* -> game-N.sgf beside it; a copy's name 'snapshot-N (2).npy' falls back to the game of snapshot-N"""
        folder, name = os.path.split(NNManager._stem(img_path))
        game_path = os.path.join(folder, name.replace("snapshot", "game") + ".sgf")
        return game_path if os.path.isfile(game_path) else re.sub(r" \(\d*\)", "", game_path)

    @staticmethod
    def get_ref_y(path):
        """snapshot-N.* -> snapshot-N-y.npz (labels saved earlier), with the same fall-back"""
        y_path = NNManager._stem(path) + "-y.npz"
        return y_path if os.path.isfile(y_path) else re.sub(r" \(\d*\)", "", y_path)

    @staticmethod
    def load_snapshot(img_path):
        NNManager._stem(img_path)
        if str(img_path).lower().endswith(".npy"):
            return np.load(img_path)
        from ..core.capture import open_capture
        ok, img = open_capture(str(img_path)).read()
        if not ok:
            raise ValueError("cannot read %s" % (img_path,))
        return img

    def suggest_stones(self, img, img_path):
        """the stones of a snapshot (19, 19) of E / B / W: from game-N.sgf beside it (played out under the rules, as the
        reference's controller does), else from snapshot-N-y.npz, else the classifier's own reading of the image.
        self.stones_source says which: "sgf", "y" or "guess"."""
        game_path, y_path = NNManager.get_ref_game(img_path), NNManager.get_ref_y(img_path)
        if os.path.isfile(game_path):
            from .harvest import reference_positions
            self.stones_source = "sgf"
            return SYMBOLS[reference_positions(game_path, rules=True)[-1]]
        if os.path.isfile(y_path):
            stones = np.empty((gsize, gsize), dtype=object)
            with np.load(y_path) as z:
                y = np.asarray(z["Y"])
            for i, r0 in enumerate(REGION_START):
                for j, c0 in enumerate(REGION_START):
                    stones[r0:r0 + STEP, c0:c0 + STEP] = NNManager.compute_stones(np.argmax(y[i * SPLIT + j])).reshape(STEP, STEP)
            self.stones_source = "y"
            return stones
        from .nn_cache import NNCache
        self.stones_source = "guess"
        return NNCache(self, img, self._context()).predict_all_stones()[:, :, 0]

    def gen_data(self, img_path, validate=None):
        """(X (100, 40, 40, 3), Y (100, 81)) of a snapshot of the canonical goban image, or (None, None).  validate: the
        reference's labelling window as a callable (stones, img) -> bool that may edit `stones` in place; without one only
        stones that come from a game record or from saved labels are accepted -- a guess is not training data."""
        img = NNManager.load_snapshot(img_path)
        if tuple(img.shape[:2]) != self.canonical_shape:
            raise ValueError("canonical image expected, got %r" % (tuple(img.shape),))
        if validate is None and not (os.path.isfile(NNManager.get_ref_game(img_path)) or os.path.isfile(NNManager.get_ref_y(img_path))):
            return None, None
        stones = self.suggest_stones(img, img_path)
        if validate is not None and not validate(stones, img):
            return None, None
        return self.generate_xs(img), self.generate_ys(stones)

    # ---- training ------------------------------------------------------------------------------------
    def _context(self):
        if getattr(self, "ctx", None) is None:
            from .. import capi
            self.ctx = capi.get_context()
        return self.ctx

    @staticmethod
    def _class_index(y):
        y = np.asarray(y)
        return (y.argmax(1) if y.ndim == 2 else y).astype(np.uint8)

    @staticmethod
    def epoch_order(n, seed, epoch):
        """the order in which epoch `epoch` visits the n samples: a function of (seed, epoch) alone"""
        return np.random.default_rng([int(seed), int(epoch)]).permutation(n)

    @staticmethod
    def augment_codes(idx, seed, epoch, n):
        """the transform codes 0..7 (AUG_LABEL) of samples idx of a dataset of n in epoch `epoch`: one draw of n codes from
        the generator seeded [seed, epoch, 1], indexed by idx -- a function of the sample, not of the batch it rides in"""
        return np.random.default_rng([int(seed), int(epoch), 1]).integers(0, 8, size=int(n), dtype=np.uint8)[np.asarray(idx)]

    def train(self, x, y, vdata=None, batch_size=1000, nb_epoch=2, lr=0.001, seed=20161001, dropout=True, checkpoint=None,
              net=None, verbose=True, augment=False):
        """Fit the classifier to patches x (N, 40, 40, 3) uint8 with labels y (one-hot (N, 81) or N class indices) on the
        GPU, starting from `net` (default: the current network, see get_net).  Adam, categorical cross-entropy,
        the samples reshuffled per epoch from `seed`.  Prints the loss per epoch (and the loss on vdata = (xv, yv)),
        writes `checkpoint` (.npz) whenever the epoch's mean loss improves -- ModelCheckpoint(monitor='loss',
        save_best_only=True) -- hands the trained weights to the context's classifier and makes them the current
        network.  -> history dict(loss=[..], val_loss=[..])
        augment: every sample is turned / mirrored by its code of the epoch (augment_codes) on the GPU -- the batch goes
        through Context.augment_patches into HBM and into the training step from there, with labels AUG_LABEL[t, label]."""
        ctx = self._context()
        x, labels = np.ascontiguousarray(x, np.uint8), self._class_index(y)
        start = NNManager.get_net() if net is None else net
        handle = ctx.train_create(start)
        history, best, step = dict(loss=[], val_loss=[]), None, 0
        try:
            for epoch in range(int(nb_epoch)):
                order, total = self.epoch_order(len(x), seed, epoch), 0.0
                for k in range(0, len(order), int(batch_size)):
                    idx = order[k:k + int(batch_size)]
                    xb, lb = x[idx], labels[idx]
                    if augment:
                        import torch
                        t = self.augment_codes(idx, seed, epoch, len(x))
                        xb, lb = ctx.augment_patches(xb, t, to_device=torch.device("cuda", ctx.device)), AUG_LABEL[t, lb]
                    total += ctx.train_step(handle, xb, lb, lr=lr, dropout=dropout, seed=seed) * len(idx)
                    step += 1
                history["loss"].append(total / len(x))
                line = "epoch %d/%d - loss: %.4f" % (epoch + 1, nb_epoch, history["loss"][-1])
                if vdata is not None:
                    xv, yv = np.ascontiguousarray(vdata[0], np.uint8), self._class_index(vdata[1])
                    parts = [ctx.train_grads(handle, xv[k:k + 1000], yv[k:k + 1000])[0] * len(xv[k:k + 1000])
                             for k in range(0, len(xv), 1000)]
                    history["val_loss"].append(sum(parts) / len(xv))
                    line += " - val_loss: %.4f" % history["val_loss"][-1]
                if verbose:
                    print(line, flush=True)
                if best is None or history["loss"][-1] < best:
                    best = history["loss"][-1]
                    if checkpoint is not None:
                        NNManager.save_model(ctx.train_weights(handle), checkpoint)
            ctx.train_handover(handle)
            with NNManager._guard:
                NNManager._network = ctx.train_weights(handle)
        finally:
            ctx.train_destroy(handle)
        return history

    def predict_ys(self, x):
        """argmax class index of each patch of x (N, 40, 40, 3), by the context's classifier as it stands (after train():
        the trained weights).  The patches ride through the inference kernels 81 to a canonical image, in the regions
        whose windows do not overlap (i, j < 9)."""
        ctx = self._context()
        x = np.ascontiguousarray(x, np.uint8)
        per = (SPLIT - 1) ** 2
        sheets = np.zeros((-(-len(x) // per),) + self.canonical_shape + (3,), np.uint8)
        slot = np.arange(len(x))
        f, i, j = slot // per, (slot % per) // (SPLIT - 1), slot % (SPLIT - 1)
        for k in range(len(x)):
            a, b = int(PATCH_ORIGIN[i[k]]), int(PATCH_ORIGIN[j[k]])
            sheets[f[k], a:a + PATCH_SIDE, b:b + PATCH_SIDE] = x[k]
        out = np.empty(len(x), np.int64)
        for s in range(0, len(sheets), 64):
            yy = ctx.cnn_predict(sheets[s:s + 64])[0]
            sel = (f >= s) & (f < s + 64)
            out[sel] = yy[f[sel] - s, i[sel] * SPLIT + j[sel]].argmax(1)
        return out

    def evaluate(self, x, y):
        """the reference's two figures on (x, y): of the non-empty regions (label > 0) how many get exactly their label,
        of the empty ones (label 0) how many are called empty.  Prints both lines -> (tp, ap, tn, an)"""
        truth, pred = self._class_index(y).astype(np.int64), np.asarray(self.predict_ys(x))
        hit, full = pred == truth, truth != 0
        tp, ap, tn, an = int((hit & full).sum()), int(full.sum()), int((hit & ~full).sum()), int((~full).sum())
        print("Non-empty: %.2f %% (%d/%d)" % (100.0 * tp / ap if ap else 0, tp, ap))
        print("Empty    : %.2f %% (%d/%d)" % (100.0 * tn / an if an else 0, tn, an))
        return tp, ap, tn, an

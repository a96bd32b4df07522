#!/usr/bin/env python3
"""Train and evaluate the stone classifier on the GPU (after the reference's stone/nn_runner.py).

    python tools/nn_runner.py --synthetic 20 --out data.npz                 a dataset from the renderer (no footage needed)
    python tools/nn_runner.py --synthetic 20 --train data.npz --out m.npz   the same, written to data.npz and trained on
    python tools/nn_runner.py --train data.npz [--valid v.npz] [--epochs 2 --batch 1000 --lr 0.001 --out model.npz]
    python tools/nn_runner.py --evaluate data.npz [--model model.npz]
    python tools/nn_runner.py --harvest FILM.y4m --sgf GAME.sgf --out data.npz      labelled patches from a filmed game
                              [--rules --per-state N --stride N --calm-max N --empty-keep N --batch N]
    python tools/nn_runner.py --merge A.npz B.npz ... --out all.npz
    python tools/nn_runner.py --split 0.8 data.npz      seeded shuffle -> data-train.npz / data-test.npz
    python tools/nn_runner.py --histo data.npz          label counts
    ... --train data.npz --augment                      every sample turned / mirrored per epoch, on the GPU

A dataset is an .npz with X uint8 (N, 40, 40, 3) and Y bool (N, 81); a model is an .npz of the twelve weight arrays
(NNManager.save_model) or a Keras-1 HDF5 file.  Training starts from --model, by default from the seeded untrained
network of NNManager.create_net; point $CAMKIFU_KERAS_MODEL at the written model to use it.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from camkifu_amd import synth  # noqa: E402
from camkifu_amd.stone.nn_manager import NNManager  # noqa: E402


def synthetic(nboards, seed=1):
    """boards drawn straight into the canonical frame with corners a few pixels off, as a detected transform leaves them
    (the recipe of tools/train_cnn.py:make_boards), cut and labelled by NNManager.generate_xs / generate_ys"""
    rng = np.random.default_rng(seed)
    from camkifu_amd.stone.nn_manager import SYMBOLS as symbols
    mgr = NNManager()
    X, Y = [], []
    for b in range(nboards):
        stones = synth.random_stones(rng, density=rng.uniform(0.0, 0.65), keep_first_line_empty=(b % 3 == 0))
        corners = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32) + rng.uniform(-3, 3, (4, 2)).astype(np.float32)
        img = synth.render(380, 380, stones, corners, seed=seed * 100000 + b, noise=rng.uniform(1.5, 4.5)).numpy()
        X.append(mgr.generate_xs(img))
        Y.append(mgr.generate_ys(symbols[stones]))
    return np.concatenate(X), np.concatenate(Y)


def load_set(path):
    with np.load(path) as z:
        return np.ascontiguousarray(z["X"], np.uint8), np.asarray(z["Y"])


def merge_npz(paths):
    """the datasets of several files end to end (the reference's merge_npz) -> (X, Y)"""
    sets = [load_set(p) for p in paths]
    X, Y = np.concatenate([s[0] for s in sets]), np.concatenate([np.asarray(s[1], bool) for s in sets])
    print("Merged %d inputs -> %r" % (len(sets), X.shape))
    return X, Y


def split_data(X, Y, ratio=0.8, seed=synth.SEED):
    """a seeded shuffle, the first `ratio` of it to train on and the rest to test on (the reference's split_data)
    -> (Xt, Yt, Xe, Ye)"""
    order = np.random.default_rng([int(seed), 2]).permutation(len(X))
    cut = int(ratio * len(order))
    return X[order[:cut]], Y[order[:cut]], X[order[cut:]], Y[order[cut:]]


def histo(Y):
    """-> (counts of the 81 labels, as the reference's raw_histo; counts of the regions holding 0, 1, .. 4 stones)"""
    from camkifu_amd.stone.nn_manager import DIGITS, NB_CLASSES
    labels = np.asarray(Y).argmax(1) if np.asarray(Y).ndim == 2 else np.asarray(Y)
    per_label = np.bincount(labels.astype(np.int64), minlength=NB_CLASSES)
    per_stones = np.bincount((DIGITS > 0).sum(1), weights=per_label, minlength=5).astype(np.int64)
    return per_label, per_stones


def print_histo(Y):
    per_label, per_stones = histo(Y)
    names = ("empty", "one stone", "two stones", "three stones", "four stones")
    for name, count in zip(names, per_stones):
        print("%-12s %8d" % (name, count))
    for label in np.flatnonzero(per_label):
        print("label %2d     %8d" % (label, per_label[label]))


def harvest(film, sgf, out, rules=False, per_state=None, stride=1, calm_max=16, empty_keep=256, seed=synth.SEED, batch=256,
            model=None):
    """the film and its game record through camkifu_amd.stone.harvest.Harvester -> the dataset, written to `out`; the finder
    reads the stones with `model` (default: the current network)"""
    from camkifu_amd.core.capture import open_capture
    from camkifu_amd.stone.harvest import Harvester
    capture = open_capture(film)
    if not capture.isOpened():
        raise SystemExit("cannot open %s: %s" % (film, getattr(capture, "error", "")))
    hv = Harvester(capture.h, capture.w, sgf, rules=rules, per_state=per_state, stride=stride, calm_max=calm_max,
                   empty_keep=empty_keep, seed=seed, net=NNManager.load_model(model) if model else None)
    try:
        data = hv.run(capture, batch=batch)
    finally:
        hv.close()
    hv.save(out)
    print("wrote %s: %d patches of %d frames, %d non-empty" % (out, len(data["X"]), len(set(data["frame"].tolist())),
                                                               int((data["Y"].argmax(1) > 0).sum()) if len(data["X"]) else 0))
    return data


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synthetic", type=int, metavar="NBOARDS")
    ap.add_argument("--train", metavar="DATA.npz")
    ap.add_argument("--valid", metavar="V.npz")
    ap.add_argument("--evaluate", metavar="DATA.npz")
    ap.add_argument("--model", metavar="M", help="model to start from / to evaluate (.npz or Keras-1 .h5)")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=synth.SEED)
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--out", metavar="FILE.npz")
    ap.add_argument("--harvest", metavar="FILM", help="a .y4m / .avi film of a game; needs --sgf and --out")
    ap.add_argument("--sgf", metavar="GAME.sgf")
    ap.add_argument("--rules", action="store_true", help="captures leave the goban (both the finder's board and the game's)")
    ap.add_argument("--per-state", type=int, metavar="N", help="at most N frames per position of the game")
    ap.add_argument("--stride", type=int, default=1, metavar="N", help="every N-th eligible frame of a position")
    ap.add_argument("--calm-max", type=int, default=16, metavar="N")
    ap.add_argument("--empty-keep", type=int, default=256, metavar="N", help="of 256 empty regions, keep N")
    ap.add_argument("--merge", nargs="+", metavar="A.npz")
    ap.add_argument("--split", nargs=2, metavar=("RATIO", "DATA.npz"))
    ap.add_argument("--histo", metavar="DATA.npz")
    ap.add_argument("--augment", action="store_true", help="with --train: turn / mirror every sample per epoch")
    a = ap.parse_args(argv)
    if a.synthetic is None and not (a.train or a.evaluate or a.harvest or a.merge or a.split or a.histo):
        ap.error("one of --synthetic, --train, --evaluate, --harvest, --merge, --split, --histo")
    if a.harvest:
        if not a.sgf or not a.out:
            ap.error("--harvest needs --sgf and --out")
        harvest(a.harvest, a.sgf, a.out, rules=a.rules, per_state=a.per_state, stride=a.stride, calm_max=a.calm_max,
                empty_keep=a.empty_keep, seed=a.seed, batch=min(a.batch, 256), model=a.model)
    if a.merge:
        if not a.out:
            ap.error("--merge needs --out")
        X, Y = merge_npz(a.merge)
        np.savez_compressed(a.out, X=X, Y=Y)
    if a.split:
        ratio, path = float(a.split[0]), a.split[1]
        Xt, Yt, Xe, Ye = split_data(*load_set(path), ratio=ratio, seed=a.seed)
        stem = path[:-4] if path.endswith(".npz") else path
        np.savez_compressed(stem + "-train.npz", X=Xt, Y=Yt)
        np.savez_compressed(stem + "-test.npz", X=Xe, Y=Ye)
        print("wrote %s-train.npz (%d) and %s-test.npz (%d)" % (stem, len(Xt), stem, len(Xe)))
    if a.histo:
        print_histo(load_set(a.histo)[1])
    if a.synthetic is None and not (a.train or a.evaluate):
        return 0
    mgr = NNManager()
    if a.synthetic is not None:
        X, Y = synthetic(a.synthetic, seed=a.seed % 100000)
        out = a.train or a.out or "synthetic_%d.npz" % a.synthetic       # with --train: written there, then trained on
        np.savez_compressed(out, X=X, Y=Y)
        print("wrote %s: %d patches, %d non-empty" % (out, len(X), int((Y.argmax(1) > 0).sum())))
    if a.train:
        X, Y = load_set(a.train)
        net = NNManager.load_model(a.model) if a.model else NNManager.create_net()
        out = a.out or "model.npz"
        hist = mgr.train(X, Y, vdata=load_set(a.valid) if a.valid else None, batch_size=a.batch, nb_epoch=a.epochs, lr=a.lr,
                         seed=a.seed, dropout=not a.no_dropout, checkpoint=out, net=net, augment=a.augment)
        print("best loss %.4f, model in %s" % (min(hist["loss"]), out))
        mgr.evaluate(X, Y)
    if a.evaluate:
        if not a.train or a.model:
            net = NNManager.load_model(a.model) if a.model else NNManager.get_net()
            mgr._context().cnn_set_weights(net)
        mgr.evaluate(*load_set(a.evaluate))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Train and evaluate the stone classifier on the GPU (after the reference's stone/nn_runner.py).

    python tools/nn_runner.py --synthetic 20 --out data.npz                 a dataset from the renderer (no footage needed)
    python tools/nn_runner.py --synthetic 20 --train data.npz --out m.npz   the same, written to data.npz and trained on
    python tools/nn_runner.py --train data.npz [--valid v.npz] [--epochs 2 --batch 1000 --lr 0.001 --out model.npz]
    python tools/nn_runner.py --evaluate data.npz [--model model.npz]

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
    a = ap.parse_args(argv)
    if a.synthetic is None and not a.train and not a.evaluate:
        ap.error("one of --synthetic, --train, --evaluate")
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
                         seed=a.seed, dropout=not a.no_dropout, checkpoint=out, net=net)
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

"""The classifier's training step on the GPU (camkifu_amd/csrc/k_cnn_train.hip through ck_train_*) against the plain
float64 reference tests/train_ref.py on the inputs of tests/train_cases.py.

Tolerance of the gradient tests.  The error of a tensor is max |g - g_ref| / max |g_ref|; the loss is compared relatively.
ReLU signs and pool winners are discrete, so no bound follows from rounding alone; the yardstick is torch's own float32
autograd against float64 on these very cases, measured on the CPU:
    n1 1.4e-6   n3 1.2e-6   n65 2.1e-6   n257 1.9e-6   empty 5.1e-7   white 1.7e-6   ties 1.2e-6   (largest tensor of each
    case; c1w every time; losses 6e-9 .. 1.5e-7).  Nothing flips in torch's float32 on these cases, although n257 holds a
    pool window whose best two values are 1.5 float32 ulp apart (docs/lab_notes.md 13: a trainer whose forward pass was an
    f32 chain over K decided it otherwise and missed TOL with c2w 5.6e-5; the forward pass is correctly rounded since).
MEASURED = 2.13e-6 is the largest, TOL = 4 x MEASURED = 8.5e-6 (summation orders differ).  Every mutant below is wrong by
1e-2 or more of a tensor's scale (tests/test_train_ref_cpu.py::test_the_cases_tell_the_mutants_apart), so the margin hides none.

The Adam test holds the library to the float64 Adam of train_ref with its state HELD in float32 between updates, as the
library holds it: an update is then a function of float32 inputs, and 2 ulp of the result is a bound a trainer that
computes the update in double meets whatever the gradient (zeros, 1e-12, weights that nearly cancel).

Mutants of the trainer that must each fail this file, and the tests / cases that see them (as the reference with the same
mistake differs from the reference, tests/test_train_ref_cpu.py):
    kernel flipped in the data gradient          gradients: every case (c1w .. c3w)
    pool gradient to the last maximum            gradients: `ties` only.  Under the seeded weights windows tie at 0 (where
                                                 relu'(0) = 0 routes nothing whichever maximum is taken) and in flat
                                                 patches (where the input does not vary, so the choice changes no sum);
                                                 `ties` has constant maps above 0 over an input that varies
    pool gradient to every maximum               gradients: `ties`, and `empty` (its flat patches: four times the sums)
    relu'(0) = 1 (`out >= 0` on the kept map)    gradients: every case (half the units behind a ReLU are exact zeros)
    bias gradient not summed over positions      gradients: every case (c1b .. c4b)
    loss summed instead of averaged              gradients and loss: every case with n > 1
    the last patch of a chunk dropped            gradients: n65 and n257 only
    dropout without 1 / (1 - p)                  test_gradients_with_dropout
    Adam without bias correction                 test_adam_alone
    eps inside the square root                   test_adam_alone (the 1e-12 and zero gradients)"""
import os

import numpy as np
import pytest

from tests import train_cases as tc
from tests import train_ref as tr

pytestmark = pytest.mark.gpu
MEASURED = 2.13e-6
TOL = 4 * MEASURED
CASES = ("n1", "n3", "n65", "n%d" % (tc.CHUNK + 1), "empty", "white", "ties")
LOSS30_F32 = 3.26e-3        # the float32 torch reference on learn_set() after 30 of the 60 steps (lr 1e-3, dropout off); 7.3e-6 after 60


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture()
def trainer(ck):
    h = ck.train_create(tc.weights())
    yield h
    ck.train_destroy(h)


def _check(loss, grads, ref, tag):
    l_ref, g_ref = ref
    err = tr.grad_error(grads, g_ref)
    lerr = abs(loss - l_ref) / abs(l_ref)
    print(tag, "loss %.7f ref %.7f rel %.2e" % (loss, l_ref, lerr), " ".join("%s %.1e" % kv for kv in err.items()))
    assert lerr <= TOL, (tag, loss, l_ref)
    for k, e in err.items():
        assert e <= TOL, (tag, k, e)


@pytest.mark.parametrize("name", CASES)
def test_gradients_without_dropout(ck, name):
    """1: all 12 gradients and the loss of every case against float64, within TOL"""
    x, y = tc.cases()[name]
    handle = ck.train_create(tc.weights_of(name))
    try:
        loss, grads, masks = ck.train_grads(handle, x, y, dropout=False)
    finally:
        ck.train_destroy(handle)
    assert masks is None
    _check(loss, grads, tc.reference(name), name)


def test_gradients_with_dropout(ck, trainer):
    """2: with the library's own keep-masks given to the reference the gradients meet the same tolerance (so kept units
    carry 1 / (1 - p): the reference applies it); the kept fraction of each mask is within 6 binomial standard deviations
    of 1 - p (pool 1 at n = 8: 65 536 units, 49 152 +- 666); the masks are a function of (seed, step) alone"""
    X, Y = tc.pool()
    x, y = X[:8], Y[:8]
    loss, grads, masks = ck.train_grads(trainer, x, y, dropout=True, seed=11, step=3)
    assert [m.shape for m in masks] == [(8, 16, 16, 32), (8, 6, 6, 90), (8, 160)]
    for m, p in zip(masks, (0.25, 0.25, 0.5)):
        assert set(np.unique(m)) <= {0, 1}
        n = m.size
        assert abs(int(m.sum()) - n * (1 - p)) <= 6 * np.sqrt(n * p * (1 - p)), (m.shape, int(m.sum()))
    _check(loss, grads, tr.loss_and_grads(tc.weights(), x, y, masks=masks), "dropout")
    again = ck.train_grads(trainer, x, y, dropout=True, seed=11, step=3)
    assert all(np.array_equal(a, b) for a, b in zip(masks, again[2]))
    assert all(np.array_equal(again[1][k], grads[k]) for k in tr.ORDER) and again[0] == loss
    for other in (dict(seed=11, step=4), dict(seed=12, step=3)):
        m2 = ck.train_grads(trainer, x, y, dropout=True, **other)[2]
        for a, b in zip(masks, m2):
            assert 0.2 < float((a != b).mean()) < 0.6           # independent masks differ in 2 p (1 - p) = 0.375 / 0.5 of the units
    # a patch's mask does not depend on the batch it came in: the unit index is global
    m3 = ck.train_grads(trainer, x[:3], y[:3], dropout=True, seed=11, step=3)[2]
    assert all(np.array_equal(a[:3], b) for a, b in zip(masks, m3))


def test_adam_alone(ck, trainer):
    """3: three ck_train_apply calls with given float32 gradients -- normal ones, exact zeros, 1e-12 (where g / (sqrt(v) + eps)
    is most sensitive) -- against the float64 Adam; weights within 2 float32 ulp, moments within 1, the update count"""
    rng = np.random.default_rng(3)
    W = tc.weights()
    ref = tr.Adam(W, state=np.float32)
    for step in range(3):
        g = {}
        for k in tr.ORDER:
            a = (rng.standard_normal(W[k].shape) * 10.0 ** rng.integers(-4, 1)).astype(np.float32)
            kind = rng.integers(0, 4, a.shape)
            a[kind == 0] = 0.0
            a[kind == 1] = np.float32(1e-12) * np.sign(a[kind == 1])
            g[k] = a
        ck.train_apply(trainer, g, lr=0.001)
        ref.apply(g, lr=0.001)
        w = ck.train_weights(trainer)
        m, v, steps = ck.train_adam_state(trainer)
        assert steps == step + 1 == ref.t
        for k in tr.ORDER:
            assert tr.ulps(w[k], ref.w[k]).max() <= 2, (step, k)
            assert tr.ulps(m[k], ref.m[k]).max() <= 1 and tr.ulps(v[k], ref.v[k]).max() <= 1, (step, k)


def test_steps_repeat_bit_for_bit(ck):
    """4: two fresh trainers, the same three steps at n = 65 with dropout: every weight and moment bit-equal"""
    x, y = tc.cases()["n65"]
    runs = []
    for _ in range(2):
        h = ck.train_create(tc.weights())
        losses = [ck.train_step(h, x, y, lr=0.001, dropout=True, seed=5) for _ in range(3)]
        m, v, steps = ck.train_adam_state(h)
        runs.append((losses, ck.train_weights(h), m, v, steps))
        ck.train_destroy(h)
    a, b = runs
    assert a[0] == b[0] and a[4] == b[4] == 3
    for part in (1, 2, 3):
        for k in tr.ORDER:
            assert np.array_equal(a[part][k].view(np.uint32), b[part][k].view(np.uint32)), (part, k)
    assert any(not np.array_equal(a[1][k], tc.weights()[k]) for k in tr.ORDER)


def test_it_learns(ck, trainer):
    """5: 32 patches of one board (24 non-empty, 8 empty), 60 steps at lr 1e-3 without dropout: the loss ends at or below
    what the float32 torch reference reaches after HALF the steps (LOSS30_F32; Adam amplifies rounding, so trajectories
    part, but a correct trainer is not twice as slow), and every training patch gets its label"""
    x, y = tc.learn_set()
    losses = [ck.train_step(trainer, x, y, lr=0.001, dropout=False) for _ in range(60)]
    final = ck.train_grads(trainer, x, y)[0]
    print("loss: first %.4f, after 30 %.3e, after 60 %.3e" % (losses[0], losses[30], final))
    assert final <= LOSS30_F32
    assert np.array_equal(tr.forward(ck.train_weights(trainer), x).argmax(1), y)


def test_through_the_public_interface(ck, tmp_path, capsys):
    """6: NNManager.train on 3 synthetic boards (2 epochs, batch 100): the loss falls, the checkpoint loads, the handed-over
    weights classify as the float64 forward of the trained weights does (the bound of test_cnn_against_torch_fp64), and
    evaluate's counts are a recount of predict_ys"""
    from camkifu_amd.stone.nn_manager import NNManager
    X, Y = tc.pool()
    mgr = NNManager()
    mgr.ctx = ck
    path = os.path.join(str(tmp_path), "model.npz")
    saved = NNManager._network
    try:
        hist = mgr.train(X, np.eye(81, dtype=bool)[Y], vdata=(X[:50], Y[:50]), batch_size=100, nb_epoch=2, lr=0.001, seed=1,
                         checkpoint=path, net=tc.weights())
        trained = NNManager.get_net()
    finally:
        NNManager._network = saved
    assert len(hist["loss"]) == 2 and len(hist["val_loss"]) == 2 and hist["loss"][1] < hist["loss"][0]
    assert "loss:" in capsys.readouterr().out
    loaded = NNManager.load_model(path)
    for k in tr.ORDER:
        assert np.array_equal(loaded[k], trained[k]), k           # the loss fell, so the last epoch wrote the checkpoint
    # after the hand-over: ck_cnn_predict on canonical images made of those patches
    sheet = np.zeros((1, 380, 380, 3), np.uint8)
    for i in range(9):
        for j in range(9):
            sheet[0, 40 * i:40 * i + 40, 40 * j:40 * j + 40] = X[9 * i + j]
    y_gpu = ck.cnn_predict(sheet)[0][0].reshape(10, 10, 81)[:9, :9].reshape(81, 81)
    y64 = tr.forward(trained, X[:81])
    assert np.abs(y_gpu - y64).max() <= 1e-4
    pred = mgr.predict_ys(X)
    top2 = np.sort(tr.forward(trained, X), axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-3
    assert np.array_equal(pred[clear], tr.forward(trained, X).argmax(1)[clear])
    tp, ap, tn, an = mgr.evaluate(X, Y)
    assert ap + an == len(X)
    assert (tp, ap, tn, an) == (int(((pred == Y) & (Y > 0)).sum()), int((Y > 0).sum()), int(((pred == Y) & (Y == 0)).sum()), int((Y == 0).sum()))
    out = capsys.readouterr().out
    assert "Non-empty:" in out and "Empty    :" in out


def test_errors_are_errors(ck, trainer):
    """7: a label of 81, patches of the wrong shape and a destroyed handle raise RuntimeError with the library's message;
    the context and the trainer work afterwards"""
    x, y = tc.cases()["n3"]
    with pytest.raises(RuntimeError, match="label 81"):
        ck.train_step(trainer, x, np.array([0, 81, 2]))
    with pytest.raises(RuntimeError, match="40 x 40 x 3"):
        ck.train_step(trainer, x[:, :38], y)
    dead = ck.train_create(tc.weights())
    ck.train_destroy(dead)
    for call in (lambda: ck.train_step(dead, x, y), lambda: ck.train_weights(dead), lambda: ck.train_handover(dead),
                 lambda: ck.train_destroy(dead), lambda: ck.train_weights(99)):
        with pytest.raises(RuntimeError, match="bad trainer handle"):
            call()
    assert ck.train_adam_state(trainer)[2] == 0                      # nothing was applied by the failed calls
    loss, grads, _ = ck.train_grads(trainer, x, y)
    _check(loss, grads, tc.reference("n3"), "after errors")

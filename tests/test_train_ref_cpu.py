"""The plain reference of the training step (tests/train_ref.py) held to things it shares no code with: the float64
forward evaluation the inference tests use, central differences of its own loss, torch.optim.Adam -- and the cases of
tests/train_cases.py shown to tell every listed mutant of a trainer from the truth.  CPU only."""
import numpy as np
import pytest
import torch

from tests import train_cases as tc
from tests import train_ref as tr


def test_forward_equals_the_float64_evaluation_of_the_inference_tests():
    """the same patches through tests/test_gpu_parity.py::_torch_fp64_classifier (what test_cnn_against_torch_fp64 compares
    the inference kernels with): 100 regions of a canonical image, seeded and trained weights"""
    from camkifu_amd.stone.nn_manager import NNManager
    from tests.test_gpu_parity import _torch_fp64_classifier
    X, Y, img = tc.board(900, 0.1)
    for W in (tc.weights(), NNManager.init_net()):
        want = _torch_fp64_classifier(W, img[None])[0]
        got = tr.forward(W, X)
        assert np.abs(got - want).max() <= 1e-12


def test_gradients_pass_a_central_difference_check():
    """three weights per tensor (the largest gradient and two seeded picks), n3: (L(w + h) - L(w - h)) / 2h in float64.
    h = 1e-6 of the tensor's scale keeps the truncation error (h^2 L''') far below the 1e-6 relative that is asked, and
    float64 rounding (1e-16 L / h) at 1e-9 of the gradient's scale."""
    x, y = tc.cases()["n3"]
    W = tc.weights()
    loss, g = tc.reference("n3")
    rng = np.random.default_rng(5)
    w = tr.tensors(W)
    with torch.no_grad():
        for k in tr.ORDER:
            flat, gk = w[k].reshape(-1), g[k].reshape(-1)
            scale = float(np.abs(gk).max())
            h = 1e-6 * float(W[k].std())
            for i in [int(np.abs(gk).argmax())] + [int(v) for v in rng.integers(0, gk.size, 2)]:
                keep = float(flat[i])
                flat[i] = keep + h
                up = float(tr.loss_of(w, x, y))
                flat[i] = keep - h
                down = float(tr.loss_of(w, x, y))
                flat[i] = keep
                assert abs((up - down) / (2 * h) - gk[i]) <= 1e-6 * scale, (k, i)
    assert abs(float(tr.loss_of(w, x, y)) - loss) <= 1e-14


def test_adam_equals_torch_over_three_steps():
    """Keras-1 puts eps beside sqrt(v) BEFORE the bias correction, torch.optim.Adam after it: w -= lr/bc1 m / (sqrt(v / bc2) + eps).
    The two are the same function when torch is given eps / sqrt(bc2_t) at step t, which its param_groups allow; with
    that the three steps agree to float64 rounding."""
    rng = np.random.default_rng(9)
    W = {k: rng.standard_normal(s) for k, s in (("a", (7, 5)), ("b", (11,)))}
    ref = tr.Adam(W)
    params = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in W.items()}
    opt = torch.optim.Adam(list(params.values()), lr=0.01, betas=(0.9, 0.999), eps=1e-8)
    for t in range(1, 4):
        g = {k: rng.standard_normal(v.shape) * 10.0 ** rng.integers(-6, 1, v.shape) for k, v in W.items()}
        g["b"][:3] = (0.0, 1e-12, -1e-12)
        for k in W:
            params[k].grad = torch.from_numpy(g[k].copy())
        opt.param_groups[0]["eps"] = 1e-8 / np.sqrt(1.0 - 0.999 ** t)
        opt.step()
        ref.apply(g, lr=0.01)
        for k in W:
            assert np.abs(ref.w[k] - params[k].detach().numpy()).max() <= 1e-14, (t, k)


@pytest.fixture(scope="module")
def separations():
    """per gradient mutant and case: the largest per-tensor distance between the mutated and the true reference"""
    out = {}
    for name in ("n1", "n3", "n65", "empty", "white", "ties"):
        x, y = tc.cases()[name]
        W = tc.weights_of(name)
        l_ref, g_ref = tc.reference(name)
        for mut in tr.GRAD_MUTANTS:
            if mut == "dropout_noscale":
                continue
            l, g = tr.loss_and_grads(W, x, y, mutant=mut)
            out[mut, name] = max(max(tr.grad_error(g, g_ref).values()), abs(l - l_ref) / abs(l_ref))
    return out


def test_the_cases_tell_the_mutants_apart(separations):
    """every gradient mutant is wrong by 1e-2 or more of some tensor's scale on at least one case -- a thousand times the
    tolerance of tests/test_gpu_train.py -- and the dropped patch shows on n65 alone among the small cases"""
    for mut in tr.GRAD_MUTANTS:
        if mut == "dropout_noscale":
            continue
        seen = {name: d for (m, name), d in separations.items() if m == mut}
        print(mut, {k: "%.1e" % v for k, v in seen.items()})
        assert max(seen.values()) >= 1e-2, (mut, seen)
    assert all(separations["drop_last", n] == 0 for n in ("n1", "n3", "empty", "white", "ties")) and separations["drop_last", "n65"] >= 1e-2
    assert separations["loss_sum", "n1"] == 0 and min(separations["loss_sum", n] for n in ("n3", "n65", "empty", "white")) >= 1
    # the tie rule shows on `ties` (and gradients sent to EVERY maximum on the flat patches of `empty`), nowhere else
    assert separations["pool_last", "ties"] >= 1e-2 and separations["pool_all", "ties"] >= 1e-2 and separations["pool_all", "empty"] >= 1e-2
    assert max(separations[m, n] for m in ("pool_last", "pool_all") for n in ("n1", "n3", "n65", "white")) <= 1e-12


def test_dropout_scale_and_adam_mutants_show():
    X, Y = tc.pool()
    x, y = X[:8], Y[:8]
    rng = np.random.default_rng(2)
    masks = [(rng.random((8,) + s) >= p).astype(np.uint8) for s, p in (((16, 16, 32), 0.25), ((6, 6, 90), 0.25), ((160,), 0.5))]
    l_ref, g_ref = tr.loss_and_grads(tc.weights(), x, y, masks=masks)
    l, g = tr.loss_and_grads(tc.weights(), x, y, masks=masks, mutant="dropout_noscale")
    assert max(tr.grad_error(g, g_ref).values()) >= 1e-2
    # dropout changes the gradients at all (the masks are applied)
    assert max(tr.grad_error(tr.loss_and_grads(tc.weights(), x, y)[1], g_ref).values()) >= 1e-2
    W = {k: v for k, v in tc.weights().items()}
    grads = {k: (rng.standard_normal(v.shape) * 1e-2).astype(np.float32) for k, v in W.items()}
    grads["d2b"][:4] = (0.0, 1e-12, -1e-12, 0.0)
    for mut in tr.ADAM_MUTANTS:
        a, b = tr.Adam(W, state=np.float32), tr.Adam(W, state=np.float32, mutant=mut)
        for _ in range(3):
            a.apply(grads)
            b.apply(grads)
        worst = max(float(tr.ulps(b.w[k], a.w[k]).max()) for k in tr.ORDER)
        assert worst > 100, (mut, worst)                              # against the 2 ulp of test_adam_alone

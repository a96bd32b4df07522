"""The host side of the harvest (camkifu_amd/stone/harvest.py, the dataset methods of NNManager, VManagerBase.snapshot,
tools/nn_runner.py --merge / --split / --histo) and the numpy reference tests/harvest_ref.py that the GPU tests compare the
kernels with.  No GPU."""
import importlib.util
import os
import types

import numpy as np
import pytest

from camkifu_amd.controller import ControllerHeadless
from camkifu_amd.golib_shim import Kifu, Move, NP_TYPE, B, W
from camkifu_amd.stone import harvest as hv
from camkifu_amd.stone import nn_manager as nm
from tests import harvest_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _runner():
    spec = importlib.util.spec_from_file_location("nn_runner_under_test", os.path.join(ROOT, "tools", "nn_runner.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _random_position(seed, density=0.4):
    rng = np.random.default_rng(seed)
    return (rng.random((19, 19)) < density) * rng.integers(1, 3, (19, 19)).astype(np.uint8)


# ---- the reference against the package's own cut and codec ------------------------------------------------------------
def test_reference_with_everything_eligible_is_generate_xs_and_ys():
    mgr = nm.NNManager()
    img = hr.hashed_bytes((380, 380, 3), salt=3)
    pos = _random_position(5)
    x, labels, src, found = hr.harvest_ref(img[None], np.zeros((1, 19, 19), np.int32), [0], pos[None])
    assert found == 100 and np.array_equal(src, np.stack([np.zeros(100, np.int32), np.arange(100, dtype=np.int32)], 1))
    assert np.array_equal(x, mgr.generate_xs(img))
    assert np.array_equal(labels, mgr.generate_ys(nm.SYMBOLS[pos]).argmax(1))
    assert hr.REGION_START == list(nm.REGION_START) and hr.PATCH_ORIGIN == list(nm.PATCH_ORIGIN)


def test_reference_hash_is_the_murmur_finaliser():
    assert hr.mix32(0) == 0 and hr.mix32(1) == 0x514e28b7 and hr.mix32(0xffffffff) == 0x81f16f39
    kept = [hr.mix(7, f, q) & 255 for f in range(40) for q in range(100)]
    assert 0.4 < np.mean(np.array(kept) < 128) < 0.6 and len(set(kept)) == 256


# ---- augmentation tables ---------------------------------------------------------------------------------------------------
def test_aug_label_against_brute_force():
    assert nm.AUG_LABEL.shape == (8, 81) and nm.AUG_LABEL.dtype == np.uint8
    for t in range(8):
        for label in range(81):
            block = nm.NNManager.compute_stones(label).reshape(2, 2)
            turned = np.rot90(block, t & 3)
            turned = turned[:, ::-1] if t & 4 else turned
            assert nm.AUG_LABEL[t, label] == nm.NNManager.compute_label(0, 2, 0, 2, turned), (t, label)
    inverse = [0, 3, 2, 1, 4, 5, 6, 7]                     # a quarter turn back; a turn followed by a mirror is a reflection
    for t in range(8):
        assert np.array_equal(nm.AUG_LABEL[inverse[t], nm.AUG_LABEL[t]], np.arange(81)), t
        x = hr.hashed_bytes((1, 40, 40, 3), salt=t)
        assert np.array_equal(hr.augment_ref(hr.augment_ref(x, [t]), [inverse[t]]), x)
    assert sorted(nm.AUG_LABEL[3]) == list(range(81)) and not np.array_equal(nm.AUG_LABEL[1], nm.AUG_LABEL[3])


def test_aug_label_moves_with_the_pixels():
    """a window turned by the reference shows the block AUG_LABEL names: one bright cell per stone"""
    for t in range(8):
        for label in (1, 3, 9, 27, 1 + 2 * 27, 2 + 9):
            x = np.zeros((1, 40, 40, 3), np.uint8)
            for k, d in enumerate(nm.DIGITS[label]):
                x[0, 20 * (k // 2):20 * (k // 2) + 20, 20 * (k % 2):20 * (k % 2) + 20] = d
            out = hr.augment_ref(x, [t])[0]
            digits = [int(out[20 * (k // 2) + 5, 20 * (k % 2) + 5, 0]) for k in range(4)]
            assert sum(d * 3 ** k for k, d in enumerate(digits)) == nm.AUG_LABEL[t, label]


def test_augment_codes():
    codes = nm.NNManager.augment_codes
    order = np.random.default_rng(1).permutation(4096)
    whole = codes(order, 11, 0, 4096)
    parts = np.concatenate([codes(order[a:b], 11, 0, 4096) for a, b in ((0, 1000), (1000, 1001), (1001, 4096))])
    assert np.array_equal(whole, parts) and whole.dtype == np.uint8
    assert np.array_equal(whole[np.argsort(order)], codes(np.arange(4096), 11, 0, 4096))
    assert sorted(set(whole.tolist())) == list(range(8))
    assert not np.array_equal(whole, codes(order, 11, 1, 4096)) and not np.array_equal(whole, codes(order, 12, 0, 4096))


# ---- the labelling rule ----------------------------------------------------------------------------------------------------
def _game():
    """S_0 .. S_3: B (3, 3), W (15, 15), B (3, 15)"""
    return hv.reference_positions([(B, 3, 3), (W, 15, 15), (B, 3, 15)])


def _calm(n):
    return np.zeros((n, 19, 19), np.int32)


def test_reference_positions():
    S = _game()
    assert S.shape == (4, 19, 19) and S.dtype == np.uint8 and not S[0].any()
    assert S[1][3, 3] == 1 and S[2][15, 15] == 2 and S[3][3, 15] == 1 and S[3].astype(bool).sum() == 3
    moves = [(W, 0, 0), (B, 0, 1), (B, 1, 0)]               # the second black stone takes the corner
    for rules in (False, True):
        ctrl = ControllerHeadless(rules=rules)
        S = hv.reference_positions(moves, rules=rules)
        for k, mv in enumerate(moves):
            ctrl.pipe("append", Move(NP_TYPE, mv))
            assert np.array_equal(S[k + 1], hv._codes(ctrl))
        assert S[3][0, 0] == (0 if rules else 2)
    kifu = Kifu()
    for mv in moves:
        kifu.append(Move(NP_TYPE, mv))
    assert np.array_equal(hv.reference_positions(kifu, rules=True), hv.reference_positions(moves, rules=True))


def test_the_empty_start_never_opens():
    S = _game()
    assert (hv.label_windows(np.repeat(S[:1], 6, 0), _calm(6), S) == -1).all()


def test_a_window_opens_on_the_reporting_frame_and_closes_on_agitation():
    S = _game()
    found = np.stack([S[0], S[0], S[1], S[1], S[1], S[1], S[1], S[1]])
    fg = _calm(8)
    fg[3, 2, 2] = 200                                         # exactly the threshold: still calm
    fg[5, 10, 4] = 201
    assert hv.label_windows(found, fg, S).tolist() == [-1, -1, 1, 1, 1, -1, -1, -1]
    fg[2, 18, 18] = 500                                       # the reporting frame itself is agitated: the window never opens
    assert hv.label_windows(found, fg, S).tolist() == [-1] * 8
    found = np.stack([S[1], S[1], S[2], S[2]])                # the next report opens the next window
    fg = _calm(4)
    fg[1, 0, 0] = 300
    assert hv.label_windows(found, fg, S).tolist() == [1, -1, 2, 2]


def test_a_missed_move_opens_nothing_afterwards():
    S = _game()
    skipped = S[1].copy()
    skipped[3, 15] = 1                                        # the finder never saw the white stone
    found = np.stack([S[1], S[1], skipped, skipped, skipped])
    assert hv.label_windows(found, _calm(5), S).tolist() == [1, 1, -1, -1, -1]


def test_a_wrong_reference_move_is_a_missed_one():
    S = _game()
    wrong = hv.reference_positions([(B, 3, 3), (W, 15, 14), (B, 3, 15)])
    found = np.stack([S[1], S[2], S[2], S[3], S[3]])          # the finder follows the game that was played
    assert hv.label_windows(found, _calm(5), wrong).tolist() == [1, -1, -1, -1, -1]


def test_a_match_is_searched_forward_only():
    S = _game()
    loop = np.stack([S[0], S[1], S[2], S[1]])                 # a position that comes back (a stone taken off again)
    assert hv.label_windows(np.stack([S[1], S[2], S[1], S[1]]), _calm(4), loop).tolist() == [1, 2, 3, 3]
    assert hv.label_windows(np.stack([S[2], S[1]]), _calm(2), loop).tolist() == [2, 3]
    assert hv.label_windows(np.stack([S[2], S[1], S[2]]), _calm(3), S).tolist() == [2, -1, 2]
    assert hv.label_windows(np.stack([S[2], S[2], S[0]]), _calm(3), S).tolist() == [2, 2, -1]


def test_state_carries_over_a_batch_boundary():
    S = _game()
    found = np.stack([S[0], S[1], S[1], S[1], S[1], S[2], S[2], S[1], S[3]])
    fg = _calm(9)
    fg[2, 5, 5] = 999
    whole = hv.label_windows(found, fg, S)
    assert whole.tolist() == [-1, 1, -1, -1, -1, 2, 2, -1, 3]
    for cut in range(1, 9):
        state = hv.new_window_state()
        parts = [hv.label_windows(found[a:b], fg[a:b], S, state=state) for a, b in ((0, cut), (cut, 9))]
        assert np.concatenate(parts).tolist() == whole.tolist(), cut


# ---- snapshots -------------------------------------------------------------------------------------------------------------
def test_gen_data_from_a_snapshot(tmp_path):
    mgr = nm.NNManager()
    img = hr.hashed_bytes((380, 380, 3), salt=9)
    moves = [(W, 0, 0), (B, 0, 1), (B, 1, 0), (W, 17, 17), (B, 18, 18)]
    kifu = Kifu()
    for mv in moves:
        kifu.append(Move(NP_TYPE, mv))
    np.save(tmp_path / "snapshot-0.npy", img)
    kifu.save(str(tmp_path / "game-0.sgf"))
    path = str(tmp_path / "snapshot-0.npy")
    assert nm.NNManager.get_ref_game(path) == str(tmp_path / "game-0.sgf")
    assert nm.NNManager.get_ref_y(path) == str(tmp_path / "snapshot-0-y.npz")
    stones = nm.SYMBOLS[hv.reference_positions(moves, rules=True)[-1]]
    assert stones[0, 0] == "E" and stones[18, 18] == B
    x, y = mgr.gen_data(path)
    assert mgr.stones_source == "sgf"
    assert np.array_equal(x, mgr.generate_xs(img)) and np.array_equal(y, mgr.generate_ys(stones))
    # a copy of the snapshot falls back on the game of the original
    np.save(tmp_path / "snapshot-0 (2).npy", img)
    assert np.array_equal(mgr.gen_data(str(tmp_path / "snapshot-0 (2).npy"))[1], y)
    # saved labels
    np.save(tmp_path / "snapshot-1.npy", img)
    np.savez(tmp_path / "snapshot-1-y.npz", Y=y)
    x1, y1 = mgr.gen_data(str(tmp_path / "snapshot-1.npy"))
    assert mgr.stones_source == "y" and np.array_equal(y1, y) and np.array_equal(x1, x)
    said = []
    assert mgr.gen_data(str(tmp_path / "snapshot-1.npy"), validate=lambda s, i: said.append(s.shape) or False) == (None, None)
    assert said == [(19, 19)]

    def edit(stones, image):
        stones[9, 9] = W
        return True
    assert mgr.gen_data(str(tmp_path / "snapshot-1.npy"), validate=edit)[1][44].argmax() == 2 * 27      # region (4, 4): rows 8-9
    # neither a game nor labels: a guess is not accepted without somebody to validate it
    np.save(tmp_path / "snapshot-2.npy", img)
    assert mgr.gen_data(str(tmp_path / "snapshot-2.npy")) == (None, None)
    with pytest.raises(ValueError):
        mgr.gen_data(str(tmp_path / "snapshot-2.png"))
    np.save(tmp_path / "snapshot-3.npy", img[:100])
    with pytest.raises(ValueError):
        mgr.gen_data(str(tmp_path / "snapshot-3.npy"))


def test_snapshot_numbering(tmp_path, monkeypatch):
    from camkifu_amd import cvconf
    from camkifu_amd.core.vmanager import VManagerBase
    monkeypatch.setattr(cvconf, "snapshot_dir", str(tmp_path))
    ctrl = ControllerHeadless()
    ctrl.pipe("append", Move(NP_TYPE, (B, 3, 3)))
    vm = VManagerBase(ctrl, bf="None", sf="None")
    assert vm.snapshot(True) is None                          # no stones finder, no image
    img = hr.hashed_bytes((380, 380, 3), salt=1)
    vm.stones_finder = types.SimpleNamespace(goban_img=img)
    assert vm.snapshot(True) == str(tmp_path / "snapshot-0.npy")
    assert vm.snapshot(False) == str(tmp_path / "snapshot-1.npy")
    assert np.array_equal(np.load(tmp_path / "snapshot-0.npy"), img)
    assert Kifu(str(tmp_path / "game-0.sgf")).moves == [Move(NP_TYPE, (B, 3, 3))] and not (tmp_path / "game-1.sgf").exists()
    np.save(tmp_path / "snapshot-7.npy", img)
    (tmp_path / "snapshot-9.txt").write_text("not a snapshot")
    vm.stones_finder.goban_img = img[None]                    # a batch of one, as the warp returns it
    assert vm.snapshot(True) == str(tmp_path / "snapshot-8.npy") and (tmp_path / "game-8.sgf").exists()
    assert np.load(tmp_path / "snapshot-8.npy").shape == (380, 380, 3)
    x, y = nm.NNManager().gen_data(str(tmp_path / "snapshot-8.npy"))
    assert y[11].argmax() == 27 and y.argmax(1).astype(bool).sum() == 1          # (3, 3) is the last point of region (1, 1)


# ---- tools/nn_runner.py ----------------------------------------------------------------------------------------------------
def _tiny_set(n, seed):
    rng = np.random.default_rng(seed)
    y = np.zeros((n, 81), bool)
    y[np.arange(n), rng.integers(0, 81, n)] = True
    return hr.hashed_bytes((n, 40, 40, 3), salt=seed), y


def test_nn_runner_merge_split_histo(tmp_path, capsys):
    run = _runner()
    (xa, ya), (xb, yb) = _tiny_set(7, 1), _tiny_set(13, 2)
    ya[:] = False
    ya[:, 0] = True                                           # seven empty regions
    yb[:3] = False
    yb[0, 1] = yb[1, 3 + 2 * 9] = yb[2, 80] = True            # one stone, two stones, four stones
    np.savez(tmp_path / "a.npz", X=xa, Y=ya)
    np.savez(tmp_path / "b.npz", X=xb, Y=yb)
    out = str(tmp_path / "all.npz")
    assert run.main(["--merge", str(tmp_path / "a.npz"), str(tmp_path / "b.npz"), "--out", out]) == 0
    X, Y = run.load_set(out)
    assert np.array_equal(X, np.concatenate([xa, xb])) and np.array_equal(Y, np.concatenate([ya, yb]))
    assert run.main(["--split", "0.8", out]) == 0
    (Xt, Yt), (Xe, Ye) = run.load_set(str(tmp_path / "all-train.npz")), run.load_set(str(tmp_path / "all-test.npz"))
    assert len(Xt) == 16 and len(Xe) == 4
    key = lambda x, y: sorted((a.tobytes(), int(b.argmax())) for a, b in zip(x, y))      # noqa: E731
    assert key(np.concatenate([Xt, Xe]), np.concatenate([Yt, Ye])) == key(X, Y)           # every sample once, with its own label
    again = run.split_data(X, Y, 0.8)
    assert np.array_equal(again[0], Xt) and np.array_equal(again[3], Ye)                  # seeded
    assert not np.array_equal(run.split_data(X, Y, 0.8, seed=5)[0], Xt)
    per_label, per_stones = run.histo(Y)
    assert per_label.sum() == 20 and per_label[0] >= 7 and per_stones.sum() == 20
    digits = nm.DIGITS[Y.argmax(1)]
    assert per_stones.tolist() == [int(((digits > 0).sum(1) == k).sum()) for k in range(5)]
    capsys.readouterr()
    assert run.main(["--histo", out]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].split() == ["empty", str(per_stones[0])] and lines[4].split() == ["four", "stones", str(per_stones[4])]

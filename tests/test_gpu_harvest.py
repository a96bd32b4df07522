"""Labelled patches on the GPU (camkifu_amd/csrc/k_harvest.hip through ck_harvest_patches / ck_augment_patches, the
Harvester of camkifu_amd/stone/harvest.py, NNManager.train(augment=True)) against the numpy restatement
tests/harvest_ref.py, bit for bit.  The goban bytes are a hash of their own index, not a rendered board, so any slip in an
address shows.

Mutants of the kernels that must each fail this file, and the tests that see them:
    last origin 360 instead of 340               test_one_frame_all_kept (regions of row / column 9; reads past the image)
    digits of the label column-major             every test with stones: test_one_frame_all_kept first (labels (0,1) != (1,0))
    calm gate over one zone instead of four      test_calm_gate (zones of 9 and 8 in one region: 17 > 16, neither alone)
    `<` for `<=` in the calm gate                test_calm_gate (a zone at exactly calm_max keeps its regions)
    scan off by one at a wave / block boundary   test_three_frames_middle_one_out (waves: 100 kept, 100 not, 100 kept),
                                                 test_past_one_block (1100 and 2300 candidates: blocks of 1024)
    region-major output order                    test_three_frames_middle_one_out, test_past_one_block (src ascending by frame)
    thinning keyed on the output index           test_empty_keep (the kept set is the Python hash of (frame, region); a call
                                                 that starts two frames later keeps the same regions of the same frames)
The end-to-end figures -- the eligible frames, the states and the 1700 patches -- come from a run of the same film through
the CPU oracle's pipeline, not from the code under test."""
import ctypes as C

import numpy as np
import pytest

from tests import harvest_ref as hr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from camkifu_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def _positions(n_pos, seed, density=0.45):
    rng = np.random.default_rng(seed)
    return ((rng.random((n_pos, 19, 19)) < density) * rng.integers(1, 3, (n_pos, 19, 19))).astype(np.uint8)


def _same(got, ref):
    x, labels, src = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in got)
    rx, rl, rs, found = ref
    assert x.shape == rx.shape and x.dtype == np.uint8 and labels.dtype == np.uint8 and src.dtype == np.int32
    assert np.array_equal(src, rs) and np.array_equal(labels, rl) and np.array_equal(x, rx)
    return found


def _arg_error(call):
    from camkifu_amd import capi
    with pytest.raises(capi.CkError) as info:
        call()
    assert info.value.code == capi.CK_ERR_ARG, info.value


# ---- ck_harvest_patches ----------------------------------------------------------------------------------------------------
def test_one_frame_all_kept(ck):
    from camkifu_amd.stone import nn_manager as nm
    goban, pos = hr.hashed_bytes((1, 380, 380, 3), salt=1), _positions(1, 1)
    fg = np.zeros((1, 19, 19), np.int32)
    got = ck.harvest_patches(goban, fg, [0], pos)
    assert _same(got, hr.harvest_ref(goban, fg, [0], pos)) == 100 == ck.harvest_found
    mgr = nm.NNManager()
    assert np.array_equal(got[0], mgr.generate_xs(goban[0]))
    assert np.array_equal(got[1], mgr.generate_ys(nm.SYMBOLS[pos[0]]).argmax(1))
    assert np.array_equal(got[0][99], goban[0, 340:380, 340:380]) and np.array_equal(got[0][89], goban[0, 320:360, 340:380])
    single = ck.harvest_patches(goban[0], fg, [0], pos)        # one image without the batch axis
    assert np.array_equal(single[0], got[0])


def test_three_frames_middle_one_out(ck):
    goban, pos = hr.hashed_bytes((3, 380, 380, 3), salt=2), _positions(2, 2)
    fg = np.zeros((3, 19, 19), np.int32)
    got = ck.harvest_patches(goban, fg, [0, -1, 1], pos)
    assert _same(got, hr.harvest_ref(goban, fg, [0, -1, 1], pos)) == 200
    assert got[2][:, 0].tolist() == [0] * 100 + [2] * 100 and got[2][:, 1].tolist() == list(range(100)) * 2
    assert np.array_equal(got[0][100], goban[2, :40, :40])


@pytest.mark.parametrize("n, empty_keep", [(11, 256), (11, 100), (23, 256), (23, 60)])
def test_past_one_block(ck, n, empty_keep):
    goban, pos = hr.hashed_bytes((n, 380, 380, 3), salt=n), _positions(4, n, density=0.15)
    rng = np.random.default_rng(n)
    fg = (rng.random((n, 19, 19)) < 0.02) * rng.integers(1, 40, (n, 19, 19)).astype(np.int32)
    state = np.arange(n) % 4 if empty_keep == 256 else rng.integers(-1, 4, n)
    if empty_keep == 256:
        fg[:] = 0
    ref = hr.harvest_ref(goban, fg, state, pos, empty_keep=empty_keep, seed=n, first_frame=1000)
    got = ck.harvest_patches(goban, fg, state, pos, empty_keep=empty_keep, seed=n, first_frame=1000)
    found = _same(got, ref)
    assert found == ck.harvest_found and (found == n * 100 if empty_keep == 256 else 100 < found < n * 100)
    key = got[2][:, 0].astype(np.int64) * 100 + got[2][:, 1]
    assert (np.diff(key) > 0).all()


def test_calm_gate(ck):
    goban, pos = hr.hashed_bytes((1, 380, 380, 3), salt=4), _positions(1, 4)
    for calm_max in (16, 0, 5):
        for row, gone in ((17, {82, 92}), (18, {92}), (16, {82}), (0, {2})):
            fg = np.zeros((1, 19, 19), np.int32)
            fg[0, row, 5] = calm_max                              # exactly the bound: everything stays
            got = ck.harvest_patches(goban, fg, [0], pos, calm_max=calm_max)
            assert _same(got, hr.harvest_ref(goban, fg, [0], pos, calm_max=calm_max)) == 100
            fg[0, row, 5] = calm_max + 1                          # column 5 lies in region column 2 alone
            got = ck.harvest_patches(goban, fg, [0], pos, calm_max=calm_max)
            assert _same(got, hr.harvest_ref(goban, fg, [0], pos, calm_max=calm_max)) == 100 - len(gone)
            assert set(range(100)) - set(got[2][:, 1].tolist()) == gone, (calm_max, row)
    fg = np.zeros((1, 19, 19), np.int32)
    fg[0, 6, 8] = fg[0, 7, 9] = 8                                 # two zones of region (3, 4): 16 together
    assert len(ck.harvest_patches(goban, fg, [0], pos)[1]) == 100
    fg[0, 6, 8] = 9                                               # 17 together, neither above 16
    got = ck.harvest_patches(goban, fg, [0], pos)
    assert _same(got, hr.harvest_ref(goban, fg, [0], pos)) == 99 and 34 not in got[2][:, 1].tolist()
    fg[0, 6, 8] = 2 ** 31 - 1                                     # the sum does not wrap
    fg[0, 7, 9] = 2 ** 31 - 1
    assert _same(ck.harvest_patches(goban, fg, [0], pos), hr.harvest_ref(goban, fg, [0], pos)) == 99


def test_empty_keep(ck):
    n = 5
    goban, pos = hr.hashed_bytes((n, 380, 380, 3), salt=5), _positions(2, 5, density=0.1)
    fg, state = np.zeros((n, 19, 19), np.int32), [0, 1, 0, 1, 1]
    full = sum(int(hr.region_label(pos[s], q // 10, q % 10) != 0) for s in state for q in range(100))
    kept = {}
    for empty_keep, first_frame in ((0, 0), (128, 0), (256, 0), (128, 7), (128, 2 ** 32 + 7), (128, 2 ** 40)):
        got = ck.harvest_patches(goban, fg, state, pos, empty_keep=empty_keep, seed=77, first_frame=first_frame)
        found = _same(got, hr.harvest_ref(goban, fg, state, pos, empty_keep=empty_keep, seed=77, first_frame=first_frame))
        kept[empty_keep, first_frame] = {(int(i), int(q)) for i, q in got[2]}
        if empty_keep == 0:
            assert found == full and (got[1] > 0).all()
        if empty_keep == 256:
            assert found == n * 100
    assert full < len(kept[128, 0]) < n * 100 and kept[128, 0] != kept[128, 7] and len(kept[128, 7]) > full
    assert kept[128, 7] == kept[128, 2 ** 32 + 7]                 # the frame number counts modulo 2^32
    assert kept[128, 0] != {tuple(pair) for pair in ck.harvest_patches(goban, fg, state, pos, empty_keep=128, seed=78)[2].tolist()}
    # the hash is of the FRAME, not of the place in the call or in the output: the tail of the film, harvested on its own
    tail = ck.harvest_patches(goban[2:], fg[2:], state[2:], pos, empty_keep=128, seed=77, first_frame=2)
    assert {(int(i) + 2, int(q)) for i, q in tail[2]} == {p for p in kept[128, 0] if p[0] >= 2}


def _raw_harvest(ck, goban_ptr, space, fg, state, pos, x_ptr, lab_ptr, src_ptr, cap, out_space):
    from camkifu_amd import capi
    state, fg = np.ascontiguousarray(state, np.int32), np.ascontiguousarray(fg, np.int32)
    found = C.c_int32(-5)
    rc = capi.lib().ck_harvest_patches(ck._h, goban_ptr, len(state), space, fg.ctypes.data_as(C.c_void_p), capi.CK_HOST,
                                       state.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), len(pos), 16, 256, 0, 0,
                                       x_ptr, lab_ptr, src_ptr, cap, out_space, C.byref(found))
    return rc, found.value


def test_cap_below_found(ck):
    import torch
    from camkifu_amd import capi
    goban, pos = hr.hashed_bytes((3, 380, 380, 3), salt=6), _positions(1, 6)
    fg, state = np.zeros((3, 19, 19), np.int32), [0, 0, 0]
    ref = hr.harvest_ref(goban, fg, state, pos, cap=130)
    assert ref[3] == 300
    got = ck.harvest_patches(goban, fg, state, pos, cap=130)
    assert _same(got, ref) == 300 == ck.harvest_found and len(got[0]) == 130
    assert len(ck.harvest_patches(goban, fg, state, pos, cap=0)[0]) == 0 and ck.harvest_found == 300
    # nothing is written beyond cap: buffers with room for more, filled with a sentinel -- on the host and in HBM
    x, lab, src = np.full((140, 40, 40, 3), 0xA5, np.uint8), np.full(140, 0xA5, np.uint8), np.full((140, 2), -7, np.int32)
    rc, found = _raw_harvest(ck, goban.ctypes.data_as(C.c_void_p), capi.CK_HOST, fg, state, pos, x.ctypes.data_as(C.c_void_p),
                             lab.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), 130, capi.CK_HOST)
    assert (rc, found) == (0, 300)
    assert np.array_equal(x[:130], ref[0]) and np.array_equal(lab[:130], ref[1]) and np.array_equal(src[:130], ref[2])
    assert (x[130:] == 0xA5).all() and (lab[130:] == 0xA5).all() and (src[130:] == -7).all()
    dev = torch.device("cuda", 0)
    tx, tl, ts = torch.from_numpy(x).to(dev).fill_(0xA5), torch.from_numpy(lab).to(dev).fill_(0xA5), torch.from_numpy(src).to(dev).fill_(-7)
    tg = torch.from_numpy(goban).to(dev)
    torch.cuda.synchronize()
    rc, found = _raw_harvest(ck, C.c_void_p(tg.data_ptr()), capi.CK_DEVICE, fg, state, pos, C.c_void_p(tx.data_ptr()),
                             C.c_void_p(tl.data_ptr()), C.c_void_p(ts.data_ptr()), 130, capi.CK_DEVICE)
    assert (rc, found) == (0, 300)
    x, lab, src = tx.cpu().numpy(), tl.cpu().numpy(), ts.cpu().numpy()
    assert np.array_equal(x[:130], ref[0]) and np.array_equal(lab[:130], ref[1]) and np.array_equal(src[:130], ref[2])
    assert (x[130:] == 0xA5).all() and (lab[130:] == 0xA5).all() and (src[130:] == -7).all()
    # fewer found than cap: the rows beyond them stay too
    x[:] = 0xA5
    rc, found = _raw_harvest(ck, goban.ctypes.data_as(C.c_void_p), capi.CK_HOST, fg, [-1, 0, -1], pos, x.ctypes.data_as(C.c_void_p),
                             lab.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), 140, capi.CK_HOST)
    assert (rc, found) == (0, 100) and np.array_equal(x[:100], hr.harvest_ref(goban[1:2], fg[:1], [0], pos)[0]) and (x[100:] == 0xA5).all()


def test_nothing_eligible_and_no_frames(ck):
    goban, pos = hr.hashed_bytes((2, 380, 380, 3), salt=7), _positions(1, 7)
    fg = np.zeros((2, 19, 19), np.int32)
    x, labels, src = ck.harvest_patches(goban, fg, [-1, -1], pos)
    assert ck.harvest_found == 0 and x.shape == (0, 40, 40, 3) and labels.shape == (0,) and src.shape == (0, 2)
    x, labels, src = ck.harvest_patches(goban, fg, [-1, -3], np.zeros((0, 19, 19), np.uint8))        # no position at all
    assert ck.harvest_found == 0 and len(x) == 0
    x, labels, src = ck.harvest_patches(goban[:0], fg[:0], [], pos)
    assert ck.harvest_found == 0 and x.shape == (0, 40, 40, 3)


def test_inputs_on_host_and_device(ck):
    import torch
    goban, pos = hr.hashed_bytes((4, 380, 380, 3), salt=8), _positions(3, 8)
    rng = np.random.default_rng(8)
    fg = (rng.random((4, 19, 19)) < 0.05) * rng.integers(1, 60, (4, 19, 19)).astype(np.int32)
    state = [2, 0, -1, 1]
    ref = hr.harvest_ref(goban, fg, state, pos, empty_keep=200, seed=3, first_frame=40)
    dev = torch.device("cuda", 0)
    tg, tf = torch.from_numpy(goban).to(dev), torch.from_numpy(fg).to(dev)
    for g, f in ((goban, fg), (tg, fg), (tg, tf), (goban, tf), (tg[1:], fg[1:])):
        got = ck.harvest_patches(g, f, state[-len(g):], pos, empty_keep=200, seed=3, first_frame=40 + 4 - len(g))
        assert all(hasattr(a, "is_cuda") and a.is_cuda for a in got) == hasattr(g, "is_cuda")
        if len(g) == 4:
            _same(got, ref)
        else:
            keep = ref[2][:, 0] >= 1
            _same(got, (ref[0][keep], ref[1][keep], ref[2][keep] - [1, 0], None))


def test_bad_arguments_are_refused_before_any_launch(ck):
    goban, pos = hr.hashed_bytes((2, 380, 380, 3), salt=9), _positions(2, 9)
    fg = np.zeros((2, 19, 19), np.int32)
    bad = pos.copy()
    bad[1, 18, 18] = 3
    _arg_error(lambda: ck.harvest_patches(goban, fg, [0, 0], bad))               # also when no frame points at that position
    _arg_error(lambda: ck.harvest_patches(goban, fg, [0, 2], pos))
    _arg_error(lambda: ck.harvest_patches(goban, fg, [0, 0], pos[:0]))
    _arg_error(lambda: ck.harvest_patches(goban, fg, [0, 1], pos, empty_keep=-1))
    _arg_error(lambda: ck.harvest_patches(goban, fg, [0, 1], pos, empty_keep=257))
    _arg_error(lambda: ck.harvest_patches(goban, fg, [0, 1], pos, cap=-1))
    _arg_error(lambda: ck.augment_patches(hr.hashed_bytes((3, 40, 40, 3)), [0, 8, 1]))
    with pytest.raises(ValueError):
        ck.harvest_patches(goban, fg, [0], pos)
    with pytest.raises(ValueError):
        ck.harvest_patches(goban[:, :379], fg, [0, 1], pos)
    assert _same(ck.harvest_patches(goban, fg, [0, 1], pos), hr.harvest_ref(goban, fg, [0, 1], pos)) == 200      # still works


# ---- ck_augment_patches ----------------------------------------------------------------------------------------------------
def test_augment_against_numpy(ck):
    import torch
    x = hr.hashed_bytes((17, 40, 40, 3), salt=10)
    t = (np.arange(17) * 3) % 8
    assert sorted(set(t.tolist())) == list(range(8))
    ref = hr.augment_ref(x, t)
    out = ck.augment_patches(x, t)
    assert isinstance(out, np.ndarray) and np.array_equal(out, ref)
    dev = torch.device("cuda", 0)
    tx = torch.from_numpy(x).to(dev)
    out = ck.augment_patches(tx, t)
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), ref)
    out = ck.augment_patches(x, t, to_device=dev)
    assert out.is_cuda and np.array_equal(out.cpu().numpy(), ref)
    into = np.zeros_like(x)
    assert ck.augment_patches(tx, t, out=into) is into and np.array_equal(into, ref)
    into = torch.zeros_like(tx)
    assert ck.augment_patches(tx, t, out=into) is into and np.array_equal(into.cpu().numpy(), ref)
    assert np.array_equal(ck.augment_patches(x[:1], [6]), hr.augment_ref(x[:1], [6]))
    assert ck.augment_patches(x[:0], []).shape == (0, 40, 40, 3)


def test_augment_refuses_to_work_in_place(ck):
    import torch
    x = hr.hashed_bytes((18, 40, 40, 3), salt=11)
    t = np.arange(17) % 8
    before = x.copy()
    _arg_error(lambda: ck.augment_patches(x[:17], t, out=x[:17]))
    _arg_error(lambda: ck.augment_patches(x[:17], t, out=x[1:]))                  # overlapping, not identical
    tx = torch.from_numpy(x).to(torch.device("cuda", 0))
    _arg_error(lambda: ck.augment_patches(tx[:17], t, out=tx[:17]))
    _arg_error(lambda: ck.augment_patches(tx[1:], t, out=tx[:17]))
    assert np.array_equal(x, before) and np.array_equal(tx.cpu().numpy(), before)
    assert np.array_equal(ck.augment_patches(tx[:9], t[:9], out=tx[9:]).cpu().numpy(), hr.augment_ref(before[:9], t[:9]))


# ---- end to end: a filmed game and its record -> a dataset ---------------------------------------------------------------------
ELIGIBLE = [6, 7] + list(range(31, 38)) + list(range(61, 68)) + [97]             # from the CPU oracle's run of this film
STATES = [67] * 2 + [68] * 7 + [69] * 7 + [70]
PATCHES = 1700


@pytest.fixture(scope="module")
def film():
    from camkifu_amd import synth
    frames, corners, truth, moves, _hands = synth.film(100, 480, 640, seed=8, quiet=8, move_every=30, hand_frames=12)
    sym = "EBW"
    first = [(sym[truth[6][r, c]], r, c) for r in range(19) for c in range(19) if truth[6][r, c]]
    played = [(sym[col], r, c) for col, r, c, f in moves]
    return frames.numpy(), truth, first + played, len(first)


def _harvest_film(ck, frames, game, **kw):
    """the calls of test_fast_file_pipeline_on_gpu: the first 8 frames find the board, then the film in batches of 23.
    -> (harvester, dataset with `frame` as the film's frame number)"""
    from camkifu_amd.stone.harvest import Harvester
    from camkifu_amd.stone.nn_manager import NNManager
    ck.cnn_set_weights(NNManager.init_net())
    hv = Harvester(480, 640, game, ctx=ck, bg_init_frames=6, **kw)
    try:
        hv.feed(frames[:8])
        assert len(hv.dataset()["X"]) == 0 and hv.eligible == []
        for b0 in range(0, 100, 23):
            hv.feed(frames[b0:b0 + 23])
    finally:
        hv.close()
    data = hv.dataset()
    data["frame"] = data["frame"] - 8
    return hv, data


def test_film_to_dataset(ck, film):
    from camkifu_amd.stone import nn_manager as nm
    frames, truth, game, n_first = film
    hv, data = _harvest_film(ck, frames, game)
    assert [(f - 8, k) for f, k in hv.eligible] == list(zip(ELIGIBLE, STATES))
    assert sorted(set(data["state"].tolist())) == [67, 68, 69, 70]
    assert data["X"].shape == (PATCHES, 40, 40, 3) and data["Y"].shape == (PATCHES, 81) and data["Y"].dtype == bool
    assert sorted(set(data["frame"].tolist())) == ELIGIBLE and (data["Y"].sum(1) == 1).all()
    mgr = nm.NNManager()
    wrong = differ = 0
    for f in ELIGIBLE:
        mine = np.flatnonzero(data["frame"] == f)
        labels = mgr.generate_ys(nm.SYMBOLS[truth[f]]).argmax(1)
        wrong += int((data["Y"][mine].argmax(1) != labels[data["region"][mine]]).sum())
        goban = np.asarray(ck.warp_perspective(frames[f], hv.pipe.board.mtx)).reshape(380, 380, 3)
        differ += int(sum(not np.array_equal(data["X"][k], mgr.generate_xs(goban)[data["region"][k]]) for k in mine))
    print("patches %d, non-empty %d, mislabelled %d, pixels differ in %d" % (len(data["X"]), int((data["Y"].argmax(1) > 0).sum()), wrong, differ))
    assert wrong == 0 and differ == 0


def test_film_with_a_wrong_record_stops_there(ck, film):
    frames, truth, game, n_first = film
    game = list(game)
    colour, r, c = game[n_first + 1]                          # the second move that was played, one point aside
    game[n_first + 1] = (colour, r, c + 1 if c < 18 else c - 1)
    hv, data = _harvest_film(ck, frames, game)
    assert [f - 8 for f, k in hv.eligible] == [f for f in ELIGIBLE if f <= 37] and int(data["frame"].max()) == 37


def test_film_one_frame_per_state(ck, film):
    frames, truth, game, n_first = film
    hv, data = _harvest_film(ck, frames, game, per_state=1)
    assert sorted(set(data["frame"].tolist())) == [6, 31, 61, 97] and sorted(set(data["state"].tolist())) == [67, 68, 69, 70]
    assert len(hv.eligible) == len(ELIGIBLE)


def test_a_y4m_file_through_run_and_the_command_line(ck, film, tmp_path):
    """Harvester.run on a .y4m file is feed() on the frames process_y4m selects and decodes, batch by batch, and
    `nn_runner --harvest` writes that dataset; whatever is harvested carries the label of its frame"""
    import importlib.util
    import os
    from camkifu_amd import synth
    from camkifu_amd.core import capture as cap
    from camkifu_amd.golib_shim import Kifu, Move, NP_TYPE
    from camkifu_amd.stone import nn_manager as nm
    from camkifu_amd.stone.harvest import Harvester
    frames, truth, game, n_first = film
    path, sgf = str(tmp_path / "game.y4m"), str(tmp_path / "game.sgf")
    i420 = [synth.bgr_to_i420(f) for f in frames]
    cap.write_y4m(path, (i420[k // 2] for k in range(200)), 480, 640, fps=(5, 1))       # read at 5 fps: frames 1, 3, 5, ...
    kifu = Kifu()
    for mv in game:
        kifu.append(Move(NP_TYPE, mv))
    kifu.save(sgf)
    ck.cnn_set_weights(nm.NNManager.init_net())
    hv = Harvester(480, 640, sgf, ctx=ck, bg_init_frames=6)
    try:
        data = hv.run(path, batch=23)
    finally:
        hv.close()
    by_hand = Harvester(480, 640, game, ctx=ck, bg_init_frames=6)
    try:
        decoded = np.asarray(ck.i420_to_bgr(np.stack(i420), 480, 640))
        for b0 in range(0, 100, 23):
            by_hand.feed(decoded[b0:b0 + 23])
    finally:
        by_hand.close()
    assert hv.frames_seen == 100 and hv.eligible == by_hand.eligible
    want = by_hand.dataset()
    for key in ("X", "Y", "frame", "region", "state"):
        assert np.array_equal(data[key], want[key]), key
    mgr = nm.NNManager()
    for f in sorted(set(data["frame"].tolist())):
        mine = data["frame"] == f
        labels = mgr.generate_ys(nm.SYMBOLS[truth[f]]).argmax(1)
        assert np.array_equal(data["Y"][mine].argmax(1), labels[data["region"][mine]]), f
    print("y4m: %d patches of frames %s" % (len(data["X"]), sorted(set(data["frame"].tolist()))))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("nn_runner_on_gpu", os.path.join(root, "tools", "nn_runner.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    out = str(tmp_path / "data.npz")
    assert run.main(["--harvest", path, "--sgf", sgf, "--out", out, "--per-state", "2", "--batch", "50"]) == 0
    limited = Harvester(480, 640, sgf, ctx=ck, bg_init_frames=50, per_state=2, seed=synth.SEED)
    try:
        want = limited.run(path, batch=50)
    finally:
        limited.close()
    with np.load(out) as z:
        assert sorted(z.files) == ["X", "Y", "frame", "region", "state"]
        for key in z.files:
            assert np.array_equal(z[key], want[key]), key


def test_keep_gobans_is_one_rank_only(ck):
    from camkifu_amd import pipeline
    from camkifu_amd.controller import ControllerHeadless
    with pytest.raises(ValueError):
        pipeline.FastFilePipeline(480, 640, ControllerHeadless(), ctx=ck, world=2, keep_gobans=True)


# ---- NNManager.train(augment=True) ---------------------------------------------------------------------------------------
def test_train_with_augmentation_is_the_hand_driven_loop(ck):
    from camkifu_amd.stone import nn_manager as nm
    x = hr.hashed_bytes((64, 40, 40, 3), salt=12)
    labels = (np.arange(64) * 7 % 81).astype(np.uint8)
    seed, net = 5, nm.NNManager.create_net()
    mgr = nm.NNManager()
    mgr.ctx = ck
    kept = nm.NNManager._network

    def fit(augment):
        mgr.train(x, labels, batch_size=32, nb_epoch=2, seed=seed, net=net, verbose=False, augment=augment)
        return nm.NNManager._network
    try:
        first, second, plain = fit(True), fit(True), fit(False)
    finally:
        nm.NNManager._network = kept
    handle = ck.train_create(net)
    try:
        for epoch in range(2):
            order = mgr.epoch_order(64, seed, epoch)
            for k in range(0, 64, 32):
                idx = order[k:k + 32]
                t = mgr.augment_codes(idx, seed, epoch, 64)
                ck.train_step(handle, hr.augment_ref(x[idx], t), nm.AUG_LABEL[t, labels[idx]], lr=0.001, dropout=True, seed=seed)
        by_hand = ck.train_weights(handle)
    finally:
        ck.train_destroy(handle)
    for name in by_hand:
        assert np.array_equal(first[name], by_hand[name]), name
        assert np.array_equal(first[name], second[name]), name
    assert any(not np.array_equal(first[name], plain[name]) for name in by_hand)

"""bench.py's CPU-side helpers: the cpu_baseline leg must time the SAME arithmetic the oracle defines (BASELINE.md 3:
filters by the C restatement with OpenMP across frames, classifier by torch on the CPU), and count the threads it
really has."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_torch_cpu_classifier_equals_the_oracle_network(ora):
    import bench
    from camkifu_amd import synth
    from camkifu_amd.stone.nn_manager import NNManager
    W = NNManager.init_net()
    sc = synth.scene(480, 640, seed=5, density=0.3)
    dst = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)
    goban = ora.warp_perspective(sc["frame"].numpy(), ora.get_perspective_transform(sc["corners"], dst))
    p = bench.patches_of(goban[None])
    assert tuple(p.shape) == (100, 3, 40, 40)
    # patch (i, j) starts at rows / columns 0, 40, ..., 320, 340 (nn_manager.py:92-126)
    assert np.array_equal(p[99].permute(1, 2, 0).numpy().astype(np.uint8), goban[340:380, 340:380])
    assert np.array_equal(p[10].permute(1, 2, 0).numpy().astype(np.uint8), goban[40:80, 0:40])
    y = bench.torch_cpu_net(W)(p).numpy()
    y_ref = ora.cnn_predict_regions(W, goban)
    assert np.abs(y - y_ref).max() <= 1e-4 and np.array_equal(y.argmax(1), y_ref.argmax(1))


def test_across_frames_baseline_equals_the_per_call_oracle(ora):
    from camkifu_amd import synth
    from camkifu_amd.stone.nn_manager import NNManager
    W = NNManager.init_net()
    frames, corners, *_ = synth.film(3, 240, 320, seed=9, quiet=1, move_every=2, hand_frames=1)
    frames = frames.numpy()
    M = ora.get_perspective_transform(corners, np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32))
    nl, labels, used = ora.baseline_frames(W, frames, M, 3)
    nl2, gobans, _ = ora.baseline_frames(None, frames, M, 2)
    assert used >= 1 and np.array_equal(nl, nl2)
    for f in range(3):
        ref = ora.board_lines(ora.canny(ora.median(frames[f], 15), 25, 75))
        g = ora.warp_perspective(frames[f], M)
        assert nl[f] == ref["status"] and np.array_equal(gobans[f], g)
        assert np.array_equal(labels[f], ora.decode_all(ora.cnn_predict_regions(W, g))[0])


def test_host_threads_is_what_the_process_may_use():
    import bench
    n = bench.host_threads()
    assert 1 <= n <= (os.cpu_count() or 1)
    if hasattr(os, "sched_getaffinity"):
        assert n <= len(os.sched_getaffinity(0))


def test_the_bench_line_fits_the_drivers_record_and_keeps_every_number():
    """round 5's line was 14.2 KB and the driver's record kept its last 8.4 KB: stages, filter_pass and
    bf16_streams of the driver's own run were lost.  bench_line() prints the numbers and leaves the prose to --verbose /
    DESIGN.md.  Stubbed run: round 5's full line (profiles/r05_bench.json, every leg present) plus this round's new legs
    must come out under 7 000 bytes, with every number still in it and the judged keys last."""
    import json
    import os
    import bench
    full = json.load(open(os.path.join(os.path.dirname(bench.__file__), "profiles", "r05_bench.json")))
    # this round's additions, at the size they print
    full["natural_texture_film"] = dict(value=21234.56, unit="frames/s", steps=15, board_found_by_fold=True, same_game_record=True,
                                        move_sequence_ratio=1.0, median_us_per_frame=23.456, canny_nms_us_per_frame=4.567,
                                        note="x" * 200)
    full["k1_content"]["natural_texture"] = dict(us_per_frame=23.45, radix_thresholds_per_tile=45.67)
    full["rccl_exchange_one_rank"]["host_ms_per_step"].update(flags=0.051, unpack=0.012)
    line = bench.bench_line(full)
    assert len(line) <= bench.LINE_BUDGET, len(line)
    short = json.loads(line)
    assert list(short)[-len(bench.LAST_KEYS):] == list(bench.LAST_KEYS)

    def numbers(o, out):
        if isinstance(o, dict):
            for k, v in o.items():
                if k not in bench.DROP_UNLESS_VERBOSE:
                    numbers(v, out)
        elif isinstance(o, (list, tuple)):
            for v in o:
                numbers(v, out)
        elif isinstance(o, (int, float)) and not isinstance(o, bool):
            out.append(float(o))
        return out
    want, got = numbers(full, []), numbers(short, [])
    want = [v for v in want if v != 0.0]                       # (idle host timers are dropped)
    from collections import Counter
    dup = numbers(full["mfma_kernel"], []) if full["mfma_kernel"]["kernel"] == full["roofline"]["kernel"] else []
    missing = Counter(want) - Counter(got) - Counter(dup)
    assert not missing, missing
    # the verbose line is the full one
    assert len(bench.bench_line(full, verbose=True)) > 12000
    for key in ("roofline", "cpu_baseline", "stages", "filter_pass", "bf16_streams", "uhd_4k", "pcie_inclusive"):
        assert key in short
    assert short["roofline"]["bound"] == "mfma" and "traffic" in short["roofline"] and "frac" in short["roofline"]
    assert {"value", "unit", "cores", "kind", "sample"} <= set(short["cpu_baseline"])


def test_dump_outputs_writes_every_array_as_float_within_the_budget(tmp_path):
    """--dump-outputs: the last step's records, counts, requests and transform as float32 / float64 .npy files; over the
    byte budget a fixed seeded sample of the frames, the same one every time"""
    import bench
    from camkifu_amd import pipeline
    n = 40
    rng = np.random.default_rng(3)
    rec = np.zeros(n, pipeline.REC)
    rec["status"], rec["n_lines"], rec["biggest_area"] = 1, rng.integers(0, 9, n), rng.random(n) * 1e5
    rec["lines"] = rng.random(rec["lines"].shape).astype(np.float32)
    rec["region_label"] = rng.integers(0, 3, rec["region_label"].shape)
    rec["region_conf"] = rng.random(rec["region_conf"].shape)
    counts = rng.integers(0, 50, (n, 19, 19)).astype(np.int32)
    emitted = [()] * n
    emitted[7] = [(2, [("B", 3, 4), ("W", 15, 16)])]
    emitted[30] = [(1, [("W", 0, 18)])]
    mtx = rng.random((3, 3))
    names = bench.dump_outputs(str(tmp_path / "all"), rec, counts, emitted, mtx)
    got = {k: np.load(str(tmp_path / "all" / (k + ".npy"))) for k in names}
    assert set(got) == {"frame_index", "board_result", "board_lines", "region_label", "region_conf", "fg_counts", "requests", "transform"}
    for a in got.values():
        assert a.dtype in (np.float32, np.float64)
    assert np.array_equal(got["frame_index"], np.arange(n))
    assert np.array_equal(got["board_lines"], rec["lines"]) and np.array_equal(got["region_conf"], rec["region_conf"])
    assert np.array_equal(got["region_label"], rec["region_label"]) and np.array_equal(got["board_result"][:, 2], rec["n_lines"])
    assert np.array_equal(got["fg_counts"], counts.reshape(n, -1))
    assert got["requests"].tolist() == [[7, 2, 1, 3, 4], [7, 2, 2, 15, 16], [30, 1, 2, 0, 18]]
    assert np.array_equal(got["transform"], mtx)
    # a budget for 10 frames: a sorted seeded sample of 10, the same on a second call
    small = 10 * 3200 + 4096
    a = bench.dump_outputs(str(tmp_path / "a"), rec, counts, emitted, None, budget=small)
    bench.dump_outputs(str(tmp_path / "b"), rec, counts, emitted, None, budget=small)
    total = sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in a)
    assert total <= small
    ia, ib = np.load(str(tmp_path / "a" / "frame_index.npy")), np.load(str(tmp_path / "b" / "frame_index.npy"))
    assert 0 < len(ia) < n and np.array_equal(ia, ib) and np.all(np.diff(ia) > 0)
    assert np.array_equal(np.load(str(tmp_path / "a" / "region_conf.npy")), rec["region_conf"][ia.astype(int)])
    assert np.isnan(np.load(str(tmp_path / "a" / "transform.npy"))).all()

#!/usr/bin/env python3
"""Timing of the frame source with and without downsampling, in ONE process on one GPU -> profiles/ingest_timing.json

1. kernels, HIP-event time (ck_timing_get) on a batch of I420 frames resident in HBM (32 frames of 3840x2160: 0.4 GB in,
   0.8 GB of BGR -- more than the 256 MiB Infinity Cache holds between two uses), every output preallocated:
     i420_to_bgr     ck_i420_to_bgr alone                     reads 1.5 hw, writes 3 hw
     composition     ck_i420_to_bgr, then ck_pyr_down         the above + reads 3 hw, writes 0.75 hw
     fused           ck_i420_to_bgr_pyr, one level            reads 1.5 hw, writes 0.75 hw
     pyr_down        ck_pyr_down alone, from BGR              reads 3 hw, writes 0.75 hw
   every shape is warmed up, then `--reps` rounds visit the four in turn (so that clock and temperature drift hits
   all of them alike); per variant: median, min, max, spread = (max - min) / median, algorithmic bytes from the shapes
   and their share of the HBM peak.  `fused_faster_than_composition` holds when the slowest fused round beats the fastest
   composition round.
2. end to end: one filmed game (synth.film) held as I420 in pinned host memory, through FastFilePipeline.process_y4m at
   downsample=0 and downsample=1 in turn: frames/s and the game record of each against the film's moves.

    python tools/ingest_timing.py [--size 3840x2160] [--n 32] [--reps 7] [--inner 16] [--film 128] [--e2e-reps 5]

There is no CPU fallback: without a GPU the first device call raises."""
import argparse
import difflib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X


def algorithmic_bytes(h, w):
    """per frame, from the shapes alone"""
    hw, oh, ow = h * w, (h + 1) // 2, (w + 1) // 2
    conv = hw * 3 // 2 + hw * 3
    down = hw * 3 + oh * ow * 3
    return dict(i420_to_bgr=conv, composition=conv + down, fused=hw * 3 // 2 + oh * ow * 3, pyr_down=down)


def spread_of(ms):
    ms = sorted(ms)
    med = float(np.median(ms))
    return dict(median_ms=round(med, 5), min_ms=round(ms[0], 5), max_ms=round(ms[-1], 5), spread=round((ms[-1] - ms[0]) / med, 4), rounds=len(ms))


def i420_of(bgr):
    """synth.bgr_to_i420 on whatever device the (n, h, w, 3) uint8 tensor lives on -> (n, h*w*3/2) uint8"""
    import torch
    f = bgr.to(torch.int32)
    n, h, w = f.shape[:3]
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128

    def sub(c):
        return (c.reshape(n, h // 2, 2, w // 2, 2).sum(dim=(2, 4)) + 2) >> 2
    return torch.cat([y.reshape(n, -1), sub(u).reshape(n, -1), sub(v).reshape(n, -1)], 1).clamp(0, 255).to(torch.uint8)


class I420Clip:
    """what process_y4m asks of a capture, over I420 frames in (pinned) host memory.  Read at file_fps = fps the reader
    visits file frames 1, 3, 5, ... (core.capture.file_frame_indices), so file frame k is clip frame k // 2: every
    clip frame is analysed once, in order."""

    def __init__(self, frames, h, w, fps=5.0):
        self.frames, self.h, self.w, self.fps, self.fsize = frames, h, w, float(fps), h * w * 3 // 2

    def __len__(self):
        return 2 * len(self.frames)

    def read_raw_batch(self, indices, out=None):
        if out is None:
            out = np.empty((len(indices), self.fsize), np.uint8)
        for k, i in enumerate(indices):
            out[k] = self.frames[i // 2]
        return out[:len(indices)]


def game_quality(reqs, truth, moves, nframes, settle=14, first_frame=50):
    """the requests against the film: the position the first assessment sees, then the moves (bench.py's measure)"""
    sym = "EBW"
    first = [(sym[truth[first_frame][r, c]], r, c) for r in range(19) for c in range(19) if truth[first_frame][r, c]]
    played = [(sym[col], r, c) for col, r, c, f in moves if f + settle < nframes]
    seen = [m for per_frame in reqs for kind, ms in per_frame for m in ms]
    ratio = difflib.SequenceMatcher(a=["%s%d,%d" % m for m in first + played], b=["%s%d,%d" % m for m in seen]).ratio()
    return dict(move_sequence_ratio=round(ratio, 4), moves_true=len(first) + len(played), moves_recorded=len(seen))


def plan(args):
    w, h = (int(v) for v in args.size.lower().split("x"))
    if (h | w) & 1:
        raise SystemExit("--size: I420 needs even dimensions")
    by = algorithmic_bytes(h, w)
    return dict(height=h, width=w, batch=args.n, rounds=args.reps, calls_per_round=args.inner,
                algorithmic_bytes_per_frame=by, film_frames=args.film, e2e_rounds=args.e2e_reps)


def kernel_leg(ctx, args, h, w, out):
    import torch
    from camkifu_amd import capi, synth
    dev = torch.device("cuda", 0)
    n = args.n
    scene = synth.scene(h, w, seed=synth.SEED, device=dev)["frame"]
    noise = torch.randint(0, 8, (n, h, w, 3), dtype=torch.uint8, device=dev)
    i420 = i420_of(scene[None] // 2 + 60 + noise).contiguous()          # n different frames of one scene
    del noise
    oh, ow = capi.pyr_shape(h, w, 1)
    bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    small = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
    small2 = torch.empty_like(small)
    variants = {
        "i420_to_bgr": (lambda: ctx.i420_to_bgr(i420, h, w, out=bgr), ("i420_to_bgr",)),
        "composition": (lambda: ctx.pyr_down(ctx.i420_to_bgr(i420, h, w, out=bgr), 1, out=small), ("i420_to_bgr", "pyr_down")),
        "fused": (lambda: ctx.i420_to_bgr(i420, h, w, out=small2, levels=1), ("i420_pyr_down",)),
        "pyr_down": (lambda: ctx.pyr_down(bgr, 1, out=small), ("pyr_down",)),
    }
    for call, _ in variants.values():                                   # warm up every shape
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    same = bool(torch.equal(small, small2))
    ctx.timing_enable(True)
    ms = {k: [] for k in variants}
    for _ in range(args.reps):
        for name, (call, scopes) in variants.items():
            ctx.timing_reset()
            for _ in range(args.inner):
                call()
            ms[name].append(sum(ctx.timing_get(s)[0] for s in scopes) / (args.inner * n))      # ms per frame
    ctx.timing_enable(False)
    by = algorithmic_bytes(h, w)
    res = {}
    for name in variants:
        s = spread_of(ms[name])
        gbs = by[name] / (s["median_ms"] * 1e-3)
        res[name] = dict(per_frame=s, algorithmic_bytes_per_frame=by[name], gb_per_s=round(gbs / 1e9, 1),
                         share_of_hbm_peak=round(gbs / HBM_PEAK, 4))
    fused, comp = res["fused"]["per_frame"], res["composition"]["per_frame"]
    res["fused_equals_composition"] = same
    res["speedup_fused_over_composition"] = round(comp["median_ms"] / fused["median_ms"], 3)
    res["fused_faster_than_composition"] = bool(fused["max_ms"] < comp["min_ms"])
    out["kernels"] = res
    del i420, bgr, small, small2
    torch.cuda.empty_cache()


def e2e_leg(ctx, args, h, w, out):
    import torch
    from camkifu_amd import capi, pipeline, synth
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.stone.nn_manager import NNManager
    dev = torch.device("cuda", 0)
    F = args.film
    film, corners, truth, moves, hands = synth.film(F, h, w, seed=synth.SEED, device=dev, quiet=52, move_every=32, hand_frames=12)
    host = torch.empty((F, h * w * 3 // 2), dtype=torch.uint8).pin_memory()
    for b0 in range(0, F, 8):
        host[b0:b0 + 8].copy_(i420_of(film[b0:b0 + 8]))
    del film
    torch.cuda.empty_cache()
    clip = I420Clip(host.numpy(), h, w)
    ctx.cnn_set_weights(NNManager.init_net())
    legs = {}
    for levels in (0, 1):
        ph, pw = capi.pyr_shape(h, w, levels)

        def run():
            p = pipeline.FastFilePipeline(ph, pw, ControllerHeadless(), ctx=ctx)
            try:
                t0 = time.perf_counter()
                reqs = p.process_y4m(clip, batch=args.batch, downsample=levels)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, reqs, p.mtx is not None
            finally:
                p.close()
        legs[levels] = dict(run=run, seconds=[])
        legs[levels]["first"] = run()                                     # warm-up, and the record that is reported
    for _ in range(args.e2e_reps):
        for levels in (0, 1):
            legs[levels]["seconds"].append(legs[levels]["run"]()[0])
    res = {}
    for levels in (0, 1):
        secs, (_, reqs, found) = legs[levels]["seconds"], legs[levels]["first"]
        fps = sorted(F / s for s in secs)
        res["downsample_%d" % levels] = dict(
            frames_per_s=dict(median=round(float(np.median(fps)), 1), min=round(fps[0], 1), max=round(fps[-1], 1),
                              spread=round((fps[-1] - fps[0]) / float(np.median(fps)), 4), rounds=len(fps)),
            analysed_size="%dx%d" % capi.pyr_shape(h, w, levels)[::-1], board_found=bool(found),
            game_record=game_quality(reqs, truth, moves, F))
    res["speedup"] = round(res["downsample_1"]["frames_per_s"]["median"] / res["downsample_0"]["frames_per_s"]["median"], 3)
    res["note"] = ("I420 frames in pinned host memory -> H2D -> conversion (downsample=1: fused with one pyrDown level) -> board and "
                   "stones paths -> requests on the host; one context, batches of %d" % args.batch)
    out["end_to_end"] = res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH of the frames")
    ap.add_argument("--n", type=int, default=32, help="frames per batch of the kernel leg")
    ap.add_argument("--reps", type=int, default=7, help="alternating rounds of the kernel leg (at least 5)")
    ap.add_argument("--inner", type=int, default=16, help="calls per variant and round")
    ap.add_argument("--film", type=int, default=128, help="frames of the filmed game of the end-to-end leg (0: skip)")
    ap.add_argument("--batch", type=int, default=32, help="frames per pipeline batch")
    ap.add_argument("--e2e-reps", type=int, default=5, help="alternating rounds of the end-to-end leg (at least 5)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_timing.json"))
    args = ap.parse_args(argv)
    if args.reps < 5 or (args.film and args.e2e_reps < 5):
        raise SystemExit("at least 5 alternating rounds per leg")
    out = dict(tool="tools/ingest_timing.py", plan=plan(args))
    h, w = out["plan"]["height"], out["plan"]["width"]
    from camkifu_amd import capi
    ctx = capi.Context(0)                                                 # no GPU: CkError, nothing is timed on a CPU
    try:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
        kernel_leg(ctx, args, h, w, out)
        if args.film:
            e2e_leg(ctx, args, h, w, out)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    k = out["kernels"]
    print("fused %.4f ms/frame, composition %.4f ms/frame: %.2fx, %s the spread"
          % (k["fused"]["per_frame"]["median_ms"], k["composition"]["per_frame"]["median_ms"], k["speedup_fused_over_composition"],
             "beyond" if k["fused_faster_than_composition"] else "NOT beyond"), file=sys.stderr)
    return out


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the overlay rasteriser, in ONE process on one GPU -> profiles/overlay_timing.json

1. kernel: ck_overlay_draw (HIP-event time, ck_timing_get("overlay_draw")) per frame for
     - the goban annotation of a synthetic mid-game position (core/annotate.goban_list) on 380 x 380 images,
     - the full-frame annotation (core/annotate.frame_list) on 1920 x 1080 frames,
   each on a batch resident in HBM, with the bytes of the covered pixels (counted on the GPU: the same list in opaque
   white on black images) and the GB/s they make; beside ck_jpeg_forward on the same frames (ck_timing_get("jpeg_enc")).
2. the tool: tools/transcode.py's record_gobans with annotate=True against annotate=False on the same 128-frame film,
   frames/s, three runs each, with the spread.
Where cv2 is importable, the pixels by which the rasteriser's segments and rings differ from cv2.line / cv2.circle are
counted and printed; that figure is reported, never asserted.

    python tools/overlay_timing.py [--n 32] [--reps 7] [--inner 8] [--film 128]

There is no CPU fallback: without a GPU the first device call raises."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_timing import HBM_PEAK, spread_of  # noqa: E402


def midgame(seed=4, stones=120):
    rng = np.random.RandomState(seed)
    codes = np.zeros(361, np.uint8)
    codes[rng.choice(361, stones, replace=False)] = rng.randint(1, 3, stones)
    fg = np.zeros((19, 19), np.int32)
    fg[5:7, 9:12] = 400
    return codes.reshape(19, 19), fg


def opaque_white(dl):
    from camkifu_amd.core import overlay
    out = overlay.DisplayList()
    out.prims = [p[:6] + (0xffffffff, p[7]) for p in dl.prims]
    return out


def kernel_leg(ctx, torch, frames, lists, quant, reps, inner):
    """-> dict: overlay kernel and forward kernel per frame, covered bytes, GB/s"""
    from camkifu_amd import capi
    n, h, w = frames.shape[:3]
    black = torch.zeros_like(frames)
    ctx.overlay_draw(black, [opaque_white(dl) for dl in lists])
    covered = int((black[..., 0] != 0).sum().item()) / n
    coef = torch.empty((n, capi.jpeg_blocks(h, w, capi.CK_JPEG_420) * 64), dtype=torch.int16, device=frames.device)
    work = frames.clone()
    for _ in range(3):
        ctx.overlay_draw(work, lists)
        ctx.jpeg_forward(work, quant, capi.CK_JPEG_420, out=coef)
    ctx.timing_enable(True)
    draw, fwd, host = [], [], []
    for _ in range(reps):
        ctx.timing_reset()
        t0 = time.perf_counter()
        for _ in range(inner):
            ctx.overlay_draw(work, lists)
        host.append((time.perf_counter() - t0) * 1e3 / (inner * n))
        draw.append(ctx.timing_get("overlay_draw")[0] / (inner * n))
        for _ in range(inner):
            ctx.jpeg_forward(work, quant, capi.CK_JPEG_420, out=coef)
        fwd.append(ctx.timing_get("jpeg_enc")[0] / (inner * n))
    ctx.timing_enable(False)
    sd = spread_of(draw)
    blended = sum(1 for p in lists[0].prims if (p[6] >> 24) != 255)
    return dict(height=h, width=w, batch=n, primitives_per_frame=len(lists[0]), blended_primitives_per_frame=blended,
                overlay_kernel_per_frame=sd, overlay_call_per_frame_host=spread_of(host), jpeg_forward_per_frame=spread_of(fwd),
                covered_pixels_per_frame=round(covered, 1), covered_bytes_per_frame=int(covered * 3),
                gb_per_s_of_covered_bytes=round(covered * 3 / (sd["median_ms"] * 1e-3) / 1e9, 2),
                share_of_hbm_peak=round(covered * 3 / (sd["median_ms"] * 1e-3) / HBM_PEAK, 5))


def cv2_difference():
    """pixels by which segments and rings differ from cv2's, or None without cv2"""
    try:
        import cv2
    except ImportError:
        return None
    from camkifu_amd import capi
    from camkifu_amd.core import overlay
    ctx = capi.get_context()
    rng = np.random.RandomState(1)
    seg = ring = 0
    for _ in range(200):
        x0, y0, x1, y1 = (int(v) for v in rng.randint(0, 96, 4))
        a, b = np.zeros((96, 96), np.uint8), np.zeros((96, 96), np.uint8)
        cv2.line(a, (x0, y0), (x1, y1), 255)
        ctx.overlay_draw(b, overlay.DisplayList().segment(x0, y0, x1, y1))
        seg += int((a != b).sum())
    for r in range(1, 41):
        a, b = np.zeros((96, 96), np.uint8), np.zeros((96, 96), np.uint8)
        cv2.circle(a, (48, 48), r, 255)
        ctx.overlay_draw(b, overlay.DisplayList().circle(48, 48, r))
        ring += int((a != b).sum())
    return dict(segments=200, segment_pixels_differing=seg, rings=40, ring_pixels_differing=ring)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32, help="frames per batch of the kernel legs")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8, help="calls per round")
    ap.add_argument("--film", type=int, default=128, help="frames of the film of the tool leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_timing.json"))
    args = ap.parse_args(argv)
    if args.reps < 5:
        raise SystemExit("at least 5 rounds per leg")
    import torch
    from camkifu_amd import capi, synth
    from camkifu_amd.board.boardfinder import GobanCorners
    from camkifu_amd.core import annotate
    from camkifu_amd.stone.nn_manager import NNManager
    from camkifu_amd.stone.stonesfinder import PosGrid
    ctx = capi.get_context()
    dev = torch.device("cuda", 0)
    out = dict(tool="tools/overlay_timing.py", device=torch.cuda.get_device_name(0),
               plan=dict(rounds=args.reps, calls_per_round=args.inner, bin_size=capi.overlay_plan(0, 0, 0, np.zeros((0, 8), np.int32), [0])[0]))
    quant = capi.jpeg_quant(90)
    codes, fg = midgame()
    grid = PosGrid(380)
    n, h, w = args.n, 1080, 1920
    # 1. the kernel, on goban images and on full frames of a filmed game
    film, corners = synth.film(n, h, w, seed=synth.SEED, device=dev, quiet=8, move_every=8, hand_frames=4)[:2]
    film = film.contiguous()
    dst = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)
    mtx = capi.get_perspective_transform(np.asarray(corners, np.float32), dst)
    gobans = ctx.warp_perspective(film, mtx, 380)
    out["goban_380"] = kernel_leg(ctx, torch, gobans, [annotate.goban_list(codes, fg, grid, f + 1, n, "B[D4] W[Q16]") for f in range(n)],
                                  quant, args.reps, args.inner)
    quad = GobanCorners([tuple(int(v) for v in p) for p in np.asarray(corners)])
    out["frame_1080"] = kernel_leg(ctx, torch, film, [annotate.frame_list((h, w), quad, mtx, codes, grid, f + 1, n, "B[D4] W[Q16]")
                                                      for f in range(n)], quant, args.reps, args.inner)
    del gobans
    # 2. the tool: the same film with and without the annotation
    spec = importlib.util.spec_from_file_location("transcode", os.path.join(ROOT, "tools", "transcode.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    frames = synth.film(args.film, h, w, seed=synth.SEED, device=dev, quiet=8, move_every=8, hand_frames=4)[0].cpu().numpy()
    del film
    ctx.cnn_set_weights(NNManager.get_net())
    rates = {False: [], True: []}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "seen.avi")
        tr.record_gobans(frames, path, ctx=ctx, annotate=True)                     # warm-up of both paths
        for _ in range(3):
            for flag in (False, True):
                t0 = time.perf_counter()
                res = tr.record_gobans(frames, path, ctx=ctx, annotate=flag)
                rates[flag].append(res["frames"] / (time.perf_counter() - t0))

    def fps_of(v):
        v = sorted(v)
        return dict(median=round(float(np.median(v)), 1), min=round(v[0], 1), max=round(v[-1], 1),
                    spread=round((v[-1] - v[0]) / float(np.median(v)), 4), runs=len(v))
    plain, drawn = fps_of(rates[False]), fps_of(rates[True])
    out["record_gobans"] = dict(film_frames=args.film, height=h, width=w, plain_frames_per_s=plain, annotated_frames_per_s=drawn,
                                annotated_over_plain=round(drawn["median"] / plain["median"], 4),
                                annotated_within_plain_spread=bool(plain["min"] <= drawn["median"] <= plain["max"]))
    diff = cv2_difference()
    out["cv2"] = diff if diff is not None else "cv2 is not importable here: not measured"
    print("difference from cv2.line / cv2.circle:", out["cv2"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the JPEG encoder, in ONE process on one GPU -> profiles/jpeg_enc_timing.json

Frames of a filmed game (synth.film) at 1920x1080, resident in HBM; 4:2:0, quality 90.
1. kernel: ck_jpeg_forward on the batch, output preallocated, HIP-event time (ck_timing_get("jpeg_enc")) per frame, beside
   ck_jpeg_reconstruct on the coefficients the forward kernel wrote (ck_timing_get("jpeg"): the same bytes the other way,
   mirrored arithmetic), in alternating rounds, and the compulsory 6 * W * H bytes of a 4:2:0 frame against the HBM peak.
2. host: the Huffman coder alone (capi.jpeg_entropy_encode), ms per frame -- one frame per call (one thread) and the whole
   batch per call (the library's worker threads, at most 16).
3. end to end: Context.jpeg_encode of the batch in HBM -> a list of bytes, frames/s.
Every leg is warmed up and runs `--reps` rounds: median / min / max.

    python tools/jpeg_enc_timing.py [--size 1920x1080] [--n 32] [--reps 7] [--inner 8]

There is no CPU fallback: without a GPU the first device call raises."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_timing import HBM_PEAK, spread_of  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--n", type=int, default=32, help="frames per batch")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8, help="kernel calls per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_enc_timing.json"))
    args = ap.parse_args(argv)
    if args.reps < 5:
        raise SystemExit("at least 5 rounds per leg")
    import torch
    from camkifu_amd import capi, synth
    w, h = (int(v) for v in args.size.lower().split("x"))
    n, S = args.n, capi.CK_JPEG_420
    ctx = capi.Context(0)
    dev = torch.device("cuda", 0)
    out = dict(tool="tools/jpeg_enc_timing.py", device=torch.cuda.get_device_name(0),
               plan=dict(height=h, width=w, sampling="4:2:0", quality=args.quality, batch=n, rounds=args.reps,
                         kernel_calls_per_round=args.inner))
    film = synth.film(n, h, w, seed=synth.SEED, device=dev, quiet=8, move_every=8, hand_frames=4)[0].contiguous()
    quant = capi.jpeg_quant(args.quality)
    try:
        # 1. the two kernels
        coef = torch.empty((n, capi.jpeg_blocks(h, w, S) * 64), dtype=torch.int16, device=dev)
        back = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        d_quant = torch.from_numpy(np.repeat(quant[None], n, axis=0).view(np.int16)).to(dev)
        for _ in range(3):
            ctx.jpeg_forward(film, quant, S, out=coef)
            ctx.jpeg_reconstruct(coef, d_quant, h, w, S, out=back)
        ctx.timing_enable(True)
        fwd, inv = [], []
        for _ in range(args.reps):
            ctx.timing_reset()
            for _ in range(args.inner):
                ctx.jpeg_forward(film, quant, S, out=coef)
            fwd.append(ctx.timing_get("jpeg_enc")[0] / (args.inner * n))
            for _ in range(args.inner):
                ctx.jpeg_reconstruct(coef, d_quant, h, w, S, out=back)
            inv.append(ctx.timing_get("jpeg")[0] / (args.inner * n))
        ctx.timing_enable(False)
        sf, si = spread_of(fwd), spread_of(inv)
        floor = 6 * w * h
        out["kernel"] = dict(forward_per_frame=sf, reconstruct_per_frame=si,
                             forward_over_reconstruct=round(sf["median_ms"] / si["median_ms"], 3),
                             floor_bytes_per_frame=floor, bytes_per_frame_with_mcu_padding=capi.jpeg_blocks(h, w, S) * 128 + h * w * 3,
                             floor_ms_at_hbm_peak=round(floor / HBM_PEAK * 1e3, 5),
                             gb_per_s_against_floor=round(floor / (sf["median_ms"] * 1e-3) / 1e9, 1),
                             share_of_hbm_peak=round(floor / (sf["median_ms"] * 1e-3) / HBM_PEAK, 4))
        # 2. the Huffman coder
        host_coef = coef.cpu().numpy()
        del coef, back, d_quant
        streams = capi.jpeg_entropy_encode(host_coef, quant, h, w, S)
        capi.jpeg_entropy_encode(host_coef[0], quant, h, w, S)
        one, many = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for f in range(n):
                capi.jpeg_entropy_encode(host_coef[f], quant, h, w, S)
            one.append((time.perf_counter() - t0) * 1e3 / n)
            t0 = time.perf_counter()
            capi.jpeg_entropy_encode(host_coef, quant, h, w, S)
            many.append((time.perf_counter() - t0) * 1e3 / n)
        out["plan"]["jpeg_bytes_per_frame"] = int(np.mean([len(s) for s in streams]))
        out["host_entropy_encode"] = dict(one_thread_ms_per_frame=spread_of(one), sixteen_threads_ms_per_frame=spread_of(many),
                                          cpus_seen=os.cpu_count(),
                                          note="includes the allocation of the output buffer of each call and the copy into bytes")
        # 3. end to end
        same = ctx.jpeg_encode(film, quality=args.quality, sampling=S) == streams
        ctx.jpeg_encode(film, quality=args.quality, sampling=S)
        secs = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ctx.jpeg_encode(film, quality=args.quality, sampling=S)
            secs.append(time.perf_counter() - t0)
        fps = sorted(n / t for t in secs)
        out["end_to_end"] = dict(frames_per_s=dict(median=round(float(np.median(fps)), 1), min=round(fps[0], 1), max=round(fps[-1], 1),
                                                   spread=round((fps[-1] - fps[0]) / float(np.median(fps)), 4), rounds=len(fps)),
                                 frames_resident_in_hbm=True, two_halves_equal_encode=bool(same))
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the JPEG encoder, in ONE process on one GPU -> profiles/jpeg_enc_timing.json

Frames of a filmed game (synth.film) at 1920x1080, resident in HBM; 4:2:0, quality 90.
1. kernel: ck_jpeg_forward on the batch, output preallocated, HIP-event time (ck_timing_get("jpeg_enc")) per frame, beside
   ck_jpeg_reconstruct on the coefficients the forward kernel wrote (ck_timing_get("jpeg"): the same bytes the other way,
   mirrored arithmetic), in alternating rounds, and the compulsory 6 * W * H bytes of a 4:2:0 frame against the HBM peak.
2. host: the Huffman coder alone (capi.jpeg_entropy_encode), ms per frame -- one frame per call (one thread) and the whole
   batch per call (the library's worker threads, at most 16).
3. end to end: Context.jpeg_encode of the batch in HBM -> a list of bytes, frames/s.
4. device_entropy: the Huffman stage on the GPU (jpeg_set_encode_entropy("device")) against the host mode in the same
   run: HIP-event time per frame of its four kernels beside the forward kernel, the bytes that come down per frame in both
   modes, jpeg_encode frames/s in both modes at 128, 32, 8 and 1 frames a call (alternating rounds), and
   tools/transcode.record_gobans on a 128-frame film in both modes.  The streams of both modes are compared.
5. optimised: Huffman tables fitted to every frame (jpeg_encode(optimize=True)) against the standard tables in the same run:
   bytes per frame and their ratio, HIP-event time per frame of jpeg_enc_histo and jpeg_enc_tables beside the four other
   steps, and jpeg_encode frames/s at 128, 32, 8 and 1 frames a call -- device-optimised against device-standard and
   host-optimised against host-standard, alternating rounds.  The streams of both entropy modes are compared.
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


KERNELS = ("jpeg_enc_size", "jpeg_enc_scan", "jpeg_enc_put", "jpeg_enc_stuff")
OPT_KERNELS = ("jpeg_enc_histo", "jpeg_enc_tables")


def _fps(ctx, frames, quality, S, reps):
    """frames/s of jpeg_encode in the host and the device mode, alternating rounds"""
    n = frames.shape[0]
    calls = max(2, 256 // n)                                 # (a round codes at least 256 frames in each mode)
    secs = {"host": [], "device": []}
    for mode in ("host", "device"):
        ctx.jpeg_set_encode_entropy(mode)
        ctx.jpeg_encode(frames, quality=quality, sampling=S)
    for _ in range(reps):
        for mode in ("host", "device"):
            ctx.jpeg_set_encode_entropy(mode)
            t0 = time.perf_counter()
            for _ in range(calls):
                ctx.jpeg_encode(frames, quality=quality, sampling=S)
            secs[mode].append((time.perf_counter() - t0) / calls)
    ctx.jpeg_set_encode_entropy("host")
    res = {}
    for mode, ts in secs.items():
        fps = sorted(n / t for t in ts)
        res[mode] = dict(median=round(float(np.median(fps)), 1), min=round(fps[0], 1), max=round(fps[-1], 1), rounds=len(fps))
    res["device_over_host"] = round(res["device"]["median"] / res["host"]["median"], 3)
    return res


def _fps_tables(ctx, frames, quality, S, reps, mode):
    """frames/s of jpeg_encode with the standard and with optimised tables in one entropy mode, alternating rounds"""
    n = frames.shape[0]
    calls = max(2, 256 // n)
    ctx.jpeg_set_encode_entropy(mode)
    secs = {"standard": [], "optimised": []}
    for tables in secs:
        ctx.jpeg_encode(frames, quality=quality, sampling=S, optimize=tables == "optimised")
    for _ in range(reps):
        for tables in secs:
            t0 = time.perf_counter()
            for _ in range(calls):
                ctx.jpeg_encode(frames, quality=quality, sampling=S, optimize=tables == "optimised")
            secs[tables].append((time.perf_counter() - t0) / calls)
    ctx.jpeg_set_encode_entropy("host")
    res = {}
    for tables, ts in secs.items():
        fps = sorted(n / t for t in ts)
        res[tables] = dict(median=round(float(np.median(fps)), 1), min=round(fps[0], 1), max=round(fps[-1], 1), rounds=len(fps))
    res["optimised_over_standard"] = round(res["optimised"]["median"] / res["standard"]["median"], 3)
    return res


def optimised(ctx, film, S, args):
    n, q = film.shape[0], args.quality
    res = {}
    ctx.jpeg_set_encode_entropy("host")
    standard = ctx.jpeg_encode(film, quality=q, sampling=S)
    want = ctx.jpeg_encode(film, quality=q, sampling=S, optimize=True)
    ctx.jpeg_set_encode_entropy("device")
    res["streams_equal_the_host_modes"] = bool(ctx.jpeg_encode(film, quality=q, sampling=S, optimize=True) == want)
    res["downloaded_bytes_per_frame_device"] = ctx.jpeg_downloaded_bytes() // n
    a, b = float(np.mean([len(s) for s in standard])), float(np.mean([len(s) for s in want]))
    res["jpeg_bytes_per_frame"] = dict(standard=int(a), optimised=int(b), optimised_over_standard=round(b / a, 4))
    ctx.timing_enable(True)
    per = {k: [] for k in ("jpeg_enc",) + OPT_KERNELS + KERNELS}
    for _ in range(args.reps):
        ctx.timing_reset()
        ctx.jpeg_encode(film, quality=q, sampling=S, optimize=True)
        for k in per:
            per[k].append(ctx.timing_get(k)[0] / n)
    ctx.timing_enable(False)
    ctx.jpeg_set_encode_entropy("host")
    res["kernel_ms_per_frame"] = {("jpeg_forward" if k == "jpeg_enc" else k): spread_of(v) for k, v in per.items()}
    res["encode_frames_per_s"] = {}
    for b in (128, 32, 8, 1):
        frames = film if b == n else (film[:b].contiguous() if b < n else film.repeat((b + n - 1) // n, 1, 1, 1)[:b].contiguous())
        res["encode_frames_per_s"]["%d_frames_a_call" % b] = {mode: _fps_tables(ctx, frames, q, S, args.reps, mode) for mode in ("device", "host")}
        del frames
    return res


def device_entropy(ctx, capi, synth, dev, film, h, w, S, args):
    import tempfile

    import torch
    n, q = film.shape[0], args.quality
    res = {}
    ctx.jpeg_set_encode_entropy("host")
    want = ctx.jpeg_encode(film, quality=q, sampling=S)
    host_down = ctx.jpeg_downloaded_bytes()
    ctx.jpeg_set_encode_entropy("device")
    res["streams_equal_the_host_modes"] = bool(ctx.jpeg_encode(film, quality=q, sampling=S) == want)
    res["downloaded_bytes_per_frame"] = dict(host=host_down // n, device=ctx.jpeg_downloaded_bytes() // n)
    # the kernels
    ctx.timing_enable(True)
    per = {k: [] for k in ("jpeg_enc",) + KERNELS}
    for _ in range(args.reps):
        ctx.timing_reset()
        ctx.jpeg_encode(film, quality=q, sampling=S)
        for k in per:
            per[k].append(ctx.timing_get(k)[0] / n)
    ctx.timing_enable(False)
    ctx.jpeg_set_encode_entropy("host")
    res["kernel_ms_per_frame"] = {("jpeg_forward" if k == "jpeg_enc" else k): spread_of(v) for k, v in per.items()}
    # frames/s by batch size
    res["encode_frames_per_s"] = {}
    for b in (128, 32, 8, 1):
        frames = film if b == n else (film[:b].contiguous() if b < n else film.repeat((b + n - 1) // n, 1, 1, 1)[:b].contiguous())
        res["encode_frames_per_s"]["%d_frames_a_call" % b] = _fps(ctx, frames, q, S, args.reps)
        del frames
    # record_gobans on a 128-frame film of 640 x 480
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import transcode
    from camkifu_amd.stone.nn_manager import NNManager
    small = synth.film(128, 480, 640, seed=8, quiet=8, move_every=30, hand_frames=12)[0].numpy()
    ctx.cnn_set_weights(NNManager.init_net())
    rec = {"host": [], "device": []}
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(1 + max(3, args.reps // 2)):
            for mode in ("host", "device"):
                ctx.jpeg_set_encode_entropy(mode)
                t0 = time.perf_counter()
                transcode.record_gobans(small, os.path.join(tmp, mode + ".avi"), quality=q, batch=32, ctx=ctx, bg_init_frames=6)
                if rnd:
                    rec[mode].append(time.perf_counter() - t0)
        with open(os.path.join(tmp, "host.avi"), "rb") as a, open(os.path.join(tmp, "device.avi"), "rb") as b:
            res["record_gobans_files_equal"] = bool(a.read() == b.read())
    ctx.jpeg_set_encode_entropy("host")
    res["record_gobans_128_frames_s"] = {m: dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4),
                                                  rounds=len(t)) for m, t in rec.items()}
    torch.cuda.synchronize()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--n", type=int, default=32, help="frames per batch")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8, help="kernel calls per round")
    ap.add_argument("--only-optimised", action="store_true", help="skip leg 4 (its record_gobans runs take the longest)")
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
        if not args.only_optimised:
            out["device_entropy"] = device_entropy(ctx, capi, synth, dev, film, h, w, S, args)
        out["optimised"] = optimised(ctx, film, S, args)
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

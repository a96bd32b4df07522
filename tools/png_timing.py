#!/usr/bin/env python3
"""Timing of the PNG reader and writer, in ONE process on one GPU -> profiles/png_timing.json

Images: goban images (380 x 380: camkifu_amd/synth.py scenes through the perspective warp) and 1920 x 1080 synth frames.
1. unfilter: HIP-event time of the unfilter kernel (ck_timing_get("png_unfilter")) per frame at both sizes, for files the
   library's own encoder wrote (adaptive filters: every type occurs).
2. host inflate: capi.png_inflate of one 1080p frame's zlib stream, ms per frame on one thread and with 16 threads at
   once (16 frames in flight, the calls release the interpreter lock).
3. encoder kernels: HIP-event time per frame of png_filter, png_count, png_build, png_size, png_scan, png_put.
4. end to end: png_encode (frames resident in HBM) and png_decode (files in host memory, frames left in HBM) frames/s at
   1, 8 and 32 frames a call.
5. bytes: the files of png_encode against Pillow's default save(.., "PNG") and against zlib level 1 with Z_RLE over the same
   filtered rows (the stand-in for cv2.imwrite), goban images and a 1080p frame.
Every timed leg is warmed up and runs `--reps` rounds: median / min / max.

    python tools/png_timing.py [--reps 5] [--out profiles/png_timing.json]

There is no CPU fallback: without a GPU the first device call raises."""
import argparse
import io
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_timing import spread_of  # noqa: E402

ENC_KERNELS = ("png_filter", "png_count", "png_build", "png_size", "png_scan", "png_put")


def _idat(data):
    """the zlib stream of a file with one IDAT chunk, as png_encode writes it"""
    at = data.index(b"IDAT")
    n = int.from_bytes(data[at - 4:at], "big")
    return data[at + 4:at + 4 + n]


def _fps(fn, n, reps):
    calls = max(2, 64 // n)
    fn()
    secs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        secs.append((time.perf_counter() - t0) / calls)
    fps = sorted(n / t for t in secs)
    return dict(median=round(float(np.median(fps)), 1), min=round(fps[0], 1), max=round(fps[-1], 1), rounds=len(fps))


def _kernel_ms(ctx, fn, names, n, reps):
    fn()
    ctx.timing_enable(True)
    per = {k: [] for k in names}
    for _ in range(reps):
        ctx.timing_reset()
        fn()
        for k in names:
            per[k].append(ctx.timing_get(k)[0] / n)
    ctx.timing_enable(False)
    return {k: spread_of(v) for k, v in per.items()}


def _bytes(ours, frames):
    """bytes of our files against Pillow's default and zlib level 1 with Z_RLE over the rows our encoder filtered"""
    res = dict(raw_bytes_per_frame=int(frames[0].size), png_encode=int(np.mean([len(d) for d in ours])))
    rle = []
    for d in ours:
        co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        rle.append(57 + len(co.compress(zlib.decompress(_idat(d))) + co.flush()))
    res["zlib_level_1_rle_same_rows"] = int(np.mean(rle))
    try:
        from PIL import Image
        pil = []
        for f in frames:
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(buf, "PNG")
            pil.append(len(buf.getvalue()))
        res["pillow_default"] = int(np.mean(pil))
    except ImportError:
        res["pillow_default"] = "not measured: Pillow is not installed"
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_timing.json"))
    args = ap.parse_args(argv)
    if args.reps < 5:
        raise SystemExit("at least 5 rounds per leg")
    import torch
    from camkifu_amd import capi, synth
    ctx = capi.Context(0)
    dev = torch.device("cuda", 0)
    out = dict(tool="tools/png_timing.py", device=torch.cuda.get_device_name(0), seams=capi.png_tiles(), rounds=args.reps)
    try:
        big = synth.film(32, 1080, 1920, seed=synth.SEED, device=dev, quiet=8, move_every=8, hand_frames=4)[0].contiguous()
        dst = np.array([(0, 0), (380, 0), (380, 380), (0, 380)], np.float32)
        gobans = []
        for k in range(32):
            sc = synth.scene(480, 640, seed=synth.SEED + k)
            gobans.append(ctx.warp_perspective(sc["frame"].numpy(), capi.get_perspective_transform(sc["corners"], dst)))
        small = torch.from_numpy(np.stack(gobans)).to(dev)
        sets = {"380x380": small, "1920x1080": big}
        files = {k: ctx.png_encode(v) for k, v in sets.items()}
        out["round_trip_exact"] = {k: bool(np.array_equal(ctx.png_decode(files[k][:4]), sets[k][:4].cpu().numpy())) for k in sets}
        out["staged_encoder_same_bytes"] = bool(capi.png_encode_staged(small[:2].cpu().numpy()) == files["380x380"][:2])
        # 1. the unfilter kernel
        out["unfilter_kernel_ms_per_frame"] = {
            k: _kernel_ms(ctx, lambda k=k: ctx.png_decode(files[k][:8], to_device=dev), ("png_unfilter",), 8, args.reps)["png_unfilter"] for k in sets}
        # 2. the host inflate
        streams = [_idat(d) for d in files["1920x1080"][:16]]
        capi.png_inflate(streams[0])
        one, many = [], []
        with ThreadPoolExecutor(16) as pool:
            for _ in range(args.reps):
                t0 = time.perf_counter()
                for s in streams[:4]:
                    capi.png_inflate(s)
                one.append((time.perf_counter() - t0) * 1e3 / 4)
                t0 = time.perf_counter()
                list(pool.map(capi.png_inflate, streams))
                many.append((time.perf_counter() - t0) * 1e3 / 16)
        out["host_inflate_1080p"] = dict(one_thread_ms_per_frame=spread_of(one), sixteen_threads_ms_per_frame=spread_of(many),
                                         zlib_stream_bytes=int(np.mean([len(s) for s in streams])), cpus_seen=os.cpu_count(),
                                         note="capi.png_inflate: includes the allocation of the output and the copy into bytes")
        t0 = time.perf_counter()
        for s in streams[:4]:
            zlib.decompress(s)
        out["host_inflate_1080p"]["zlib_decompress_one_thread_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / 4, 3)
        # 3. the encoder's kernels
        out["encoder_kernel_ms_per_frame"] = {k: _kernel_ms(ctx, lambda k=k: ctx.png_encode(sets[k][:8]), ENC_KERNELS, 8, args.reps) for k in sets}
        # 4. end to end
        out["frames_per_s"] = {}
        for k in sets:
            out["frames_per_s"][k] = {}
            for b in (1, 8, 32):
                fr, fl = sets[k][:b].contiguous(), files[k][:b]
                out["frames_per_s"][k]["%d_frames_a_call" % b] = dict(
                    png_encode=_fps(lambda: ctx.png_encode(fr), b, args.reps),
                    png_decode=_fps(lambda: ctx.png_decode(fl, to_device=dev), b, args.reps))
        # 5. bytes
        out["bytes_per_frame"] = {"380x380": _bytes(files["380x380"][:8], small[:8].cpu().numpy()),
                                  "1920x1080": _bytes(files["1920x1080"][:2], big[:2].cpu().numpy())}
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

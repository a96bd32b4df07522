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
6. --runs: the encoder's runs mode beside its default mode, a round of the one after a round of the other: bytes per frame
   (runs mode, default mode, the Z_RLE stand-in) on goban images, the same images annotated with core/annotate.py's goban
   list, 1080p synth frames and an all-zero 1080p frame; kernel time per frame of every step (png_edges and png_join among
   them); png_encode frames/s at 1, 8 and 32 frames a call.
   (Without --runs a `runs` section the output file already holds is kept and marked `carried_over`.)
6b. --inflate: the section `device_inflate`, measured alone (the rest of the output file stays): png_decode with the device
   inflate beside the host inflate (16 threads), a round of the one after a round of the other.  Files as png_encode writes
   them in its default and runs modes, and the same filtered rows deflated by zlib level 6.  Kernel time of png_inflate per
   image at 1, 8, 32 and 128 images a call, tokens per window step, bytes per microsecond per wave; png_decode frames/s and
   bytes uploaded per frame in both modes.  --inflate-variant NAME files the kernel legs of another build of the library,
   loaded through CK_HIP_LIB (-DCK_PNG_INFLATE_OPL=2 or 4: offsets a lane; -DCK_PNG_INFLATE_SERIAL=1: only lane 0 decodes,
   one token a step), each beside this build's figure for the same leg; --inflate-sizes / --inflate-batches narrow the legs.
7. --baseline FILE: FILE is what another build's run of this tool wrote, the parent commit's for instance.  The default
   mode's medians of this run (sections 3 and 4, and the `none` legs of the runs section) are listed against the baseline's
   [min .. max], each with `inside` and the distance of the medians in per cent, and the baseline's figures are copied beside
   them (`default_mode_against_baseline`): whether a compile-time mode parameter has leaked into the default path.
Every timed leg is warmed up and runs `--reps` rounds: median / min / max.

    python tools/png_timing.py [--reps 5] [--runs] [--baseline FILE] [--out profiles/png_timing.json]

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


RUN_KERNELS = ("png_filter", "png_edges", "png_join", "png_count", "png_build", "png_size", "png_scan", "png_put")
MODES = ("none", "runs")


def _rle_bytes(data):
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return 57 + len(co.compress(zlib.decompress(_idat(data))) + co.flush())


def _runs_section(ctx, dev, small, big, reps):
    """the runs mode beside the default mode, in this process and in alternating rounds: bytes, kernel times, frames/s"""
    import torch
    from camkifu_amd.core import annotate
    from camkifu_amd.stone.stonesfinder import PosGrid
    from camkifu_amd import capi, synth
    grid = PosGrid(380)
    fg = np.zeros((19, 19), np.int64)
    fg[8:11, 8:11] = 1 << 20                                 # nine agitated zones: translucent red rectangles
    lists = [annotate.goban_list(synth.scene(480, 640, seed=synth.SEED + k)["stones"], fg, grid, k + 1, 8, "B[D4] W[Q16]") for k in range(8)]
    sets = {"gobans_380x380": small[:8].contiguous(), "gobans_annotated_380x380": ctx.overlay_draw(small[:8].clone(), lists),
            "synth_1920x1080": big[:2].contiguous(), "zeros_1920x1080": torch.zeros((1, 1080, 1920, 3), dtype=torch.uint8, device=dev)}
    res = dict(bytes_per_frame={}, note="zlib_level_1_rle_same_rows: zlib level 1 with Z_RLE over the rows our encoder filtered, plus the "
               "57 bytes of the container: the stand-in for cv2.imwrite")
    for k, fr in sets.items():
        runs, plain = ctx.png_encode(fr, runs=True), ctx.png_encode(fr, runs=False)
        if not np.array_equal(ctx.png_decode(runs), fr.cpu().numpy()):
            raise SystemExit("runs mode: %s does not round trip" % k)
        rle = int(np.mean([_rle_bytes(d) for d in runs]))
        r = int(np.mean([len(d) for d in runs]))
        res["bytes_per_frame"][k] = dict(runs=r, default=int(np.mean([len(d) for d in plain])), zlib_level_1_rle_same_rows=rle,
                                         runs_over_rle=round(r / rle, 3))
    ctx.png_encode(sets["gobans_annotated_380x380"], runs=True)
    st = ctx.png_run_stats()
    res["tokens_per_frame_annotated_gobans"] = dict(literals=int(np.mean([s["literals"] for s in st])), matches=int(np.mean([s["matches"] for s in st])))
    res["staged_encoder_same_bytes"] = bool(capi.png_encode_staged(small[:2].cpu().numpy(), runs=True) == ctx.png_encode(small[:2], runs=True))
    timed = {"380x380": small, "1920x1080": big}
    # kernel times: a round is one call in each mode
    ker = {k: {m: {n: [] for n in RUN_KERNELS} for m in MODES} for k in timed}
    for k, fr in timed.items():
        fr8 = fr[:8].contiguous()
        for m in MODES:
            ctx.png_encode(fr8, runs=(m == "runs"))
        ctx.timing_enable(True)
        for _ in range(reps):
            for m in MODES:
                ctx.png_set_encode_matches(m)
                ctx.timing_reset()
                ctx.png_encode(fr8)
                for n in RUN_KERNELS:
                    ker[k][m][n].append(ctx.timing_get(n)[0] / 8)
        ctx.timing_enable(False)
        ctx.png_set_encode_matches("none")
    res["encoder_kernel_ms_per_frame"] = {k: {m: {n: spread_of(v) for n, v in ker[k][m].items() if m == "runs" or n not in ("png_edges", "png_join")}
                                              for m in MODES} for k in timed}
    # frames/s: a round is `calls` calls in each mode
    res["png_encode_frames_per_s"] = {}
    for k, fr in timed.items():
        res["png_encode_frames_per_s"][k] = {}
        for b in (1, 8, 32):
            frb, calls = fr[:b].contiguous(), max(2, 64 // b)
            fps = {m: [] for m in MODES}
            for m in MODES:
                ctx.png_encode(frb, runs=(m == "runs"))
            for _ in range(reps):
                for m in MODES:
                    ctx.png_set_encode_matches(m)
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        ctx.png_encode(frb)
                    fps[m].append(b * calls / (time.perf_counter() - t0))
            ctx.png_set_encode_matches("none")
            res["png_encode_frames_per_s"][k]["%d_frames_a_call" % b] = {
                m: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1), rounds=len(v)) for m, v in fps.items()}
    return res


def _rewrap(data, level):
    """the file with the same filtered rows deflated by zlib at `level`: matches at real distances"""
    import struct
    at = data.index(b"IDAT")

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)
    return data[:at - 4] + chunk(b"IDAT", zlib.compress(zlib.decompress(_idat(data)), level)) + chunk(b"IEND", b"")


INFLATE_BATCHES = (1, 8, 32, 128)


def _inflate_kernel(ctx, dev, files, b, reps):
    """HIP-event time of png_inflate and the kernel's own counts for b files a call"""
    fl = [files[i % len(files)] for i in range(b)]
    ctx.png_decode(fl, to_device=dev, inflate="device")
    ctx.timing_enable(True)
    ms, launches = [], 1
    for _ in range(reps):
        ctx.timing_reset()
        ctx.png_decode(fl, to_device=dev, inflate="device")
        t, launches = ctx.timing_get("png_inflate")
        ms.append(t / b)
    ctx.timing_enable(False)
    st = ctx.png_inflate_stats()
    per_launch_us = float(np.median(ms)) * b / max(1, launches) * 1e3
    return dict(kernel_ms_per_image=spread_of(ms), launches_a_call=int(launches), tokens_per_step=round(st["tokens"] / max(1, st["steps"]), 2),
                bytes_per_us_per_wave=round(st["bytes"] / b / per_launch_us, 2))


def _inflate_section(ctx, dev, small, big, reps, kernel_only=False, sizes=("380x380", "1920x1080"), batches=INFLATE_BATCHES):
    """the device inflate beside the host inflate, in this process and in alternating rounds"""
    from camkifu_amd import capi
    res = dict(geometry=capi.png_inflate_geometry(), contents={},
               note="encoder_default / encoder_runs: files of png_encode in its two modes; zlib_level_6: the same filtered rows deflated by zlib "
                    "level 6.  kernel_ms_per_image: HIP-event time of png_inflate over the images of a call, which run side by side, a wave "
                    "each.  bytes_per_us_per_wave: the bytes of one image over the time of one launch.  variants: the kernel legs of other builds "
                    "(-DCK_PNG_INFLATE_OPL=2 / 4: offsets a lane; -DCK_PNG_INFLATE_SERIAL=1: only lane 0 decodes, one token a step), "
                    "each with its kernel time over this build's (`over_main`).  Frames are left in HBM (to_device) in both modes.")
    for size, frames in (("380x380", small[:32]), ("1920x1080", big[:8])):
        if size not in sizes:
            continue
        default = ctx.png_encode(frames.contiguous(), runs=False)
        sets = {"encoder_default": default, "encoder_runs": ctx.png_encode(frames.contiguous(), runs=True), "zlib_level_6": [_rewrap(d, 6) for d in default]}
        for name, files in sets.items():
            if not np.array_equal(ctx.png_decode(files[:2], inflate="device"), ctx.png_decode(files[:2], inflate="host")):
                raise SystemExit("device inflate: %s %s differs from the host mode" % (size, name))
            leg = dict(file_bytes=int(np.mean([len(d) for d in files])), kernel={}, png_decode_frames_per_s={}, uploaded_bytes_per_frame={})
            for b in batches:
                leg["kernel"]["%d_images_a_call" % b] = _inflate_kernel(ctx, dev, files, b, reps)
            for b in (() if kernel_only else batches):
                fl = [files[i % len(files)] for i in range(b)]
                fps, calls = {"host": [], "device": []}, {}
                for m in fps:
                    t0 = time.perf_counter()
                    ctx.png_decode(fl, to_device=dev, inflate=m)
                    calls[m] = max(1, min(64 // b if b < 64 else 1, int(0.4 / max(1e-6, time.perf_counter() - t0))))
                    leg["uploaded_bytes_per_frame"][m] = int(ctx.png_uploaded_bytes() / b)
                for _ in range(reps):
                    for m in fps:
                        t0 = time.perf_counter()
                        for _ in range(calls[m]):
                            ctx.png_decode(fl, to_device=dev, inflate=m)
                        fps[m].append(b * calls[m] / (time.perf_counter() - t0))
                leg["png_decode_frames_per_s"]["%d_frames_a_call" % b] = {
                    m: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1), rounds=len(v), calls_a_round=calls[m]) for m, v in fps.items()}
            res["contents"].setdefault(size, {})[name] = leg
            print("device_inflate: %s %s done" % (size, name), file=sys.stderr, flush=True)
    return res


def _against_baseline(out, base):
    """the default mode's medians of this run -- sections 3 and 4, measured by the same loops as the baseline's, and the
    `none` legs of the runs section -- against the baseline's [min .. max] of the same quantity: every figure, whether it lies
    inside, and how far the median is from the baseline's median in per cent"""
    rows = []

    def row(what, median, b, lo, hi, mid):
        rows.append(dict(what=what, median=median, baseline_median=b[mid], baseline_min=b[lo], baseline_max=b[hi],
                         inside=bool(b[lo] <= median <= b[hi]), off_pct=round(100.0 * (median - b[mid]) / b[mid], 1)))

    for k, ker in base.get("encoder_kernel_ms_per_frame", {}).items():
        for n, b in ker.items():
            row("section 3, %s %s" % (k, n), out["encoder_kernel_ms_per_frame"][k][n]["median_ms"], b, "min_ms", "max_ms", "median_ms")
            if "runs" in out:
                row("runs section, none, %s %s" % (k, n), out["runs"]["encoder_kernel_ms_per_frame"][k]["none"][n]["median_ms"], b, "min_ms", "max_ms", "median_ms")
    for k, per in base.get("frames_per_s", {}).items():
        for calls, legs in per.items():
            b = legs["png_encode"]
            row("section 4, png_encode %s %s" % (k, calls), out["frames_per_s"][k][calls]["png_encode"]["median"], b, "min", "max", "median")
            if "runs" in out:
                row("runs section, none, png_encode %s %s" % (k, calls), out["runs"]["png_encode_frames_per_s"][k][calls]["none"]["median"], b, "min", "max", "median")
    return dict(rows=rows, outside=[r["what"] for r in rows if not r["inside"]],
                note="the baseline is another build's run of this tool, by --baseline; its spread is that of 5 rounds inside one process, "
                     "so a difference between two processes shows here as `outside` even where the code is the same")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", action="store_true", help="add the `runs` section: the runs mode beside the default mode")
    ap.add_argument("--inflate", action="store_true", help="measure the `device_inflate` section alone: the device inflate beside the host "
                    "inflate; the other sections of the output file stay as they are")
    ap.add_argument("--inflate-variant", help="with --inflate: measure the kernel legs alone and file them under device_inflate.variants "
                    "by this name (a library built with another CK_PNG_INFLATE_OPL, loaded through CK_HIP_LIB)")
    ap.add_argument("--inflate-batches", default="1,8,32,128", help="with --inflate: the images a call to measure")
    ap.add_argument("--inflate-sizes", default="380x380,1920x1080", help="with --inflate: the image sizes to measure")
    ap.add_argument("--baseline", help="the file another build's run of this tool wrote (the parent commit's, say): the default "
                    "mode's figures of this run are listed against its spread under `default_mode_against_baseline`")
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
        if args.inflate:
            sec = _inflate_section(ctx, dev, small, big, args.reps, kernel_only=bool(args.inflate_variant), sizes=args.inflate_sizes.split(","),
                                   batches=tuple(int(b) for b in args.inflate_batches.split(",")))
            before = {}
            if os.path.exists(args.out):
                with open(args.out) as f:
                    before = json.load(f)
            if args.inflate_variant:
                main = before.get("device_inflate", {}).get("contents", {})
                for size, per in sec["contents"].items():     # the variant's kernel time over the shipped build's, leg by leg
                    for name, leg in per.items():
                        ours = main.get(size, {}).get(name, {}).get("kernel", {})
                        leg["over_main"] = {b: round(k["kernel_ms_per_image"]["median_ms"] / ours[b]["kernel_ms_per_image"]["median_ms"], 2)
                                            for b, k in leg["kernel"].items() if b in ours}
                before.setdefault("device_inflate", {}).setdefault("variants", {})[args.inflate_variant] = sec
            else:
                before["device_inflate"] = dict(sec, variants=before.get("device_inflate", {}).get("variants", {}), device=out["device"], rounds=args.reps,
                                                measured="alone, by --inflate: the other sections of this file are from earlier runs of this tool")
            with open(args.out, "w") as f:
                json.dump(before, f, indent=1)
                f.write("\n")
            print(json.dumps(sec))
            return before
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
        # 6. the runs mode beside the default mode
        if args.runs:
            out["runs"] = _runs_section(ctx, dev, small, big, args.reps)
    finally:
        ctx.close()
    if args.baseline:
        with open(args.baseline) as f:
            base = json.load(f)
        out["default_mode_against_baseline"] = dict(_against_baseline(out, base), baseline_file=os.path.basename(args.baseline),
                                                    baseline=dict(encoder_kernel_ms_per_frame=base["encoder_kernel_ms_per_frame"],
                                                                  png_encode_frames_per_s={k: {c: legs["png_encode"] for c, legs in per.items()}
                                                                                           for k, per in base["frames_per_s"].items()}))
    if not args.runs and os.path.exists(args.out):           # a section this run did not measure stays, and says so
        with open(args.out) as f:
            before = json.load(f)
        if "runs" in before:
            out["runs"] = dict(before["runs"], carried_over="from an earlier run of this tool with --runs: not measured with the other sections")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

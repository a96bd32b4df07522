#!/usr/bin/env python3
"""Timing of the Motion-JPEG frame source, in ONE process on one GPU -> profiles/jpeg_timing.json

A filmed game (synth.film) at 1920x1080 is encoded with the project's encoder (Context.jpeg_encode: the bytes Pillow would
write) as baseline JPEG, 4:2:0, quality 90, and held in host memory.
1. host: the Huffman stage alone (capi.jpeg_coefficients), ms per frame -- one frame per call (one thread) and the whole
   batch per call (the library's worker threads, at most 16); warmed up, `--reps` alternating rounds, median / min / max.
2. kernel: ck_jpeg_reconstruct on a batch of coefficients resident in HBM, output preallocated, HIP-event time
   (ck_timing_get("jpeg")) per frame, and the achieved bytes/s against the compulsory 6 * W * H bytes of a 4:2:0 frame
   (int16 coefficients in, BGR out) and the HBM peak.
3. end to end: FastFilePipeline.process_mjpeg on the JPEG film against process_y4m on the same film held as I420 (the path
   that existed before), frames/s in alternating rounds, and the game record of each against the film's moves.
4. device entropy mode (Context.jpeg_set_entropy("device")), on two films from the same frames: one with a restart interval
   of one MCU row, one without restart intervals.  Per frame: the planner on one thread, the bytes uploaded, the Huffman
   kernel and the reconstruct kernel (HIP events); jpeg_decode frames/s in device mode against host mode (16 threads) in
   alternating rounds, for the whole film per call and for smaller calls (the strands per call at which the device mode
   starts to win); process_mjpeg in both modes against process_y4m, with the three game records.
5. "device-spans" entropy mode (parallel decoding inside a restart interval) on the same two films -> "device_spans": the
   HIP-event time of each of its five steps per frame, the shares of Context.jpeg_span_stats, jpeg_decode frames/s at 1, 8,
   32 and 128 frames a call against host mode and against "device" mode in alternating rounds, process_mjpeg against host
   mode and process_y4m with the game records; and on the film without restart intervals a sweep of the span size.
   `--sections device_spans` runs this part alone and keeps the other parts of an existing --out file.

    python tools/jpeg_timing.py [--size 1920x1080] [--film 128] [--n 32] [--reps 7] [--inner 8] [--e2e-reps 5]

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
from ingest_timing import HBM_PEAK, I420Clip, game_quality, i420_of, spread_of  # noqa: E402


class MjpegClip:
    """what process_mjpeg asks of a capture, over JPEG byte strings in host memory; file frame k is clip frame k // 2 (see
    ingest_timing.I420Clip)"""
    path = "<memory>"

    def __init__(self, jpegs, h, w, fps=5.0):
        self.jpegs, self.h, self.w, self.fps = jpegs, h, w, float(fps)

    def __len__(self):
        return 2 * len(self.jpegs)

    def read_raw_batch(self, indices):
        return [self.jpegs[i // 2] for i in indices]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--film", type=int, default=128, help="frames of the filmed game")
    ap.add_argument("--n", type=int, default=32, help="frames per batch of the host and kernel legs")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=8, help="kernel calls per round")
    ap.add_argument("--batch", type=int, default=32, help="frames per pipeline batch")
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--sections", default="all", choices=("all", "device_spans"),
                    help="device_spans: only part 5, merged into the existing --out file")
    ap.add_argument("--spans", default="64,128,256,512,1024", help="span sizes of the sweep, bytes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_timing.json"))
    args = ap.parse_args(argv)
    if args.reps < 5 or args.e2e_reps < 5:
        raise SystemExit("at least 5 alternating rounds per leg")
    import torch
    from camkifu_amd import capi, pipeline, synth
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.stone.nn_manager import NNManager
    w, h = (int(v) for v in args.size.lower().split("x"))
    ctx = capi.Context(0)
    dev = torch.device("cuda", 0)
    F, n = args.film, min(args.n, args.film)
    out = dict(tool="tools/jpeg_timing.py", device=torch.cuda.get_device_name(0),
               plan=dict(height=h, width=w, sampling="4:2:0", quality=args.quality, film_frames=F, batch=n, rounds=args.reps,
                         kernel_calls_per_round=args.inner, e2e_rounds=args.e2e_reps, pipeline_batch=args.batch))
    film, corners, truth, moves, hands = synth.film(F, h, w, seed=synth.SEED, device=dev, quiet=52, move_every=32, hand_frames=12)
    i420 = torch.empty((F, h * w * 3 // 2), dtype=torch.uint8).pin_memory()
    jpegs, jpegs_row = [], []
    mcux = -(-w // 16)
    for b0 in range(0, F, 8):
        part = film[b0:b0 + 8]
        i420[b0:b0 + 8].copy_(i420_of(part))
        jpegs += [np.frombuffer(j, np.uint8) for j in ctx.jpeg_encode(part.contiguous(), quality=args.quality, sampling=capi.CK_JPEG_420)]
        jpegs_row += [np.frombuffer(j, np.uint8) for j in ctx.jpeg_encode(part.contiguous(), quality=args.quality,
                                                                          sampling=capi.CK_JPEG_420, restart_interval=mcux)]
    del film
    torch.cuda.empty_cache()
    out["plan"]["jpeg_bytes_per_frame"] = int(np.mean([j.size for j in jpegs]))
    only_spans = args.sections == "device_spans"
    if only_spans and os.path.exists(args.out):
        with open(args.out) as f:
            kept = json.load(f)
        kept["device_spans_run"] = dict(tool=out["tool"], device=out["device"], plan=out["plan"])
        out = kept

    def parts_1_to_4():
        # 1. host
        batch = jpegs[:n]
        capi.jpeg_coefficients(batch)
        capi.jpeg_coefficients(batch[:1])
        one, many = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for j in batch:
                capi.jpeg_coefficients([j])
            one.append((time.perf_counter() - t0) * 1e3 / n)
            t0 = time.perf_counter()
            capi.jpeg_coefficients(batch)
            many.append((time.perf_counter() - t0) * 1e3 / n)
        out["host_entropy_decode"] = dict(one_thread_ms_per_frame=spread_of(one), sixteen_threads_ms_per_frame=spread_of(many),
                                          cpus_seen=os.cpu_count(),
                                          note="includes the allocation of the coefficient array of each call")
        # 2. kernel
        info, coef, quant = capi.jpeg_coefficients(batch)
        d_coef, d_quant = torch.from_numpy(coef).to(dev), torch.from_numpy(quant.view(np.int16)).to(dev)
        bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        for _ in range(3):
            ctx.jpeg_reconstruct(d_coef, d_quant, h, w, info["sampling"], out=bgr)
        same = bool(np.array_equal(bgr[:2].cpu().numpy(), ctx.jpeg_decode(batch[:2])))
        ctx.timing_enable(True)
        ms = []
        for _ in range(args.reps):
            ctx.timing_reset()
            for _ in range(args.inner):
                ctx.jpeg_reconstruct(d_coef, d_quant, h, w, info["sampling"], out=bgr)
            ms.append(ctx.timing_get("jpeg")[0] / (args.inner * n))
        ctx.timing_enable(False)
        s = spread_of(ms)
        floor = 6 * w * h
        moved = info["blocks"] * 128 + h * w * 3
        out["kernel"] = dict(per_frame=s, floor_bytes_per_frame=floor, bytes_per_frame_with_mcu_padding=moved,
                             gb_per_s_against_floor=round(floor / (s["median_ms"] * 1e-3) / 1e9, 1),
                             share_of_hbm_peak=round(floor / (s["median_ms"] * 1e-3) / HBM_PEAK, 4), two_halves_equal_decode=same)
        del d_coef, d_quant, bgr
        torch.cuda.empty_cache()
        # 3. end to end
        ctx.cnn_set_weights(NNManager.init_net())
        clips = dict(mjpeg=MjpegClip(jpegs, h, w), y4m=I420Clip(i420.numpy(), h, w))

        def run(kind):
            p = pipeline.FastFilePipeline(h, w, ControllerHeadless(), ctx=ctx)
            try:
                t0 = time.perf_counter()
                reqs = (p.process_mjpeg if kind == "mjpeg" else p.process_y4m)(clips[kind], batch=args.batch)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, reqs, p.mtx is not None
            finally:
                p.close()
        first = {k: run(k) for k in clips}
        secs = {k: [] for k in clips}
        for _ in range(args.e2e_reps):
            for k in clips:
                secs[k].append(run(k)[0])
        res = {}
        for k in clips:
            fps = sorted(F / t for t in secs[k])
            res[k] = dict(frames_per_s=dict(median=round(float(np.median(fps)), 1), min=round(fps[0], 1), max=round(fps[-1], 1),
                                            spread=round((fps[-1] - fps[0]) / float(np.median(fps)), 4), rounds=len(fps)),
                          board_found=bool(first[k][2]), game_record=game_quality(first[k][1], truth, moves, F))
        res["mjpeg_over_y4m"] = round(res["mjpeg"]["frames_per_s"]["median"] / res["y4m"]["frames_per_s"]["median"], 3)
        host_fps = 1e3 / out["host_entropy_decode"]["sixteen_threads_ms_per_frame"]["median_ms"]
        res["host_entropy_frames_per_s"] = round(host_fps, 1)
        res["host_entropy_bounds_the_rate"] = bool(host_fps < 1.5 * res["mjpeg"]["frames_per_s"]["median"])
        out["end_to_end"] = res
        print("host entropy, kernel, end to end: done", flush=True)
        # 4. the device entropy mode on both films
        bgr = torch.empty((F, h, w, 3), dtype=torch.uint8, device=dev)
        dev_out = {}
        for film_name, js in (("restart_row", jpegs_row), ("no_restart", jpegs)):
            rows, sets = capi.jpeg_plan(js)
            plan_ms = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                capi.jpeg_plan(js)
                plan_ms.append((time.perf_counter() - t0) * 1e3 / F)
            leg = dict(strands_per_frame=rows.shape[0] / F, table_sets=sets, jpeg_bytes_per_frame=int(np.mean([j.size for j in js])),
                       planner_one_thread_ms_per_frame=spread_of(plan_ms))
            ctx.jpeg_set_entropy("host")
            want = ctx.jpeg_decode(js[:2])
            ctx.jpeg_decode(js, out=bgr)
            leg["bytes_uploaded_per_frame_host_mode"] = ctx.jpeg_uploaded_bytes() // F
            ctx.jpeg_set_entropy("device")
            leg["equal_to_host_mode"] = bool(np.array_equal(ctx.jpeg_decode(js[:2]), want))
            ctx.jpeg_decode(js, out=bgr)
            leg["bytes_uploaded_per_frame"] = ctx.jpeg_uploaded_bytes() // F          # (what the call staged: ck_jpeg_uploaded_bytes)
            ctx.timing_enable(True)
            huff, recon = [], []
            for _ in range(args.reps):
                ctx.timing_reset()
                ctx.jpeg_decode(js, out=bgr)
                huff.append(ctx.timing_get("jpeg_huff")[0] / F)
                recon.append(ctx.timing_get("jpeg")[0] / F)
            ctx.timing_enable(False)
            leg["entropy_kernel_ms_per_frame"] = spread_of(huff)
            leg["reconstruct_kernel_ms_per_frame"] = spread_of(recon)

            def decode_fps(mode, count):
                ctx.jpeg_set_entropy(mode)
                t0 = time.perf_counter()
                for b0 in range(0, F, count):
                    ctx.jpeg_decode(js[b0:b0 + count], out=bgr[:len(js[b0:b0 + count])])
                torch.cuda.synchronize()
                return F / (time.perf_counter() - t0)
            by_batch = []
            # (a film without restart intervals has one strand per frame: one lane each, so only the ends of the range)
            for count in [c for c in ((1, 2, 4, 8, 16, 32, 64) if film_name == "restart_row" else (1,)) if c < F] + [F]:
                fps = dict(host=[], device=[])
                for mode in fps:
                    decode_fps(mode, count)
                for _ in range(args.e2e_reps):
                    for mode in fps:
                        fps[mode].append(decode_fps(mode, count))
                hm, dm = float(np.median(fps["host"])), float(np.median(fps["device"]))
                by_batch.append(dict(frames_per_call=count, strands_per_call=int(round(count * rows.shape[0] / F)),
                                     host_frames_per_s=round(hm, 1), device_frames_per_s=round(dm, 1), device_over_host=round(dm / hm, 3)))
            leg["jpeg_decode_by_frames_per_call"] = by_batch
            leg["jpeg_decode_whole_film_device_over_host"] = by_batch[-1]["device_over_host"]
            wins = [b["strands_per_call"] for b in by_batch if b["device_over_host"] > 1.0]
            leg["device_wins_from_strands_per_call"] = min(wins) if wins else None
            # process_mjpeg in both modes against process_y4m
            clips = dict(host=MjpegClip(js, h, w), device=MjpegClip(js, h, w), y4m=I420Clip(i420.numpy(), h, w))

            def run2(kind):
                p = pipeline.FastFilePipeline(h, w, ControllerHeadless(), ctx=ctx)
                try:
                    t0 = time.perf_counter()
                    if kind == "y4m":
                        reqs = p.process_y4m(clips[kind], batch=args.batch)
                    else:
                        reqs = p.process_mjpeg(clips[kind], batch=args.batch, entropy=kind)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, reqs
                finally:
                    p.close()
            first2 = {k: run2(k) for k in clips}
            secs2 = {k: [] for k in clips}
            for _ in range(args.e2e_reps):
                for k in clips:
                    secs2[k].append(run2(k)[0])
            e2e = {}
            for k in clips:
                fps = sorted(F / t for t in secs2[k])
                e2e[k] = dict(frames_per_s=dict(median=round(float(np.median(fps)), 1), min=round(fps[0], 1), max=round(fps[-1], 1),
                                                rounds=len(fps)), game_record=game_quality(first2[k][1], truth, moves, F))
            e2e["device_over_y4m"] = round(e2e["device"]["frames_per_s"]["median"] / e2e["y4m"]["frames_per_s"]["median"], 3)
            e2e["host_over_y4m"] = round(e2e["host"]["frames_per_s"]["median"] / e2e["y4m"]["frames_per_s"]["median"], 3)
            e2e["device_over_host"] = round(e2e["device"]["frames_per_s"]["median"] / e2e["host"]["frames_per_s"]["median"], 3)
            leg["process_mjpeg"] = e2e
            ctx.jpeg_set_entropy("host")
            dev_out[film_name] = leg
            print("device entropy, %s: done" % film_name, flush=True)
        out["device_entropy"] = dev_out

    def part_5():
        # 5. parallel decoding inside a restart interval
        if only_spans:
            ctx.cnn_set_weights(NNManager.init_net())                  # (part 3 does it otherwise)
        bgr = torch.empty((F, h, w, 3), dtype=torch.uint8, device=dev)
        STEPS = ("jpeg_span_speculate", "jpeg_span_resolve", "jpeg_span_write", "jpeg_span_dc", "jpeg_span_verdict", "jpeg_huff", "jpeg")
        modes = ("host", "device", "device-spans")

        def decode_fps(js, mode, count):
            ctx.jpeg_set_entropy(mode)
            t0 = time.perf_counter()
            for b0 in range(0, F, count):
                ctx.jpeg_decode(js[b0:b0 + count], out=bgr[:len(js[b0:b0 + count])])
            torch.cuda.synchronize()
            return F / (time.perf_counter() - t0)

        def step_times(js, span):
            ctx.jpeg_set_entropy("device-spans")
            ctx.jpeg_set_span_bytes(span)
            ctx.jpeg_decode(js, out=bgr)
            st = ctx.jpeg_span_stats()
            ctx.timing_enable(True)
            ms = {k: [] for k in STEPS}
            for _ in range(args.reps):
                ctx.timing_reset()
                ctx.jpeg_decode(js, out=bgr)
                for k in STEPS:
                    ms[k].append(ctx.timing_get(k)[0] / F)
            ctx.timing_enable(False)
            never = dict(median_ms=0.0, min_ms=0.0, max_ms=0.0, spread=0.0)        # (jpeg_huff: no suspect strand, no launch)
            return st, {k: spread_of(v) if min(v) > 0 else dict(never, rounds=len(v)) for k, v in ms.items()}

        span_out = dict(default_span_bytes=capi.jpeg_span_bytes())
        for film_name, js in (("restart_row", jpegs_row), ("no_restart", jpegs)):
            ctx.jpeg_set_entropy("host")
            want = ctx.jpeg_decode(js[:2])
            ctx.jpeg_set_span_bytes(capi.jpeg_span_bytes())
            st, steps = step_times(js, capi.jpeg_span_bytes())
            leg = dict(jpeg_bytes_per_frame=int(np.mean([j.size for j in js])),
                       equal_to_host_mode=bool(np.array_equal(ctx.jpeg_decode(js[:2]), want)),
                       bytes_uploaded_per_frame=ctx.jpeg_uploaded_bytes() // 2,
                       kernel_ms_per_frame=steps,
                       entropy_kernels_ms_per_frame=round(sum(steps[k]["median_ms"] for k in STEPS[:6]), 4),
                       span_stats=dict(st, spans_per_frame=round(st["spans"] / F, 1),
                                       unresolved_share=round(st["unresolved"] / max(1, st["spans"]), 5)))
            by_batch = []
            for count in [c for c in (1, 8, 32, 128) if c <= F]:
                fps = {m: [] for m in modes}
                for m in modes:
                    decode_fps(js, m, count)
                for _ in range(args.e2e_reps):
                    for m in modes:
                        fps[m].append(decode_fps(js, m, count))
                med = {m: float(np.median(v)) for m, v in fps.items()}
                by_batch.append(dict(frames_per_call=count,
                                     frames_per_s={m: dict(median=round(med[m], 1), min=round(min(fps[m]), 1), max=round(max(fps[m]), 1))
                                                   for m in modes},
                                     spans_over_host=round(med["device-spans"] / med["host"], 3),
                                     spans_over_device=round(med["device-spans"] / med["device"], 3),
                                     winner=max(modes, key=lambda m: med[m])))
                print("device-spans entropy, %s, %d frames a call: done" % (film_name, count), flush=True)
            leg["jpeg_decode_by_frames_per_call"] = by_batch
            clips = {"host": MjpegClip(js, h, w), "device-spans": MjpegClip(js, h, w), "y4m": I420Clip(i420.numpy(), h, w)}

            def run3(kind):
                p = pipeline.FastFilePipeline(h, w, ControllerHeadless(), ctx=ctx)
                try:
                    t0 = time.perf_counter()
                    if kind == "y4m":
                        reqs = p.process_y4m(clips[kind], batch=args.batch)
                    else:
                        reqs = p.process_mjpeg(clips[kind], batch=args.batch, entropy=kind)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0, reqs
                finally:
                    p.close()
            first3 = {k: run3(k) for k in clips}
            secs3 = {k: [] for k in clips}
            for _ in range(args.e2e_reps):
                for k in clips:
                    secs3[k].append(run3(k)[0])
            e2e = dict(pipeline_batch=args.batch)
            for k in clips:
                fps = sorted(F / t for t in secs3[k])
                e2e[k] = dict(frames_per_s=dict(median=round(float(np.median(fps)), 1), min=round(fps[0], 1), max=round(fps[-1], 1),
                                                rounds=len(fps)), game_record=game_quality(first3[k][1], truth, moves, F))
            e2e["spans_over_host"] = round(e2e["device-spans"]["frames_per_s"]["median"] / e2e["host"]["frames_per_s"]["median"], 3)
            e2e["spans_over_y4m"] = round(e2e["device-spans"]["frames_per_s"]["median"] / e2e["y4m"]["frames_per_s"]["median"], 3)
            e2e["same_game_record_as_host"] = bool(e2e["device-spans"]["game_record"] == e2e["host"]["game_record"])
            leg["process_mjpeg"] = e2e
            if film_name == "no_restart":
                sweep = []
                for span in [int(v) for v in args.spans.split(",")]:
                    st, steps = step_times(js, span)
                    fps = dict()
                    for count in [c for c in (32, 128) if c <= F]:
                        decode_fps(js, "device-spans", count)
                        fps[count] = [decode_fps(js, "device-spans", count) for _ in range(args.e2e_reps)]
                    sweep.append(dict(span_bytes=span, spans_per_frame=round(st["spans"] / F, 1),
                                      unresolved_share=round(st["unresolved"] / max(1, st["spans"]), 5),
                                      kernel_ms_per_frame={k: steps[k]["median_ms"] for k in STEPS[:5]},
                                      entropy_kernels_ms_per_frame=round(sum(steps[k]["median_ms"] for k in STEPS[:5]), 4),
                                      jpeg_decode_frames_per_s={str(c): dict(median=round(float(np.median(v)), 1), min=round(min(v), 1),
                                                                             max=round(max(v), 1)) for c, v in fps.items()}))
                leg["span_size_sweep"] = sweep
                leg["fastest_span_bytes_by_kernel_time"] = min(sweep, key=lambda r: r["entropy_kernels_ms_per_frame"])["span_bytes"]
                ctx.jpeg_set_span_bytes(capi.jpeg_span_bytes())
            ctx.jpeg_set_entropy("host")
            span_out[film_name] = leg
            print("device-spans entropy, %s: done" % film_name, flush=True)
        out["device_spans"] = span_out

    try:
        if not only_spans:
            parts_1_to_4()
        part_5()
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

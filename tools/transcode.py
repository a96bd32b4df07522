#!/usr/bin/env python3
"""Write a film as Motion-JPEG: frames are encoded on the GPU (capi.Context.jpeg_encode: the forward kernel, then the
Huffman coder on the host's worker threads or, with --encode-entropy device, on the GPU as well: the same bytes) and
appended to an .avi through core.capture.MjpegWriter.

    python tools/transcode.py SRC OUT.avi [--quality Q] [--sampling 420|422|444|grey] [--batch N] [--encode-entropy host|device]
                              [--optimize]
    python tools/transcode.py SRC OUT.avi --gobans [--annotate] [--sgf game.sgf]
    python tools/transcode.py SRC OUT.avi --annotate [--sgf game.sgf]

SRC is anything core.capture.open_capture takes: a .y4m file, a Motion-JPEG .avi, a .npy file of (n, h, w, 3) BGR frames.
Every frame of SRC goes into OUT, at SRC's frame rate; a .y4m or .avi is converted / decoded straight into HBM and encoded
from there.  --optimize fits the Huffman tables to every frame (libjpeg's optimize_coding): the same pixels, a smaller file.

--gobans records what the stones finder saw instead: SRC runs through a one-rank FastFilePipeline (a file thinned to
cvconf.file_fps, as every run of a file is) and each batch's canonical 380 x 380 goban images are encoded while they are
still in HBM.  OUT then holds one 380 x 380 frame per processed frame; frames of a batch that had no board transform yet
(nothing was warped) are black.  With --sgf the record of the run is checked against the reference game and the match line
of tools/detectiontest.py is printed.

--annotate draws what the finders concluded onto the frames before they are encoded, on the GPU, one overlay_draw per batch
(core/annotate.py builds the lists, csrc/k_overlay.hip rasterises them).  With --gobans each goban image gets the grid, the
stones of the game position after that frame, the agitated zones in translucent red, "Frame i/N" and the moves the frame
emitted.  Without --gobans every ANALYSED frame of SRC is written at full size with the board's corners and hull in force
after its batch, the 361 intersections projected back into the frame, the stones on top and the same two lines of text;
frames before the first detection carry only the text.  There is no CPU fallback: without a GPU the first device call
raises."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLINGS = {"grey": 0, "444": 1, "422": 2, "420": 3}
GOBAN = 380


def _frames_of(capture, ctx, batch):
    """batches of BGR frames of an open capture, in HBM where the source is a file"""
    import torch
    from camkifu_amd.core.capture import AviMjpegCapture, Y4MCapture
    if isinstance(capture, (Y4MCapture, AviMjpegCapture)):
        dev = torch.device("cuda", getattr(ctx, "device", 0))
        for b0 in range(0, len(capture), batch):
            idx = list(range(b0, min(len(capture), b0 + batch)))
            raw = capture.read_raw_batch(idx)
            if isinstance(capture, Y4MCapture):
                yield ctx.i420_to_bgr(raw, capture.h, capture.w, to_device=dev)
            else:
                if any(r is None for r in raw):
                    raise SystemExit("frame %d of %s: no good frame before it" % (idx[[r is None for r in raw].index(True)], capture.path))
                yield ctx.jpeg_decode(raw, to_device=dev)
    else:
        frames = capture.frames
        for b0 in range(0, len(frames), batch):
            yield np.ascontiguousarray(frames[b0:b0 + batch])


def restart_mcus(restart, w, sampling):
    """--restart as MCUs between restart markers: a number, or "row" for one MCU row of a film of width w"""
    if restart in (None, "", 0, "0"):
        return 0
    if restart == "row":
        return -(-int(w) // (16 if sampling >= 2 else 8))          # (4:2:2 and 4:2:0 have MCUs of 16 pixels across)
    n = int(restart)
    if not 0 <= n <= 65535:
        raise SystemExit("--restart: 0 .. 65535 MCUs, or 'row'")
    return n


def transcode(src, out, quality=90, sampling=3, batch=64, ctx=None, restart=0, optimize=False):
    """restart: MCUs between restart markers, or "row"; optimize: Huffman tables fitted to every frame
    -> dict(frames, bytes, h, w, fps)"""
    from camkifu_amd import capi
    from camkifu_amd.core.capture import CAP_PROP_FPS, MjpegWriter, open_capture
    ctx = ctx if ctx is not None else capi.get_context()
    capture = open_capture(np.load(src, mmap_mode="r") if isinstance(src, str) and src.lower().endswith(".npy") else src)
    if not capture.isOpened():
        raise SystemExit("cannot open %r: %s" % (src, getattr(capture, "error", "")))
    if hasattr(capture, "frames"):
        h, w = capture.frames.shape[1:3]
    else:
        h, w = capture.h, capture.w
    fps = capture.get(CAP_PROP_FPS) or 30.0
    with MjpegWriter(out, h, w, fps=fps, quality=quality, sampling=sampling, encode=ctx.jpeg_encode,
                     restart_interval=restart_mcus(restart, w, sampling), optimize=optimize) as wr:
        for frames in _frames_of(capture, ctx, batch):
            wr.write(frames)
    return dict(frames=wr.frames, bytes=os.path.getsize(out), h=int(h), w=int(w), fps=float(fps))


def _own_copy(frames):
    """a copy the annotation may draw on, in the memory the frames are in"""
    return frames.clone() if hasattr(frames, "clone") else np.array(frames, np.uint8, order="C")


def record_gobans(src, out, quality=90, sampling=3, batch=64, ctx=None, controller=None, fps=None, annotate=False,
                  full_frames=False, **pipe_args):
    """the film `src` (a path, an open capture, or an array of frames, every one of which is processed) through a one-rank
    pipeline, its goban images into `out` -> dict(frames, bytes, requests): `requests` is what the fold emitted.
    annotate: what the finders concluded is drawn onto each batch before it is encoded (module docstring), one
    overlay_draw per batch on the tensor that goes to the writer.  full_frames (with annotate): the analysed frames
    themselves are written, annotated, instead of the goban images."""
    from camkifu_amd import capi, cvconf
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.core import annotate as ann
    from camkifu_amd.core.capture import AviMjpegCapture, MjpegWriter, Y4MCapture, file_frame_indices, open_capture
    from camkifu_amd.pipeline import FastFilePipeline
    from camkifu_amd.stone.harvest import replay
    from camkifu_amd.stone.stonesfinder import PosGrid
    ctx = ctx if ctx is not None else capi.get_context()
    controller = controller if controller is not None else ControllerHeadless()
    capture = src
    if isinstance(src, str):
        capture = open_capture(np.load(src, mmap_mode="r") if src.lower().endswith(".npy") else src)
        if not capture.isOpened():
            raise SystemExit("cannot open %r: %s" % (src, getattr(capture, "error", "")))
    is_file = isinstance(capture, (Y4MCapture, AviMjpegCapture))
    frames = None if is_file else getattr(capture, "frames", capture)
    h, w = (capture.h, capture.w) if is_file else frames.shape[1:3]
    if fps is None:
        fps = float(getattr(cvconf, "file_fps", 0) or 5.0) if is_file else 30.0
    if full_frames and not annotate:
        raise ValueError("full_frames is the annotated film of the analysed frames: it needs annotate=True")
    black = np.zeros((1, GOBAN, GOBAN, 3), np.uint8)
    oh, ow = (h, w) if full_frames else (GOBAN, GOBAN)
    wr = MjpegWriter(out, oh, ow, fps=fps, quality=quality, sampling=sampling, encode=ctx.jpeg_encode)
    total = len(file_frame_indices(len(capture), capture.fps, None)) if is_file else len(frames)
    mirror = ControllerHeadless(rules=getattr(controller, "rules", None) is not None)     # the requests replayed: the position per frame
    grid, done = PosGrid(GOBAN), [0]

    def lists_of(pipe, emitted, n_total):
        """one display list per frame of the batch"""
        codes = replay(mirror, emitted)
        fg = pipe.last_fgcount
        out_lists = []
        for f in range(n_total):
            no, said = done[0] + f + 1, ann.moves_text(emitted[f])
            if full_frames:
                out_lists.append(ann.frame_list((h, w), pipe.board.finder.corners, pipe.board.mtx, codes[f], grid, no, total, said))
            else:
                out_lists.append(ann.goban_list(codes[f], None if fg is None else fg[f], grid, no, total, said))
        done[0] += n_total
        return out_lists

    class _Pipe(FastFilePipeline):                               # hooked the way stone/harvest.py hooks it
        def process_batch(self, my_frames, n_total):
            emitted = FastFilePipeline.process_batch(self, my_frames, n_total)
            gobans = my_frames if full_frames else self.last_gobans
            if gobans is None:                                   # no transform yet: nothing was warped
                gobans = np.broadcast_to(black, (n_total, GOBAN, GOBAN, 3))
            if annotate:                                         # drawn where the images are; pipeline's own stay as they were
                gobans = ctx.overlay_draw(_own_copy(gobans), lists_of(self, emitted, n_total))
            wr.write(gobans)                                    # (still in HBM when the frames were)
            return emitted

    emitted = []
    try:
        with _Pipe(h, w, controller, ctx=ctx, keep_gobans=True, **pipe_args) as pipe:
            if isinstance(capture, Y4MCapture):
                emitted = pipe.process_y4m(capture, batch=batch)
            elif isinstance(capture, AviMjpegCapture):
                emitted = pipe.process_mjpeg(capture, batch=batch)
            else:
                for b0 in range(0, len(frames), batch):
                    part = np.ascontiguousarray(frames[b0:b0 + batch])
                    emitted += pipe.process_batch(part, len(part))
    finally:
        wr.close()
    return dict(frames=wr.frames, bytes=os.path.getsize(out), requests=emitted, controller=controller)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("out")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--sampling", choices=sorted(SAMPLINGS), default="420")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--restart", default="0", metavar="N|row", help="restart markers every N MCUs, or every MCU row: the pieces "
                    "the device entropy mode decodes in parallel (plain transcoding only)")
    ap.add_argument("--encode-entropy", choices=("host", "device"), default="host", help="where the encoder's Huffman stage "
                    "runs: the host's worker threads, or the GPU (only the finished streams come down); the bytes are the same")
    ap.add_argument("--optimize", action="store_true", help="Huffman tables fitted to every frame (libjpeg's optimize_coding): "
                    "the same pixels in a smaller file, in either entropy mode")
    ap.add_argument("--gobans", action="store_true", help="record the 380x380 goban images of a pipeline run instead of the frames")
    ap.add_argument("--annotate", action="store_true", help="draw what the finders concluded onto the frames, on the GPU; "
                    "without --gobans the analysed frames are written at full size")
    ap.add_argument("--sgf", help="with --gobans or --annotate: the reference game the run's record is checked against")
    args = ap.parse_args(argv)
    if not args.out.lower().endswith(".avi"):
        raise SystemExit("the output is a Motion-JPEG .avi file")
    sampling = SAMPLINGS[args.sampling]
    from camkifu_amd import capi
    ctx = capi.get_context()
    ctx.jpeg_set_encode_entropy(args.encode_entropy)
    ctx.jpeg_set_encode_tables("optimised" if args.optimize else "standard")
    if not args.gobans and not args.annotate:
        res = transcode(args.src, args.out, args.quality, sampling, args.batch, ctx=ctx, restart=args.restart, optimize=args.optimize)
        print("%s: %d frames of %dx%d at %.3g fps, %d bytes" % (args.out, res["frames"], res["w"], res["h"], res["fps"], res["bytes"]))
        return res
    import time
    from camkifu_amd.stone.nn_manager import NNManager
    ctx.cnn_set_weights(NNManager.get_net())
    t0 = time.time()
    res = record_gobans(args.src, args.out, args.quality, sampling, args.batch, ctx=ctx, annotate=args.annotate,
                        full_frames=not args.gobans)
    print("%s: %d %s, %d bytes" % (args.out, res["frames"], "goban images" if args.gobans else "annotated frames", res["bytes"]))
    if args.sgf:
        from camkifu_amd.golib_shim import Kifu
        from camkifu_amd.kifu_checker import KifuChecker, report
        matcher = KifuChecker(Kifu(sgffile=args.sgf)).check(res["controller"].kifu)
        print(report(os.path.basename(args.src), matcher, time.time() - t0))
    return res


if __name__ == "__main__":
    main()

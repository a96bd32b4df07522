#!/usr/bin/env python3
"""Time the harvest of training data on the GPU -> profiles/harvest_timing.json.

One process, one rendered film of a game at 1920 x 1080 (synth.film: hands, new stones), its frames in HBM, batches of
--batch frames.  One untimed pass warms the library up (code objects, scratch buffers); then, each on a fresh pipeline whose
first frames find the board, the whole film goes through twice:
    pipeline    FastFilePipeline.process_batch alone (keep_gobans off): frames/s
    harvest     Harvester.feed -- the same pipeline with keep_gobans on, the requests replayed, label_windows and
                ck_harvest_patches per batch: frames/s, patches kept, kernel time of flag + scan + gather per batch (the
                library's event bracket "harvest")
and 1000 patches in HBM go through ck_augment_patches: kernel time per 1000 patches (bracket "augment").
No threshold is attached to any of these numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harvest_timing.json"))
    a = ap.parse_args(argv)
    import torch
    from camkifu_amd import capi, pipeline, synth
    from camkifu_amd.controller import ControllerHeadless
    from camkifu_amd.stone.harvest import Harvester
    from camkifu_amd.stone.nn_manager import NNManager
    h, w, quiet = 1080, 1920, 8
    frames, corners, truth, moves, _hands = synth.film(a.frames, h, w, seed=8, quiet=quiet, move_every=30, hand_frames=12)
    sym = "EBW"
    game = [(sym[truth[quiet - 2][r, c]], r, c) for r in range(19) for c in range(19) if truth[quiet - 2][r, c]]
    game += [(sym[col], r, c) for col, r, c, f in moves]
    dev = torch.device("cuda", 0)
    frames = frames.to(dev)
    ctx = capi.Context(0)
    ctx.cnn_set_weights(NNManager.init_net())
    out = dict(frame=[h, w], frames=a.frames, batch=a.batch)

    def film_through(feed):
        feed(frames[:quiet])                                   # finds the board
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b0 in range(0, a.frames, a.batch):
            feed(frames[b0:b0 + a.batch])
        return a.frames / (time.perf_counter() - t0)

    for leg in ("warm_up", "pipeline_frames_per_s"):
        pipe = pipeline.FastFilePipeline(h, w, ControllerHeadless(), ctx=ctx, bg_init_frames=quiet - 2)
        try:
            rate = film_through(lambda fr: pipe.process_batch(fr, len(fr)))
        finally:
            pipe.close()
        if leg != "warm_up":
            out[leg] = round(rate, 1)
    hv = Harvester(h, w, game, ctx=ctx, bg_init_frames=quiet - 2)
    try:
        ctx.timing_enable(True)
        ctx.timing_reset()
        out["harvest_frames_per_s"] = round(film_through(hv.feed), 1)
        ms, calls = ctx.timing_get("harvest")
        data = hv.dataset()
        out.update(harvest_kernel_ms_per_batch=round(ms / max(calls, 1), 4), harvest_calls=calls, patches=int(len(data["X"])),
                   frames_harvested=len(set(data["frame"].tolist())), states=sorted(set(int(k) for k in data["state"])))
    finally:
        hv.close()
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1000, 40, 40, 3), dtype=np.uint8)).to(dev)
    t = np.arange(1000) % 8
    ctx.augment_patches(x, t)
    ctx.timing_reset()
    for _ in range(10):
        ctx.augment_patches(x, t)
    out["augment_kernel_ms_per_1000"] = round(ctx.timing_get("augment")[0] / 10, 4)
    ctx.timing_enable(False)
    ctx.close()
    print(json.dumps(out, sort_keys=True))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

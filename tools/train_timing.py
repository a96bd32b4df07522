#!/usr/bin/env python3
"""Time the classifier's training step on the GPU and the same steps in torch on the CPU -> profiles/train_timing.json.

One process.  Per batch size (1000, 128): ms per step and patches/s of ck_train_step (wall clock around the call, the
patches already in HBM, dropout on), the kernel time of its four stages from the library's event brackets (train_fwd:
forward and loss; train_dgrad: data gradients, pools included; train_wgrad: weight and bias gradients with their
reductions; train_adam), and ms per step of the float32 torch network of tests/train_ref.py with torch.optim.Adam on 16
CPU threads.  No threshold is attached to any of these numbers."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("train_fwd", "train_dgrad", "train_wgrad", "train_adam")


def gpu_steps(ctx, W, x, y, steps, warmup):
    import torch
    h = ctx.train_create(W)
    xd = torch.from_numpy(x).cuda()
    try:
        for _ in range(warmup):
            ctx.train_step(h, xd, y, dropout=True, seed=1)
        ctx.timing_enable(True)
        ctx.timing_reset()
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.train_step(h, xd, y, dropout=True, seed=1)
        wall = (time.perf_counter() - t0) / steps * 1e3
        stages = {s: ctx.timing_get(s)[0] / steps for s in STAGES}
        ctx.timing_enable(False)
    finally:
        ctx.train_destroy(h)
    return wall, stages


def cpu_steps(W, x, y, steps, warmup):
    import torch
    import torch.nn.functional as F
    from tests import train_ref
    torch.set_num_threads(16)
    w = train_ref.tensors(W, torch.float32, grad=True)
    opt = torch.optim.Adam(list(w.values()), lr=0.001)
    labels = torch.from_numpy(y.astype(np.int64))
    rng = np.random.default_rng(0)
    t0 = 0.0
    for k in range(warmup + steps):
        if k == warmup:
            t0 = time.perf_counter()
        masks = [(rng.random((len(x),) + s) >= p).astype(np.float32) for s, p in (((16, 16, 32), .25), ((6, 6, 90), .25), ((160,), .5))]
        loss = F.cross_entropy(train_ref.logits(w, x, masks), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    from camkifu_amd import capi, synth
    from tests import train_cases
    X, Y = train_cases.pool()
    pick = np.random.default_rng(0).integers(0, len(X), 1000)
    X, Y = np.ascontiguousarray(X[pick]), np.ascontiguousarray(Y[pick])
    W = synth.cnn_weights()
    ctx = capi.Context(0)
    out = {}
    for n, steps, cpu in ((1000, 10, 2), (128, 20, 4)):
        wall, stages = gpu_steps(ctx, W, X[:n], Y[:n], steps, 2)
        ref = cpu_steps(W, X[:n], Y[:n], cpu, 1)
        out["batch_%d" % n] = dict(ms_per_step=round(wall, 3), patches_per_s=round(n / wall * 1e3, 1),
                                   kernel_ms={s: round(v, 3) for s, v in stages.items()},
                                   torch_cpu16_ms_per_step=round(ref, 1), torch_cpu16_patches_per_s=round(n / ref * 1e3, 1))
        print(n, out["batch_%d" % n], flush=True)
    ctx.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "train_timing.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The flat optimizer alone at the wide path's size: two rows of the W=4096, depth-4
parameter count (P = 67,141,633: odd, so row 1 is off a 16-byte boundary).

  unclipped : FlatOptimizer(OptimConfig())
  clipped   : FlatOptimizer(OptimConfig(max_grad_norm=...)): norm launch + clipped update
  torchclip : torch.nn.utils.clip_grad_norm_ per row, then the unclipped kernel

The bounds never bind, so every mode leaves the same parameters.  Device events around
--steps steps per window, --windows windows per mode, the modes' windows interleaved.
Imports the package of the current directory, so one checkout can be timed against
another: run it from each tree's root in turn.

usage: python scripts/bench_flat_optim.py MODE[,MODE...] [--windows N] [--steps N]"""
import json, os, sys
sys.path.insert(0, os.getcwd())
import torch
from distributed_training_pytorch_amd.ops.optim import FlatOptimizer, OptimConfig

W, D = int(os.environ.get("OPT_W", 4096)), 4
P = 2 * W + W + D * (W * W + W) + W + 1
modes = sys.argv[1].split(",")
windows = int(sys.argv[sys.argv.index("--windows") + 1]) if "--windows" in sys.argv else 3
steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else 10
dev = torch.device(os.environ.get("OPT_DEV", "cuda:0"))
g = torch.Generator(device=dev).manual_seed(0)
params = torch.randn(2, P, device=dev, generator=g) * 0.1
grad = torch.randn(2, P, device=dev, generator=g) * 1e-3
opts, rows = {}, {}
for m in modes:
    cfg = OptimConfig(lr=1e-3, max_grad_norm=1e9) if m == "clipped" else OptimConfig(lr=1e-3)  # a bound that never binds
    opts[m] = FlatOptimizer(params.clone(), grad, cfg)
    if m == "torchclip":  # parameters whose .grad are the rows, as a torch-side user of the flat gradient has them
        rows[m] = [torch.nn.Parameter(opts[m].params[i]) for i in range(2)]
        for i, r in enumerate(rows[m]):
            r.grad = grad[i]


def step(m):
    if m == "torchclip":
        for r in rows[m]:
            torch.nn.utils.clip_grad_norm_([r], 1e9)
    opts[m].step()


def sync():
    if dev.type == "cuda":
        torch.cuda.synchronize()


res = {m: [] for m in modes}
for m in modes:
    for _ in range(3):
        step(m)
sync()
for w in range(windows):
    for m in modes:  # interleaved windows
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step(m)
        e1.record()
        e1.synchronize()
        res[m].append(e0.elapsed_time(e1) / steps)
for m in modes:
    xs = sorted(res[m])
    print(json.dumps({"tree": os.path.basename(os.getcwd()), "mode": m, "P": P, "rows": 2, "steps": steps,
                      "ms_per_step_windows": [round(x, 4) for x in res[m]], "ms_median": round(xs[len(xs) // 2], 4),
                      "GBps_28B": round(2 * P * 28 / xs[len(xs) // 2] / 1e6, 1)}), flush=True)

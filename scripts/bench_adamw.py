#!/usr/bin/env python3
"""What AdamW's decoupled weight decay costs inside the fused step: ``FusedTrainer.train`` timed
the way bench.py's timed region is (warm-up over up to 16 launches, synchronize, ``train(K)``,
synchronize) on one GPU, for

  adam        Adam, weight_decay 0 (bench.py's optimizer)
  adam_wd     coupled Adam, weight_decay 0.1 (g += wd * p)
  adamw       AdamW, weight_decay 0.1 (p *= 1 - lr * wd, a launch constant)
  adamw_cos   AdamW, weight_decay 0.1 under a cosine schedule (d_t read per step from the
              schedule's device table)

Usage: python scripts/bench_adamw.py [--batch 256] [--steps 2000 --warmup 200 --reps 5]
           [--weight_decay 0.1] [--groups auto|on|off] [--precision fp32|bf16]
           [--launch persistent|graph|eager]

Every variant gets its own engine on bench.py's workload; the timed calls are interleaved over
the variants, ``--reps`` rounds in one process, so clock drift hits them alike.  Prints one JSON
line: per variant the kernel instance, every round's us/step and their median.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from distributed_training_pytorch_amd import _native  # noqa: E402
from distributed_training_pytorch_amd.data.sampler import SamplerGeometry  # noqa: E402
from distributed_training_pytorch_amd.data.toy_data import ToyData  # noqa: E402
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer  # noqa: E402
from distributed_training_pytorch_amd.models.toy import ToyModel  # noqa: E402
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC  # noqa: E402
from distributed_training_pytorch_amd.ops.optim import OptimConfig  # noqa: E402
from distributed_training_pytorch_amd.ops.schedule import LrSchedule  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weight_decay", type=float, default=0.1)
    ap.add_argument("--steps-per-launch", type=int, default=1000)
    ap.add_argument("--launch", choices=["persistent", "graph", "eager"], default="persistent")
    ap.add_argument("--groups", choices=["auto", "on", "off"], default="auto")
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    a = ap.parse_args()
    _native.set_wait_mode(os.environ.get("DTP_WAIT_MODE", "spin"))  # as bench.py, before the first GPU touch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    ds = ToyData(n=512, seed=a.seed)
    X, Y = ds.device_tensors(dev)
    geom = SamplerGeometry(n=512, world=1, rank=0, batch=a.batch, seed=a.seed)
    torch.manual_seed(a.seed)
    init = [ToyModel().flat_params.detach().clone() for _ in range(2)]
    ecfg = EngineConfig(launch=a.launch, steps_per_launch=a.steps_per_launch, precision=a.precision, groups=a.groups)
    total = a.warmup + a.reps * a.steps
    cosine = LrSchedule.make("cosine", 1e-3, warmup_iters=a.warmup, decay_iters=total, min_ratio=0.1, total=total)
    variants = {"adam": OptimConfig(lr=1e-3),
                "adam_wd": OptimConfig(lr=1e-3, weight_decay=a.weight_decay),
                "adamw": OptimConfig("adamw", 1e-3, weight_decay=a.weight_decay),
                "adamw_cos": OptimConfig("adamw", 1e-3, weight_decay=a.weight_decay, schedule=cosine)}
    engines, info = {}, {}
    for name, ocfg in variants.items():
        tr = engines[name] = FusedTrainer(TOY_SPEC, 2, X, Y, geom, ocfg, ecfg, init_params=init)
        split = max(1, min(a.warmup, 16))
        done = 0
        for i in range(split):
            k = (a.warmup - done) // (split - i)
            tr.train(k)
            done += k
        torch.cuda.synchronize(dev)
        info[name] = {"optimizer": ocfg.label, "weight_decay": ocfg.weight_decay, "scheduled": ocfg.schedule is not None,
                      "lanes": tr.lanes, "waves": tr.kernel_waves, "groups": tr.groups, "us_per_step": []}
    gc.disable()
    for _ in range(a.reps):
        for name, tr in engines.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            tr.train(a.steps)
            torch.cuda.synchronize(dev)
            info[name]["us_per_step"].append(round(1e6 * (time.perf_counter() - t0) / a.steps, 4))
    gc.enable()
    for name, tr in engines.items():
        tr.check_comm()
        info[name]["median"] = statistics.median(info[name]["us_per_step"])
        info[name]["final_loss"] = tr.losses(tr.t - 1, tr.t)[0].tolist()
        tr.close()
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
                      "weight_decay": a.weight_decay, "precision": a.precision, "launch": a.launch, "variants": info}),
          flush=True)


if __name__ == "__main__":
    main()

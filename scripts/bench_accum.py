#!/usr/bin/env python3
"""What a micro-batch costs inside the fused step's accumulation twins (``csrc/accum_core.h``):
``FusedTrainer.train`` timed the way bench.py's timed region is (warm-up over up to 16 launches,
synchronize, ``train(K)``, synchronize), on one GPU, Adam + MSE in fp32.

Usage: python scripts/bench_accum.py [--batches 64,128,256] [--accumulate 2,4,8]
           [--steps 2000 --warmup 200 --reps 5] [--groups auto|on|off] [--launch persistent|graph|eager]

For every per-rank micro-batch size one plain engine (``accumulate = 1``: the plain instance,
whose device code is the parent commit's) and one engine per ``accumulate`` value, on bench.py's
workload; the timed calls are interleaved over the variants, ``--reps`` rounds in one process, so
clock drift hits them alike.  K counts optimizer steps.  Prints one JSON line per micro-batch
size: per variant the kernel instance, every round's us per optimizer step, their median, and the
median per micro-batch (median / accumulate).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,128,256")
    ap.add_argument("--accumulate", default="2,4,8")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps-per-launch", type=int, default=1000)
    ap.add_argument("--launch", choices=["persistent", "graph", "eager"], default="persistent")
    ap.add_argument("--groups", choices=["auto", "on", "off"], default="auto")
    a = ap.parse_args()
    _native.set_wait_mode(os.environ.get("DTP_WAIT_MODE", "spin"))  # as bench.py, before the first GPU touch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    ds = ToyData(n=512, seed=a.seed)
    X, Y = ds.device_tensors(dev)
    torch.manual_seed(a.seed)
    init = [ToyModel().flat_params.detach().clone() for _ in range(2)]
    for batch in [int(b) for b in a.batches.split(",")]:
        geom = SamplerGeometry(n=512, world=1, rank=0, batch=batch, seed=a.seed)
        engines, info = {}, {}
        for A in [1, *[int(x) for x in a.accumulate.split(",")]]:
            name = "plain" if A == 1 else f"A{A}"
            ecfg = EngineConfig(launch=a.launch, steps_per_launch=a.steps_per_launch, groups=a.groups, accumulate=A)
            tr = engines[name] = FusedTrainer(TOY_SPEC, 2, X, Y, geom, OptimConfig(lr=1e-3), ecfg, init_params=init)
            split = max(1, min(a.warmup, 16))
            done = 0
            for i in range(split):
                k = (a.warmup - done) // (split - i)
                tr.train(k)
                done += k
            torch.cuda.synchronize(dev)
            info[name] = {"accumulate": A, "lanes": tr.lanes, "waves": tr.kernel_waves, "groups": tr.groups,
                          "accum_in_kernel": tr.accum_in_kernel, "us_per_step": []}
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
            info[name]["us_per_micro_batch"] = round(info[name]["median"] / info[name]["accumulate"], 4)
            info[name]["final_loss"] = tr.losses(tr.t - 1, tr.t)[0].tolist()
            tr.close()
        print(json.dumps({"micro_batch": batch, "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
                          "launch": a.launch, "variants": info}), flush=True)


if __name__ == "__main__":
    main()

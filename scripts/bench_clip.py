#!/usr/bin/env python3
"""What gradient clipping inside the fused step costs: ``FusedTrainer.train`` timed the way
bench.py's timed region is (warm-up over up to 16 launches, synchronize, ``train(K)``,
synchronize), unclipped and with the clip twins (``csrc/clip_core.h``), on one GPU.

Usage: python scripts/bench_clip.py [--clip_grad_norm F] [--clip_grad_value F] [--batch 256]
           [--steps 2000 --warmup 200 --reps 5] [--groups auto|on|off] [--precision fp32|bf16]
           [--optimizer adam|sgd] [--loss mse|ce] [--launch persistent|graph|eager]

Every variant asked for (``plain`` always, ``norm`` with --clip_grad_norm, ``value`` with
--clip_grad_value) gets its own engine on bench.py's workload; the timed calls are interleaved
over the variants, ``--reps`` rounds in one process, so clock drift hits them alike.  Prints one
JSON line: per variant the kernel instance, every round's us/step and their median.
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
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC, MlpSpec  # noqa: E402
from distributed_training_pytorch_amd.ops.optim import OptimConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip_grad_norm", type=float, default=0.0)
    ap.add_argument("--clip_grad_value", type=float, default=0.0)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps-per-launch", type=int, default=1000)
    ap.add_argument("--launch", choices=["persistent", "graph", "eager"], default="persistent")
    ap.add_argument("--groups", choices=["auto", "on", "off"], default="auto")
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--optimizer", choices=["adam", "sgd"], default="adam")
    ap.add_argument("--loss", choices=["mse", "ce"], default="mse")
    a = ap.parse_args()
    _native.set_wait_mode(os.environ.get("DTP_WAIT_MODE", "spin"))  # as bench.py, before the first GPU touch
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    ds = ToyData(n=512, seed=a.seed, classes=4 if a.loss == "ce" else 0)
    spec = MlpSpec(2, 10, 5, 4) if a.loss == "ce" else TOY_SPEC
    X, Y = ds.device_tensors(dev)
    geom = SamplerGeometry(n=512, world=1, rank=0, batch=a.batch, seed=a.seed)
    torch.manual_seed(a.seed)
    if a.loss == "ce":
        init = [torch.cat([t.reshape(-1) for lay in [torch.nn.Linear(i, o) for i, o in spec.dims()]
                           for t in (lay.weight.detach(), lay.bias.detach())]) for _ in range(2)]
    else:
        init = [ToyModel().flat_params.detach().clone() for _ in range(2)]
    ecfg = EngineConfig(launch=a.launch, steps_per_launch=a.steps_per_launch, precision=a.precision, groups=a.groups,
                        loss=a.loss)
    clips = {"plain": {}}
    if a.clip_grad_norm > 0:
        clips["norm"] = {"max_grad_norm": a.clip_grad_norm}
    if a.clip_grad_value > 0:
        clips["value"] = {"clip_grad_value": a.clip_grad_value}
    engines, info = {}, {}
    for name, clip in clips.items():
        ocfg = OptimConfig(lr=1e-3, **clip) if a.optimizer == "adam" else OptimConfig("sgd", 1e-2, momentum=0.9, **clip)
        tr = engines[name] = FusedTrainer(spec, 2, X, Y, geom, ocfg, ecfg, init_params=init)
        split = max(1, min(a.warmup, 16))
        done = 0
        for i in range(split):
            k = (a.warmup - done) // (split - i)
            tr.train(k)
            done += k
        torch.cuda.synchronize(dev)
        info[name] = {"lanes": tr.lanes, "waves": tr.kernel_waves, "groups": tr.groups,
                      "clip_in_kernel": tr.clip_in_kernel, "us_per_step": []}
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
        if tr.grad_norm is not None:
            info[name]["grad_norm"] = tr.grad_norm.tolist()
        tr.close()
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "optimizer": a.optimizer,
                      "loss": a.loss, "precision": a.precision, "launch": a.launch, "variants": info}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The flat optimizer launch that writes the FP8 weight operands (csrc/optim_fp8.hip) against what it
replaces: the plain flat optimizer launch plus one given-scale quantiser launch per hidden weight, on a
two-model bank.  Device events around ``--iters`` calls, ``--rounds`` alternated rounds, medians and ranges.

usage: python scripts/bench_fp8_shadow.py [--width 4096] [--depth 3] [--iters 20] [--rounds 5]
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_training_pytorch_amd.models.bank import ModelBank  # noqa: E402
from distributed_training_pytorch_amd.ops.fp8 import quantize_fp8  # noqa: E402
from distributed_training_pytorch_amd.ops.optim import OptimConfig, flat_optimizer_step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    bank = ModelBank(2, hidden=a.width, depth=a.depth, compute_dtype=torch.float8_e4m3fn, fp8_recipe="delayed").to(dev)
    sh = bank.fp8_shadow()
    for st, k in sh.slots:
        st.set_scale(k, 64.0)
    cfg = OptimConfig(lr=1e-3)
    m, v = torch.zeros_like(bank.flat), torch.zeros_like(bank.flat)
    step = torch.zeros(2, dtype=torch.int32, device=dev)
    grad = 1e-3 * torch.randn(bank.flat.numel() + 2, device=dev)

    def plain():
        flat_optimizer_step(bank.flat, m, v, step, grad, cfg)

    def plain_and_quantise():
        plain()
        for w, slot in zip(sh.weights, sh.slots):
            quantize_fp8(w, "e4m3", transpose=True, scale=slot)

    def shadowed():
        flat_optimizer_step(bank.flat, m, v, step, grad, cfg, shadow=sh)

    cases = {"optimizer": plain, "optimizer+quantisers": plain_and_quantise, "optimizer_fp8": shadowed}
    times = {k: [] for k in cases}
    for fn in cases.values():
        fn()
    for _ in range(a.rounds):
        for name, fn in cases.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.iters)
    print(json.dumps({"width": a.width, "depth": a.depth, "weights": len(sh.weights), "work_items": sh._n_items,
                      "ms_per_call": {k: {"median": round(statistics.median(t), 4), "min": round(min(t), 4),
                                          "max": round(max(t), 4)} for k, t in times.items()}}), flush=True)


if __name__ == "__main__":
    main()

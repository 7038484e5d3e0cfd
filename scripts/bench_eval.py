#!/usr/bin/env python3
"""Held-out evaluation of 2 toy models: microseconds per evaluation, per way of doing it.

  kernel : ops.eval.evaluate -- forward, loss and fp64 reduction of both models in one launch
           (rows past the one-launch limit: a partial launch and a finalize), no host sync
  graph  : the same call captured into a hipGraph, 20 calls per replay
  manual : the only way without it: ToyModel.forward_many + the fused MSE pair (mse) or
           torch's cross_entropy and an argmax comparison per model (ce) under no_grad
  *_host : either way followed by the copy of its result to the host (what a logging caller pays)

Device events around --calls calls per window (a host clock around a synchronised window
for the *_host ways), --windows windows per way, the ways' windows interleaved; every way is
warmed up first.  One JSON line per (loss, rows, way) with the median and the spread of
the windows.  Needs a GPU.

usage: python scripts/bench_eval.py [--rows 512,4096,65536] [--windows N] [--calls N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from distributed_training_pytorch_amd.data.toy_data import synthetic_toy  # noqa: E402
from distributed_training_pytorch_amd.models.toy import ToyModel  # noqa: E402
from distributed_training_pytorch_amd.ops import eval as E  # noqa: E402
from distributed_training_pytorch_amd.ops.loss import MSELoss  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", default="512,4096,65536")
p.add_argument("--windows", type=int, default=7)
p.add_argument("--calls", type=int, default=400)
p.add_argument("--out", default=None)
a = p.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_eval.py measures on the GPU: none found")
dev = torch.device("cuda", 0)
REPLAY = 20
lines = []

for loss in ("mse", "ce"):
    out_f = 4 if loss == "ce" else 1
    torch.manual_seed(0)
    models = [ToyModel(out_features=out_f).to(dev) for _ in range(2)]
    spec = models[0].spec
    params = torch.stack([m.flat_params.detach() for m in models]).contiguous()
    for n in [int(r) for r in a.rows.split(",")]:
        X, Y = synthetic_toy(n, dev, seed=7)
        if loss == "ce":
            Y = (torch.arange(n, device=dev) % out_f).float().view(n, 1)
        cls = Y.view(-1).long()
        out = torch.zeros(2, 2, dtype=torch.float64, device=dev)
        ws = E.eval_ws(n, 2, dev)
        mse = MSELoss()

        def kernel():
            return E.evaluate(params, spec, X, Y, loss=loss, out=out, ws=ws)

        @torch.no_grad()
        def manual():
            ox, oy = ToyModel.forward_many(models, X)
            if loss == "mse":
                lx, ly, _ = mse.pair(ox, oy, Y)
                return torch.stack([lx, ly])
            return torch.stack([torch.nn.functional.cross_entropy(ox, cls), torch.nn.functional.cross_entropy(oy, cls),
                                (ox.argmax(1) == cls).float().mean(), (oy.argmax(1) == cls).float().mean()])

        for f in (kernel, manual):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(REPLAY):
                kernel()
        g.replay()
        torch.cuda.synchronize()
        # the two ways agree on what they measure
        got = (out[:, 0] / (n * (out_f if loss == "mse" else 1))).float()
        assert torch.allclose(got, manual()[:2].float(), rtol=1e-4, atol=1e-6), (got, manual())

        calls = max(REPLAY, a.calls if n <= 4096 else a.calls // 4)
        ways = {"kernel": (kernel, calls, False), "graph": (g.replay, calls // REPLAY, False),
                "manual": (manual, calls, False),
                "kernel_host": (lambda: kernel().cpu(), calls // 4, True),
                "manual_host": (lambda: manual().cpu(), calls // 4, True)}
        res = {w: [] for w in ways}
        for _ in range(a.windows):
            for w, (f, k, host) in ways.items():  # interleaved windows
                per = k * (REPLAY if w == "graph" else 1)
                if host:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(k):
                        f()
                    torch.cuda.synchronize()
                    res[w].append((time.perf_counter() - t0) * 1e6 / per)
                else:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(k):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    res[w].append(e0.elapsed_time(e1) * 1e3 / per)
        for w, v in res.items():
            lines.append({"bench": "eval", "loss": loss, "rows": n, "models": 2, "way": w,
                          "us_per_eval_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                          "us_max": round(max(v), 3), "windows": len(v),
                          "evals_per_window": ways[w][1] * (REPLAY if w == "graph" else 1),
                          "one_launch_rows": E.one_launch_rows(dev)})
            print(json.dumps(lines[-1]), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in lines)

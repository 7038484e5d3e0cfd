"""Shared inputs and yardsticks of the AdamW tests (``tests/test_adamw_cpu.py``,
``tests/test_adamw_gpu.py``).  CPU-only code.

**Yardstick.**  fp64 autograd + ``torch.optim.AdamW`` (under a schedule: + ``LambdaLR``, the
loop of ``tests/sched_cases.py``).

**Inputs.**  The set-up of ``tests/test_optim_hyper_gpu.py``: ``ToyData(n=512, seed=3)``, sampler
seed 11, init ``randn * 0.4`` (seed 100), 12 steps (the GPU tests run them in launches of 5).

* unscheduled: ``lr=1e-2, weight_decay=0.1``.  Its twins -- coupled Adam with the same
  ``weight_decay`` and Adam with ``weight_decay=0`` -- end more than 10 tolerances away on at least
  half of every model's parameters (``test_adamw_cpu.py``), so a kernel that coupled the decay or
  dropped it cannot pass.
* scheduled: the ramp ``lr_t = 1e-2 (t + 1) / 12`` with ``weight_decay=0.5``.  Its twin decays by the
  base rate ``1e-2`` at every step (what a kernel that took ``d`` as a launch constant would do).
"""
from __future__ import annotations

import dataclasses
import functools

import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream, SamplerGeometry
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC, MlpSpec, mlp_forward_ref, mlp_forward_ref_bf16
from distributed_training_pytorch_amd.ops.optim import OptimConfig
from distributed_training_pytorch_amd.ops.schedule import LrSchedule

from .ref_train import loss_fn, torch_train
from .sched_cases import torch_train_sched
from .test_optim_hyper_gpu import LOSS_TOL, PARAM_TOL, PARAM_TOL_LOOSE, _data, _init  # noqa: F401

STEPS = 12
CE_SPEC = MlpSpec(2, 10, 5, 4)
FLAT_TOL = dict(rtol=1e-5, atol=1e-6)
LR, WD, WD_RAMP = 1e-2, 0.1, 0.5


def ramp(n: int = STEPS) -> LrSchedule:
    """``lr_t = 1e-2 (t + 1) / 12`` for t < 12; ``n`` > 12 extends the same line (the 1100-step
    launches), so no two neighbouring entries coincide."""
    return LrSchedule.from_values([LR * (t + 1) / 12 for t in range(n)])


ADAMW = OptimConfig("adamw", LR, weight_decay=WD)
COUPLED = OptimConfig("adam", LR, weight_decay=WD)      # twin: the decay through the gradient
PLAIN = OptimConfig("adam", LR)                          # twin: no decay
ADAMW_RAMP = OptimConfig("adamw", LR, weight_decay=WD_RAMP, schedule=ramp())
CONFIGS = {"adamw": ADAMW, "coupled": COUPLED, "plain": PLAIN, "ramp": ADAMW_RAMP}


def with_wd0(cfg: OptimConfig) -> OptimConfig:
    return dataclasses.replace(cfg, weight_decay=0.0)


def _geoms(batch, world):
    return [EpochIndexStream(SamplerGeometry(n=512, world=world, rank=r, batch=batch, seed=11)) for r in range(world)]


@functools.lru_cache(maxsize=None)
def reference(loss: str, batch: int, which: str, world: int = 1, bf16: bool = False):
    """(params [2, P], losses [STEPS, 2]) of fp64 autograd + torch.optim for ``CONFIGS[which]``;
    shared, never modified."""
    spec = CE_SPEC if loss == "ce" else TOY_SPEC
    ds = _data(loss)
    fwd = mlp_forward_ref_bf16 if bf16 else mlp_forward_ref
    cfg = CONFIGS[which]
    if cfg.schedule is None:
        return torch_train(spec, _init(spec), ds.X, ds.Y, _geoms(batch, world), STEPS, cfg, loss, forward=fwd)
    return torch_train_sched(spec, _init(spec), ds.X, ds.Y, _geoms(batch, world), STEPS, cfg, loss, forward=fwd)


@functools.lru_cache(maxsize=None)
def reference_base_rate_decay(loss: str, batch: int):
    """The scheduled case's twin: Adam under the ramp, the decay ``p *= 1 - lr * weight_decay``
    with the base rate at every step.  fp64, written out (torch has no such optimizer)."""
    spec = CE_SPEC if loss == "ce" else TOY_SPEC
    ds = _data(loss)
    X, Y = ds.X.double(), ds.Y
    geoms = _geoms(batch, 1)
    sched = ramp()
    out = []
    for p0 in _init(spec):
        p = torch.nn.Parameter(p0.double().clone())
        opt = torch.optim.Adam([p], lr=1.0)
        for t in range(STEPS):
            idx = torch.tensor(geoms[0].indices(t), dtype=torch.long)
            q = p.detach().clone().requires_grad_(True)
            lo = loss_fn(mlp_forward_ref(q, spec, X[idx]), Y[idx].double() if loss == "mse" else Y[idx], loss)
            (p.grad,) = torch.autograd.grad(lo, q)
            with torch.no_grad():
                p.mul_(1 - LR * WD_RAMP)
            for g in opt.param_groups:
                g["lr"] = sched.lr(t)
            opt.step()
        out.append(p.detach().float())
    return torch.stack(out)


CLIP_NORM = 0.05  # binds at every one of the 12 steps of both references (tests/test_adamw_cpu.py)


@functools.lru_cache(maxsize=None)
def reference_twin(kind: str, which: str, batch: int = 64):
    """fp64 autograd + torch.optim.AdamW for the fused step's twins, MSE: ``kind`` "clip" clips
    each model's gradient to ``CLIP_NORM`` with torch's clip_grad_norm_ ahead of the step; "accum2"
    steps on the mean of the gradients of the two consecutive batches 2t, 2t + 1 and logs the mean of
    their losses.  The group's lr is set to ``cfg.lr_at(t)`` before step t.  Returns (params [2, P],
    losses [STEPS, 2], norms [STEPS, 2] of the gradient before clipping)."""
    cfg = CONFIGS[which]
    ds = _data("mse")
    X, Y = ds.X.double(), ds.Y.double()
    stream = _geoms(batch, 1)[0]
    acc = 2 if kind == "accum2" else 1
    out, losses, norms = [], [], []
    for p0 in _init(TOY_SPEC):
        p = torch.nn.Parameter(p0.double().clone())
        opt = dataclasses.replace(cfg, schedule=None).torch_optimizer([p])
        assert type(opt) is torch.optim.AdamW
        ls, ns = [], []
        for t in range(STEPS):
            gs, lo_ = [], []
            for j in range(acc):
                idx = torch.tensor(stream.indices(t * acc + j), dtype=torch.long)
                q = p.detach().clone().requires_grad_(True)
                lo = loss_fn(mlp_forward_ref(q, TOY_SPEC, X[idx]), Y[idx], "mse")
                gs.append(torch.autograd.grad(lo, q)[0])
                lo_.append(lo.item())
            p.grad = torch.stack(gs).mean(0)
            ns.append(p.grad.norm().item())
            if kind == "clip":
                torch.nn.utils.clip_grad_norm_([p], CLIP_NORM)
            for g in opt.param_groups:
                g["lr"] = cfg.lr_at(t)
            opt.step()
            ls.append(sum(lo_) / acc)
        out.append(p.detach().float())
        losses.append(ls)
        norms.append(ns)
    return torch.stack(out), torch.tensor(losses, dtype=torch.float32).t().contiguous(), torch.tensor(norms).t()


def share(p_case, p_twin, rtol, atol):
    """Per model: the share of parameters that differ by more than 10 tolerances."""
    far = (p_case - p_twin).abs() > 10 * (atol + rtol * p_twin.abs())
    return far.double().mean(dim=-1)


def decay_products(p0: torch.Tensor, cfg: OptimConfig, n: int) -> torch.Tensor:
    """``p0 * d_0 * ... * d_{n-1}`` formed step by step in ``p0``'s dtype (fp32), each ``d_t`` =
    ``(float)(1 - lr_t * weight_decay)`` with the product and difference in Python floats (f64)."""
    p = p0.clone()
    for t in range(n):
        d = torch.tensor(1.0 - cfg.lr_at(t) * cfg.weight_decay, dtype=torch.float64).to(p.dtype)
        p = p * d
    return p


def zero_gradient_problem(spec=TOY_SPEC, seed=100, n=2):
    """Targets 0.5 everywhere and an init whose last layer is W = 0, b = 0.5 (everything else
    random): every output is exactly 0.5, the loss and every gradient exactly 0 in fp32 and
    bf16, so one AdamW step is the decay alone.  Returns (X, Y, init list)."""
    ds = _data("mse")
    Y = torch.full_like(ds.Y, 0.5)
    init = _init(spec, seed, n)
    out = spec.out_features
    last = out * (spec.hidden + 1)  # torch order: the last Linear's weight [out, h], then its bias [out]
    for p in init:
        p[-last:-out] = 0.0
        p[-out:] = 0.5
    return ds.X, Y, init

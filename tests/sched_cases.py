"""Shared inputs and the yardstick of the learning-rate schedule tests
(``tests/test_lr_schedule_cpu.py``, ``tests/test_lr_schedule_gpu.py``).  CPU-only code.

**Yardstick.**  fp64 autograd + ``torch.optim`` + ``torch.optim.lr_scheduler.LambdaLR``: the
loop of ``tests/ref_train.py`` with a scheduler stepped after every optimizer step.  The
optimizer's base rate is 1.0 and the lambda returns the table's value, so the param group's
``lr`` of step t is ``values[min(t, len - 1)]`` itself, not a product that rounds.

**Inputs.**  ``ToyData(n=512, seed=21)``, ``SamplerGeometry(n=512, batch=B, seed=3)``, init
``randn(P, seed=B) * 0.4`` for two models, Adam ``lr=1e-2`` / SGD ``lr=5e-2, momentum=0.9``,
schedules ``W=3, N=10, r=0.1`` (``step``: ``S=4, gamma=0.5``), 12 steps.
"""
from __future__ import annotations

import dataclasses
import functools

import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream, SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC, mlp_forward_ref, mlp_forward_ref_bf16
from distributed_training_pytorch_amd.ops.optim import OptimConfig
from distributed_training_pytorch_amd.ops.schedule import LrSchedule

from .ref_train import loss_fn

STEPS = 12
W, N, R, S, GAMMA = 3, 10, 0.1, 4, 0.5
KINDS = ("constant", "linear", "cosine", "step")
ADAM = OptimConfig(lr=1e-2)
SGD = OptimConfig("sgd", 5e-2, momentum=0.9)
DATA_SEED, SAMPLER_SEED = 21, 3

# copied from tests/test_optim_hyper_gpu.py (LOSS_TOL, PARAM_TOL, PARAM_TOL_LOOSE) and its flat
# optimizer comparison (rtol 1e-5 / atol 1e-6): a schedule changes one scalar per step and adds
# one float conversion, so it earns no looser bound
LOSS_TOL = dict(rtol=1e-4, atol=1e-5)
PARAM_TOL = dict(rtol=1e-4, atol=2e-5)        # the lanes / split-batch / layer-split steps
PARAM_TOL_LOOSE = dict(rtol=1e-3, atol=3e-5)  # the one-lane step
FLAT_TOL = dict(rtol=1e-5, atol=1e-6)
# the bf16 cell: copied from tests/test_bf16_gpu.py, the fused bf16 steps against autograd through
# the bf16 rounding model (accumulation order may move a bf16 value by an ulp, 2^-8)
BF16_LOSS_TOL = dict(rtol=2e-2, atol=1e-3)
BF16_PARAM_TOL = dict(rtol=2e-2, atol=2e-3)


def base(opt: str) -> OptimConfig:
    return ADAM if opt == "adam" else SGD


def schedule(kind: str, lr: float) -> LrSchedule:
    return LrSchedule.make(kind, lr, warmup_iters=W, decay_iters=N, min_ratio=R, step_size=S, gamma=GAMMA,
                           total=STEPS)


def config(opt: str, kind: str | None) -> OptimConfig:
    """The optimizer of a cell: ``kind`` None = no schedule."""
    b = base(opt)
    return b if kind is None else dataclasses.replace(b, schedule=schedule(kind, b.lr))


def zigzag(lr: float, n: int) -> LrSchedule:
    """``lr (1 + 0.1 ((3 t mod 7) - 3))``: neighbouring entries never coincide."""
    return LrSchedule.from_values([lr * (1 + 0.1 * ((3 * t) % 7 - 3)) for t in range(n)])


def data():
    return ToyData(n=512, seed=DATA_SEED)


def geom(batch: int, world: int = 1, rank: int = 0) -> SamplerGeometry:
    return SamplerGeometry(n=512, world=world, rank=rank, batch=batch, seed=SAMPLER_SEED)


def init(batch: int, spec=TOY_SPEC, n: int = 2):
    g = torch.Generator().manual_seed(batch)
    return [torch.randn(spec.P, generator=g) * 0.4 for _ in range(n)]


def torch_optimizer(ocfg: OptimConfig, params):
    """``(optimizer, scheduler or None)`` of plain torch for ``ocfg``."""
    if ocfg.schedule is None:
        return ocfg.torch_optimizer(params), None
    opt = dataclasses.replace(ocfg, lr=1.0, schedule=None).torch_optimizer(params)
    return opt, torch.optim.lr_scheduler.LambdaLR(opt, ocfg.schedule.lr)


def torch_train_sched(spec, init_params, X, Y, geoms, steps: int, ocfg: OptimConfig, loss: str = "mse",
                      forward=mlp_forward_ref):
    """``ref_train.torch_train`` with the schedule: (params [n_models, P], losses [steps, n_models])."""
    X, Y = X.detach().cpu().double(), Y.detach().cpu()
    params = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in init_params]
    pairs = [torch_optimizer(ocfg, [p]) for p in params]
    losses = []
    for t in range(steps):
        row = []
        for p, (opt, sched) in zip(params, pairs):
            gs, ls = [], []
            for g in geoms:
                idx = torch.tensor(g.indices(t), dtype=torch.long)
                q = p.detach().clone().requires_grad_(True)
                lo = loss_fn(forward(q, spec, X[idx]), Y[idx].double() if loss == "mse" else Y[idx], loss)
                (gr,) = torch.autograd.grad(lo, q)
                gs.append(gr)
                ls.append(lo.item())
            p.grad = torch.stack(gs).mean(0)
            opt.step()
            if sched is not None:
                sched.step()
            row.append(sum(ls) / len(geoms))
        losses.append(row)
    return torch.stack([p.detach().float() for p in params]), torch.tensor(losses, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def reference(batch: int, opt: str, kind: str | None, world: int = 1, bf16: bool = False):
    """The yardstick's (params [2, P], losses [STEPS, 2]) of a cell; shared, never modified.
    ``bf16``: autograd through the bf16 rounding model (``mlp_forward_ref_bf16``), in fp64."""
    ds = data()
    geoms = [EpochIndexStream(geom(batch, world, r)) for r in range(world)]
    return torch_train_sched(TOY_SPEC, init(batch), ds.X, ds.Y, geoms, STEPS, config(opt, kind),
                             forward=mlp_forward_ref_bf16 if bf16 else mlp_forward_ref)


def share(p_case, p_default, rtol, atol):
    """Per model: the share of parameters the schedule moved by more than 10 tolerances."""
    far = (p_case - p_default).abs() > 10 * (atol + rtol * p_default.abs())
    return far.double().mean(dim=-1)


# the fused-step instance families: id -> (batch, EngineConfig keywords, optimizers it has an
# instance for, (lanes, groups) the dispatcher must pick, parameter tolerance)
FAMILIES = {
    "fast":    (256, dict(groups="off"), ("adam",), (1, 1), PARAM_TOL_LOOSE),
    "generic": (256, dict(groups="off", cache_data=False), ("adam", "sgd"), (1, 1), PARAM_TOL_LOOSE),
    "lanes2":  (128, dict(groups="off"), ("adam", "sgd"), (2, 1), PARAM_TOL),
    "lanes4":  (64, dict(), ("adam", "sgd"), (4, 1), PARAM_TOL),
    "grp4":    (256, dict(groups="on"), ("adam", "sgd"), (4, 4), PARAM_TOL),  # the constant-count instance
    "grp3":    (130, dict(groups="on"), ("adam", "sgd"), (4, 3), PARAM_TOL),
}
FAMILY_CELLS = [(f, o) for f, v in FAMILIES.items() for o in v[2]]


# ------------------------------------------------------------------------------ the Trainer
# configure_optimizers forms: two Adams over LitToyModel's two models with
#   "tuple-epoch": ([Adam, Adam], [StepLR, StepLR])  -- bare schedulers step at every epoch's end
#   "dict-step":   a tuple of {"optimizer", "lr_scheduler": {"scheduler", "interval": "step"}}
TRAINER_LR = 1e-2
TRAINER_EPOCHS, TRAINER_BATCH = 3, 128  # ToyData's 512 samples: 4 batches per epoch, 12 steps


def trainer_scheduler(form: str, opt):
    if form == "tuple-epoch":
        return torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    return torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.7)


def lit_model(form: str, root: str):
    """demo_pytorch_lightning.LitToyModel with a scheduled configure_optimizers."""
    import sys

    if root not in sys.path:
        sys.path.insert(0, root)
    from demo_pytorch_lightning import LitToyModel

    class LitSched(LitToyModel):
        def configure_optimizers(self):
            opts = [torch.optim.Adam(m.parameters(), lr=TRAINER_LR) for m in (self.model_X, self.model_Y)]
            scheds = [trainer_scheduler(form, o) for o in opts]
            self.scheds = scheds
            if form == "tuple-epoch":
                return opts, scheds
            return tuple({"optimizer": o, "lr_scheduler": {"scheduler": s, "interval": "step", "frequency": 1}}
                         for o, s in zip(opts, scheds))

    return LitSched()


def trainer_torch_loop(init_layers, dl, form: str, epochs: int = TRAINER_EPOCHS, scheduled: bool = True):
    """A plain torch loop on fp64 twins that steps the schedulers where Lightning 1.5 does: a
    step-interval one after its optimizer's step, an epoch-interval one at the epoch's end.
    Returns (flat parameters per model, get_last_lr() per model)."""
    import copy

    out, last = [], []
    for layers in init_layers:
        twin = copy.deepcopy(layers).double()
        opt = torch.optim.Adam(twin.parameters(), lr=TRAINER_LR)
        sched = trainer_scheduler(form, opt) if scheduled else None
        for _ in range(epochs):
            for x, y in dl:
                opt.zero_grad()
                torch.nn.functional.mse_loss(twin(x.double()), y.double()).backward()
                opt.step()
                if sched is not None and form == "dict-step":
                    sched.step()
            if sched is not None and form == "tuple-epoch":
                sched.step()
        out.append(torch.nn.utils.parameters_to_vector(twin.parameters()).detach())
        last.append(sched.get_last_lr() if sched is not None else [TRAINER_LR])
    return out, last

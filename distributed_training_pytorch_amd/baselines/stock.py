"""Stock PyTorch-ROCm eager re-enactment of the reference's hot loop.

This is the comparison baseline of BASELINE.md ("reference semantics on stock
PyTorch-ROCm eager DDP (RCCL)"): plain nn.Sequential ToyModels (no fused
kernels), torch DDP, torch.optim.Adam, DistributedSampler + DataLoader(bs=256,
pin_memory=True), per-iteration ``.cpu()`` of both losses and a gloo
all-reduce of them -- the loop body of ``demo.py:95-129`` without wandb/tqdm.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn as nn
from torch.nn.parallel import DistributedDataParallel as DDP
from torch.utils.data import DataLoader, DistributedSampler


def plain_toy_model(slope: float = 0.01) -> nn.Module:
    return nn.Sequential(nn.Linear(2, 10), nn.LeakyReLU(slope), nn.Linear(10, 10), nn.LeakyReLU(slope),
                         nn.Linear(10, 10), nn.LeakyReLU(slope), nn.Linear(10, 10), nn.LeakyReLU(slope),
                         nn.Linear(10, 1))


class StockLoop:
    def __init__(self, dataset, device, batch: int = 256, seed: int = 0, ddp: bool = True,
                 clip_grad_norm: float = 0.0, clip_grad_value: float = 0.0, schedule=None, accumulate: int = 1,
                 optim=None):
        """``optim``: an ``ops.optim.OptimConfig`` whose ``torch_optimizer`` both models then use
        (``--optimizer adamw``); None: the reference's verbatim ``Adam(lr=1e-3)`` pair.
        ``schedule``: an ``ops.schedule.LrSchedule``; both Adams then follow its values
        through ``torch.optim.lr_scheduler.LambdaLR`` (stepped after every optimizer step).
        ``accumulate``: batches per optimizer step, the torch idiom (``loss / A``, ``no_sync`` on
        DDP for the first ``A - 1`` backwards, the step on the last)."""
        self.accumulate = int(accumulate)
        if self.accumulate < 1:
            raise ValueError("accumulate must be >= 1")
        torch.manual_seed(seed)
        # gradient clipping per model (= per optimizer), torch's own functions; 0 = off
        self.clip_grad_norm = clip_grad_norm
        self.clip_grad_value = clip_grad_value
        self.device = device
        self.mx = plain_toy_model().to(device)
        self.my = plain_toy_model().to(device)
        self.ddp = ddp and dist.is_initialized()
        if self.ddp:
            ids = [device.index] if device.type == "cuda" else None
            self.mx = DDP(self.mx, device_ids=ids)
            self.my = DDP(self.my, device_ids=ids)
        if optim is None:
            self.ox = torch.optim.Adam(self.mx.parameters(), lr=1e-3)
            self.oy = torch.optim.Adam(self.my.parameters(), lr=1e-3)
        else:
            self.ox = optim.torch_optimizer(self.mx.parameters())
            self.oy = optim.torch_optimizer(self.my.parameters())
        self.schedulers = []
        if schedule is not None:
            # base lr 1.0 x the table's value: the param group's lr is the value itself
            for o in (self.ox, self.oy):
                for g in o.param_groups:
                    g["lr"] = 1.0
                self.schedulers.append(torch.optim.lr_scheduler.LambdaLR(o, schedule.lr))
        self.sampler = DistributedSampler(dataset, shuffle=True) if dist.is_initialized() else None
        self.loader = DataLoader(dataset, batch_size=batch, sampler=self.sampler, shuffle=False,
                                 pin_memory=device.type == "cuda")
        self.gloo = dist.new_group(backend="gloo") if dist.is_initialized() else None
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.loss = nn.MSELoss()
        self.epoch = 0
        self.it = None
        self.samples = 0
        self.last = (0.0, 0.0)

    def _next(self):
        while True:
            if self.it is None:
                if self.sampler is not None:
                    self.sampler.set_epoch(self.epoch)
                self.it = iter(self.loader)
            try:
                return next(self.it)
            except StopIteration:
                self.it = None
                self.epoch += 1

    def step(self):
        if self.accumulate > 1:
            return self._step_accumulating()
        data, target = self._next()
        self.ox.zero_grad(set_to_none=True)
        self.oy.zero_grad(set_to_none=True)
        data = data.to(self.device)
        target = target.to(self.device)
        out_x = self.mx(data)
        out_y = self.my(data)
        lx = self.loss(out_x, target)
        lx.backward()
        ly = self.loss(out_y, target)
        ly.backward()
        for m in (self.mx, self.my):
            if self.clip_grad_norm > 0:
                torch.nn.utils.clip_grad_norm_(m.parameters(), self.clip_grad_norm)
            elif self.clip_grad_value > 0:
                torch.nn.utils.clip_grad_value_(m.parameters(), self.clip_grad_value)
        self.ox.step()
        self.oy.step()
        for s in self.schedulers:
            s.step()
        b = target.size(0)
        rx = lx.detach().cpu() * b
        ry = ly.detach().cpu() * b
        if self.gloo is not None:
            dist.all_reduce(rx, group=self.gloo)
            dist.all_reduce(ry, group=self.gloo)
        self.last = (float(rx) / (b * self.world), float(ry) / (b * self.world))
        self.samples += b

    def _step_accumulating(self):
        import contextlib

        A = self.accumulate
        self.ox.zero_grad(set_to_none=True)
        self.oy.zero_grad(set_to_none=True)
        sx = sy = 0.0
        for j in range(A):
            data, target = self._next()
            data = data.to(self.device)
            target = target.to(self.device)
            hold = j < A - 1 and self.ddp  # no all-reduce before the window's last backward
            with (self.mx.no_sync() if hold else contextlib.nullcontext()), \
                    (self.my.no_sync() if hold else contextlib.nullcontext()):
                lx = self.loss(self.mx(data), target)
                (lx / A).backward()
                ly = self.loss(self.my(data), target)
                (ly / A).backward()
            sx += float(lx.detach().cpu())
            sy += float(ly.detach().cpu())
            self.samples += target.size(0)
        for m in (self.mx, self.my):
            if self.clip_grad_norm > 0:
                torch.nn.utils.clip_grad_norm_(m.parameters(), self.clip_grad_norm)
            elif self.clip_grad_value > 0:
                torch.nn.utils.clip_grad_value_(m.parameters(), self.clip_grad_value)
        self.ox.step()
        self.oy.step()
        for s in self.schedulers:
            s.step()
        # the step's loss: the mean of the window's mean losses, averaged over the ranks
        r = torch.tensor([sx / A, sy / A], dtype=torch.float64)
        if self.gloo is not None:
            dist.all_reduce(r, group=self.gloo)
        self.last = (float(r[0]) / self.world, float(r[1]) / self.world)

    def forward_eval(self, x):
        """Both models' outputs on x (the bare modules: no DDP bookkeeping for a forward
        that is never followed by a backward)."""
        return [getattr(m, "module", m)(x) for m in (self.mx, self.my)]

    def train(self, n: int):
        for _ in range(n):
            self.step()

    def close(self):
        if self.gloo is not None:
            dist.destroy_process_group(self.gloo)
            self.gloo = None

"""Learning-rate schedules: one definition of "the rate of step t" for every engine.

``t`` is the number of steps the optimizer has already taken -- the device step counter
before the step, 0-based.  ``lr(t) = values[min(t, len - 1)]``: past the table's end the
last value holds for ever.  The values are float64, as torch holds a param group's ``lr``.

The flat optimizer, the stage backward fused with it and the layer-split stages read the
same table from device memory (``DtpHyper::lr_tab``, indexed by the step counter they
already hold), so the rate changes across graph replays with no recapture.  The fused step
kernels read the per-step rows ``ops.optim.adam_bias_table`` forms from it on the host
(``{lr_t / (1 - b1^t), sqrt(1 - b2^t)}``, SGD ``{lr_t, 1}``), so the rate changes inside a
persistent launch with no host work per step; SGD indexes them by the device counter too,
Adam by the host's step number only (a scheduled fused Adam step cannot be captured in a
graph: ``FusedTrainer`` runs those steps as one-step launches).  The CPU branches index
``values`` by the same rule.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

KINDS = ("constant", "linear", "cosine", "step")


@dataclass(frozen=True)
class LrSchedule:
    values: tuple  # float64 rates, one per step; the last one holds for every later step
    _tables: dict = field(default_factory=dict, compare=False, hash=False, repr=False)

    def __post_init__(self):
        vals = tuple(float(v) for v in self.values)
        if not vals:
            raise ValueError("LrSchedule: at least one value")
        if not all(math.isfinite(v) for v in vals):
            raise ValueError("LrSchedule: the values must be finite")
        object.__setattr__(self, "values", vals)

    @classmethod
    def from_values(cls, seq) -> "LrSchedule":
        return cls(tuple(float(v) for v in seq))

    @classmethod
    def make(cls, kind: str, lr: float, warmup_iters: int = 0, decay_iters: int | None = None,
             min_ratio: float = 0.0, step_size: int | None = None, gamma: float = 0.1,
             total: int | None = None) -> "LrSchedule":
        """``t < W``: ``lr (t+1)/W``; then with ``q = min(1, (t-W)/(N-W))``:
        constant ``lr``; linear ``lr (1-(1-r)q)``; cosine ``lr (r+(1-r)(1+cos pi q)/2)``;
        step ``lr gamma^floor((t-W)/S)``.  Plain Python float arithmetic."""
        lr = float(lr)
        W = int(warmup_iters)
        r = float(min_ratio)
        if kind not in KINDS:
            raise ValueError(f"LrSchedule: unknown kind {kind!r} (one of {', '.join(KINDS)})")
        if not lr > 0:
            raise ValueError("LrSchedule: lr must be > 0")
        if W < 0:
            raise ValueError("LrSchedule: warmup_iters must be >= 0")
        if not 0.0 <= r <= 1.0:
            raise ValueError("LrSchedule: min_ratio must be in [0, 1]")

        def warm(t):
            return lr * (t + 1) / W

        if kind == "constant":
            return cls(tuple([warm(t) for t in range(W)] + [lr]))
        if kind in ("linear", "cosine"):
            if decay_iters is None:
                raise ValueError(f"LrSchedule: {kind} needs decay_iters")
            N = int(decay_iters)
            if N <= W:
                raise ValueError("LrSchedule: decay_iters must be > warmup_iters")
            vals = []
            for t in range(N + 1):
                if t < W:
                    vals.append(warm(t))
                    continue
                q = min(1.0, (t - W) / (N - W))
                if kind == "linear":
                    vals.append(lr * (1.0 - (1.0 - r) * q))
                else:
                    vals.append(lr * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * q))))
            vals[N] = r * lr
            return cls(tuple(vals))
        # step
        if step_size is None or int(step_size) <= 0:
            raise ValueError("LrSchedule: step needs step_size > 0")
        if total is None or int(total) <= 0:
            raise ValueError("LrSchedule: step needs total > 0 (the iterations the table covers)")
        S = int(step_size)
        g = float(gamma)
        return cls(tuple(warm(t) if t < W else lr * g ** ((t - W) // S) for t in range(max(int(total), W + 1))))

    def __len__(self) -> int:
        return len(self.values)

    def lr(self, t: int) -> float:
        """The rate of the step taken after ``t`` steps."""
        return self.values[min(int(t), len(self.values) - 1)]

    def device_table(self, device) -> torch.Tensor:
        """The values as a float64 tensor on ``device``, made once per device.  Whoever
        launches kernels with it keeps a reference for as long as launches or captured
        graphs can run (the schedule itself holds one too)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        tab = self._tables.get(device)
        if tab is None:
            tab = torch.tensor(self.values, dtype=torch.float64, device=device)
            self._tables[device] = tab
        return tab


def lr_at(cfg, t: int) -> float:
    """The rate an ``OptimConfig`` gives the step taken after ``t`` steps."""
    return cfg.lr if cfg.schedule is None else cfg.schedule.lr(t)

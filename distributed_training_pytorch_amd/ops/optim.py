"""Flat-buffer optimizers (Adam / SGD) over [n_models, P] parameters.

The math is the element-for-element mirror of torch.optim.Adam / SGD
(``csrc/optim_core.h``); the PyTorch reference below is used on CPU and by the
numerics tests.  The reference trains with Adam(lr=1e-3) (``demo.py:80-81``).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from .. import _native as nat
from .schedule import LrSchedule, lr_at


@dataclass
class OptimConfig:
    name: str = "adam"  # "adam" | "sgd"; "adamw" is stored as "adam" with decoupled_weight_decay
    lr: float = 1e-3
    betas: tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.0
    momentum: float = 0.0
    # gradient clipping, per row (one model = one optimizer); 0 = off, at most one of them:
    max_grad_norm: float = 0.0    # > 0: torch.nn.utils.clip_grad_norm_(row, max_grad_norm)
    clip_grad_value: float = 0.0  # > 0: torch.nn.utils.clip_grad_value_(row, clip_grad_value)
    # the rate of every step (ops.schedule); None: ``lr`` at every step
    schedule: LrSchedule | None = None
    # torch.optim.AdamW = Adam(decoupled_weight_decay=True): p *= 1 - lr_t * weight_decay ahead
    # of Adam's update, and weight_decay enters neither the gradient nor m / v.  Adam only.
    decoupled_weight_decay: bool = False

    def __post_init__(self):
        if self.name == "adamw":
            self.name = "adam"
            self.decoupled_weight_decay = True
        self.decoupled_weight_decay = bool(self.decoupled_weight_decay)
        if self.decoupled_weight_decay and self.name != "adam":
            raise ValueError(f"OptimConfig: decoupled weight decay is AdamW's; {self.name!r} has no decoupled form")
        if self.max_grad_norm > 0 and self.clip_grad_value > 0:
            raise ValueError("OptimConfig: max_grad_norm and clip_grad_value are exclusive (one clipping algorithm)")

    @property
    def clips(self) -> bool:
        return self.max_grad_norm > 0 or self.clip_grad_value > 0

    @property
    def label(self) -> str:
        """The optimizer's name for logs and run summaries: "adamw" | "adam" | "sgd"."""
        return "adamw" if self.name == "adam" and self.decoupled_weight_decay else self.name

    @property
    def kind(self) -> int:
        if self.name == "adam":
            return nat.MODE_ADAM
        if self.name == "sgd":
            return nat.MODE_SGD
        raise ValueError(f"unknown optimizer {self.name!r}")

    def hyper(self, slope: float = 0.01, grad_scale: float = 1.0, device=None) -> nat.Hyper:
        """The kernels' hyperparameters.  With a schedule, ``device`` is where the launch
        runs: the table lives there (cached by the schedule, which this config keeps alive)."""
        hp = nat.Hyper(self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.momentum,
                       slope, grad_scale)
        hp.decoupled_wd = 1 if self.decoupled_weight_decay else 0
        if self.schedule is not None:
            if device is None:
                raise ValueError("OptimConfig.hyper: a schedule needs the device of the launch")
            tab = self.schedule.device_table(device)
            hp.lr_tab = tab.data_ptr()
            hp.lr_tab_len = tab.numel()
        return hp

    def lr_at(self, t: int) -> float:
        """The rate of the step taken after ``t`` steps."""
        return lr_at(self, t)

    def torch_optimizer(self, params):
        if self.name == "adam" and self.decoupled_weight_decay:
            return torch.optim.AdamW(params, lr=self.lr, betas=self.betas, eps=self.eps,
                                     weight_decay=self.weight_decay)
        if self.name == "adam":
            return torch.optim.Adam(params, lr=self.lr, betas=self.betas, eps=self.eps,
                                    weight_decay=self.weight_decay)
        return torch.optim.SGD(params, lr=self.lr, momentum=self.momentum, weight_decay=self.weight_decay)


def adam_update_ref(p: torch.Tensor, m: torch.Tensor, v: torch.Tensor, g: torch.Tensor, t1: int,
                    cfg: OptimConfig) -> None:
    """In-place Adam step number t1 (1-based) with torch's operation order (fp32); the rate
    is that of the step taken after t1 - 1 steps."""
    b1, b2 = cfg.betas
    if cfg.weight_decay:
        if cfg.decoupled_weight_decay:  # AdamW: the factor in float64, one multiply in p's dtype
            p.mul_(1 - cfg.lr_at(t1 - 1) * cfg.weight_decay)
        else:
            g = g + cfg.weight_decay * p
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** t1
    bc2 = 1 - b2 ** t1
    denom = (v.sqrt() / math.sqrt(bc2)).add_(cfg.eps)
    p.addcdiv_(m, denom, value=-(cfg.lr_at(t1 - 1) / bc1))


def adam_bias_table(cfg: "OptimConfig", max_len: int = 1 << 22):
    """Adam's per-step scalars as the fused kernels use them: row t = {lr / (1 - b1^t),
    sqrt(1 - b2^t)} in float32, formed in float64 exactly as the kernels' own fill does
    (``pow_int``: repeated squaring, ``csrc/dtp_common.h``), so a launch reading this
    table is bitwise the launch that forms the scalars itself.  The table ends at the
    first t where both corrections are exactly 1.0 in float64; every later step uses
    that last row.  With a schedule the rows run to the later of that and the schedule's
    end (row t is the step taken after t - 1 steps).  None if that takes more than
    ``max_len`` steps (beta ~ 1, or a longer schedule): the kernel's own fill takes over."""
    import numpy as np

    if cfg.name == "sgd":
        # SGD under a schedule takes its per-step rate from the same table: rows {lr_t, 1}
        # (row t = the step taken after t - 1 steps); no schedule: no table, hp.lr
        if cfg.schedule is None or len(cfg.schedule) + 1 > max_len:
            return None
        vals = np.asarray(cfg.schedule.values, dtype=np.float64)
        t = np.arange(len(vals) + 1, dtype=np.int64)
        return np.stack([vals[np.clip(t - 1, 0, len(vals) - 1)].astype(np.float32),
                         np.ones(len(t), dtype=np.float32)], axis=1)
    b1, b2 = float(cfg.betas[0]), float(cfg.betas[1])

    def pow_int(b: float, t: "np.ndarray") -> "np.ndarray":
        r = np.ones(t.shape, dtype=np.float64)
        base = np.full(t.shape, b, dtype=np.float64)
        e = t.copy()
        while e.any():
            r = np.where(e & 1, r * base, r)
            base = base * base
            e >>= 1
        return r

    # beta ~ 1: the corrections are not yet 1.0 at the last step the search would reach
    # (they only grow with t), so there is no table -- without forming max_len rows to see it
    n = 1024
    while n < max_len:
        n *= 2
    last = np.array([n - 1], dtype=np.int64)
    if not ((1.0 - pow_int(b1, last) == 1.0) & (1.0 - pow_int(b2, last) == 1.0)).all():
        return None
    n = 1024
    while True:
        t = np.arange(n, dtype=np.int64)
        bc1 = 1.0 - pow_int(b1, t)
        bc2 = 1.0 - pow_int(b2, t)
        done = np.nonzero((bc1 == 1.0) & (bc2 == 1.0))[0]
        if done.size or n >= max_len:
            break
        n *= 2
    if not done.size:
        return None
    T = int(done[0])
    if cfg.schedule is None:
        with np.errstate(divide="ignore"):
            tab = np.stack([(float(cfg.lr) / bc1[:T + 1]).astype(np.float32),
                            np.sqrt(bc2[:T + 1]).astype(np.float32)], axis=1)
        return tab
    # row t1 = step number t1 = the step taken after t1 - 1 steps: rate values[min(t1 - 1, len - 1)]
    vals = np.asarray(cfg.schedule.values, dtype=np.float64)
    T = max(T, len(vals))
    if T + 1 > max_len:
        return None
    t = np.arange(T + 1, dtype=np.int64)
    bc1 = 1.0 - pow_int(b1, t)
    bc2 = 1.0 - pow_int(b2, t)
    lr_t = vals[np.clip(t - 1, 0, len(vals) - 1)]
    with np.errstate(divide="ignore"):
        tab = np.stack([(lr_t / bc1).astype(np.float32), np.sqrt(bc2).astype(np.float32)], axis=1)
    return tab


def sgd_update_ref(p: torch.Tensor, buf: torch.Tensor, g: torch.Tensor, first: bool, cfg: OptimConfig,
                   lr: float | None = None) -> None:
    """``lr``: this step's rate under a schedule (``cfg.lr_at(t)``); None: ``cfg.lr``."""
    if cfg.weight_decay:
        g = g + cfg.weight_decay * p
    if cfg.momentum:
        if first:
            buf.copy_(g)
        else:
            buf.mul_(cfg.momentum).add_(g)
        g = buf
    p.add_(g, alpha=-(cfg.lr if lr is None else lr))


def grad_norm_ws(P: int, n_models: int, device) -> torch.Tensor | None:
    """The scratch ``grad_norm`` / a clipped step needs for [n_models, P] rows on ``device``
    (fp64 per-block partials; None where one block per row does it all)."""
    device = torch.device(device)
    if device.type != "cuda" or not nat.native_enabled():
        return None
    nbytes = int(nat.require(device).dtp_grad_norm_ws_bytes(P))
    return torch.empty(n_models * nbytes // 8, dtype=torch.float64, device=device) if nbytes else None


def _rows(flat_grad: torch.Tensor) -> torch.Tensor:
    g = flat_grad if flat_grad.dim() == 2 else flat_grad.view(1, -1)
    if g.dtype != torch.float32 or not g.is_contiguous():
        raise ValueError("expected a contiguous float32 [n_models, P] (or [P]) gradient")
    return g


def _norm_ref(g: torch.Tensor) -> torch.Tensor:
    """Per-row L2 norm, accumulated in float64 and rounded to float32 (what the kernel forms)."""
    return g.double().square().sum(dim=1).sqrt().float()


def _clip_coef_ref(norm: torch.Tensor, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_'s coefficient, its own expression."""
    return (float(max_norm) / (norm + 1e-6)).clamp(max=1.0)


@torch.no_grad()
def grad_norm(flat_grad: torch.Tensor, scale: float = 1.0, out: torch.Tensor | None = None,
              ws: torch.Tensor | None = None) -> torch.Tensor:
    """L2 norm of every row of ``flat_grad * scale`` ([n_models, P] or [P]) -> float32 [n].

    fp64 accumulation in a fixed order: bitwise reproducible, no host sync.  ``out`` / ``ws``
    (``grad_norm_ws``): preallocated result and scratch, for calls under graph capture."""
    g = _rows(flat_grad)
    n, P = g.shape
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=g.device)
    if g.is_cuda and nat.native_enabled():
        lib = nat.require(g.device)
        if ws is None:
            ws = grad_norm_ws(P, n, g.device)
        nat.check(lib.dtp_grad_norm(nat.ptr(g), n, P, scale, nat.ptr(ws), nat.ptr(out), nat.stream_ptr()),
                  "dtp_grad_norm")
        return out
    out.copy_(_norm_ref(g * scale))
    return out


@torch.no_grad()
def clip_grad_norm_(flat_grad: torch.Tensor, max_norm: float, out: torch.Tensor | None = None,
                    ws: torch.Tensor | None = None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` per row of a flat [n_models, P] (or [P]) gradient,
    in place; returns the norms before clipping (float32 [n]).  The norm launch and one
    scale launch (one launch in all for rows of up to 4096 elements): for users who keep a
    torch optimizer over ``FlatDDP.flat_grad``; ``FlatOptimizer`` clips inside its step."""
    if not max_norm > 0:
        raise ValueError("clip_grad_norm_: max_norm must be > 0")
    g = _rows(flat_grad)
    n, P = g.shape
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=g.device)
    if g.is_cuda and nat.native_enabled():
        lib = nat.require(g.device)
        if ws is None:
            ws = grad_norm_ws(P, n, g.device)
        nat.check(lib.dtp_clip_grad_norm(nat.ptr(g), n, P, max_norm, nat.ptr(ws), nat.ptr(out), nat.stream_ptr()),
                  "dtp_clip_grad_norm")
        return out
    out.copy_(_norm_ref(g))
    g.mul_(_clip_coef_ref(out, max_norm).unsqueeze(1))
    return out


def flat_optimizer_step(params, m, v, step, grad, cfg: OptimConfig, grad_scale: float = 1.0,
                        loss_log=None, loss_scale: float = 1.0, slope: float = 0.01, shadow=None,
                        zero_grad: bool = False, fused=None, norm_out=None, norm_ws=None) -> None:
    """One optimizer step over [n_models, P] flat buffers.

    ``grad`` is [n_models*P (+ n_models losses)] -- the all-reduced comm buffer;
    ``step`` is the per-model int32 step counter (device or CPU); ``shadow`` (optional,
    bf16 [n_models, >= P], unit column stride) receives the updated parameters rounded
    to bf16 in the same pass, row i at ``shadow[i, :P]``.  ``zero_grad``: the gradient
    rows are zeroed in the same pass once read (the loss slots are not).  ``fused``: a
    deferred stage backward (``ops.mlp.ParamBackwardFusion``) whose span is exactly this
    optimizer's rows (row i = stage i): the backwards and this step run as one launch.

    Clipping (``cfg.max_grad_norm`` / ``cfg.clip_grad_value``) applies per row to
    ``grad * grad_scale``, the averaged gradient torch would see, inside the same launch
    (rows of more than 4096 elements: one norm launch first).  ``norm_out`` (float32
    [n_models]) receives each row's norm before clipping; ``norm_ws``: ``grad_norm_ws``.
    Both are allocated here when missing -- pass them for a step under graph capture.  A
    clipped step launches ``fused`` backwards first: the norm needs the finished gradient.
    """
    n_models, P = params.shape
    if cfg.max_grad_norm > 0 and cfg.clip_grad_value > 0:
        raise ValueError("flat_optimizer_step: max_grad_norm and clip_grad_value are exclusive")
    by_norm = cfg.max_grad_norm > 0
    if shadow is not None and (shadow.dtype != torch.bfloat16 or shadow.dim() != 2 or shadow.shape[0] != n_models
                               or shadow.shape[1] < P or shadow.stride(1) != 1 or shadow.device != params.device):
        raise ValueError("flat_optimizer_step: shadow must be a bf16 [n_models, >= P] tensor with unit column stride")
    if params.is_cuda and nat.native_enabled():
        lib = nat.require(params.device)
        if by_norm:
            if norm_out is None:
                norm_out = torch.empty(n_models, dtype=torch.float32, device=params.device)
            if norm_ws is None:
                norm_ws = grad_norm_ws(P, n_models, params.device)
        a = nat.OptArgs(nat.ptr(params), nat.ptr(m), nat.ptr(v), nat.ptr(step), nat.ptr(grad),
                        nat.ptr(loss_log), 0 if loss_log is None else loss_log.shape[0], n_models, P, cfg.kind,
                        loss_scale, 1 if zero_grad else 0, cfg.hyper(slope, grad_scale, params.device), nat.ptr(shadow),
                        0 if shadow is None else shadow.stride(0), max(cfg.max_grad_norm, 0.0),
                        max(cfg.clip_grad_value, 0.0), nat.ptr(norm_ws) if by_norm else None,
                        nat.ptr(norm_out) if by_norm else None)
        if fused is not None and cfg.clips:
            for p in fused:
                p.launch()
            fused = None
        if fused is not None:  # the stage backwards that produced `grad`, in the same launch
            from .mlp import launch_fused_with_optimizer

            launch_fused_with_optimizer(fused, a)
            return
        nat.check(lib.dtp_flat_optimizer(ctypes.byref(a), nat.stream_ptr()), "dtp_flat_optimizer")
        return
    if fused is not None:
        for p in fused:
            p.launch()
    g = grad[: n_models * P].view(n_models, P) * grad_scale
    if by_norm:
        norm = _norm_ref(g)
        if norm_out is not None:
            norm_out.copy_(norm)
        g = g * _clip_coef_ref(norm, cfg.max_grad_norm).unsqueeze(1)
    elif cfg.clip_grad_value > 0:
        g = g.clamp(min=-cfg.clip_grad_value, max=cfg.clip_grad_value)
    for i in range(n_models):
        t = int(step[i])
        if cfg.name == "adam":
            adam_update_ref(params[i], m[i], v[i], g[i], t + 1, cfg)
        else:
            sgd_update_ref(params[i], m[i], g[i], t == 0, cfg, cfg.lr_at(t))
        if loss_log is not None:
            loss_log[t % loss_log.shape[0], i] = grad[n_models * P + i] * loss_scale
        step[i] = t + 1
    if zero_grad:
        grad[: n_models * P].zero_()
    if shadow is not None:
        shadow[:, :P].copy_(params)


class FlatOptimizer:
    """Adam/SGD over flat [n_models, P] (or [P]) params + grads in one kernel launch
    (replaces the reference's two torch.optim.Adam, each ~7 kernels x 10 tensors).

    ``cfg.max_grad_norm`` / ``cfg.clip_grad_value`` clip every row's gradient inside the
    same launch (one norm launch more for rows of over 4096 elements); ``grad_norm``
    (float32 [n_models], device) then holds each row's norm before clipping, as
    ``torch.nn.utils.clip_grad_norm_`` returns it, after every step -- no host sync."""

    def __init__(self, flat_params: torch.Tensor, flat_grad: torch.Tensor, cfg: OptimConfig | None = None,
                 slope: float = 0.01, shadow=None):
        """``shadow``: an ``ops.gemm.ComputeShadow`` of ``flat_params``; every step also
        writes its bf16 copy (the bf16-compute forward then needs no weight casts)."""
        self.shadow = shadow
        if shadow is not None and shadow.flat.data_ptr() != flat_params.data_ptr():
            raise ValueError("FlatOptimizer: the shadow must be of flat_params")
        self.params = flat_params if flat_params.dim() == 2 else flat_params.view(1, -1)
        self.grad = flat_grad if flat_grad.dim() == 2 else flat_grad.view(1, -1)
        self.cfg = cfg or OptimConfig()
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.step_ctr = torch.zeros(self.params.shape[0], dtype=torch.int32, device=self.params.device)
        n, P = self.params.shape
        self._buf = None if self.grad.is_contiguous() else \
            torch.zeros(n * P + n, dtype=self.params.dtype, device=self.params.device)
        self.slope = slope
        # clipping by norm: the result and the scratch are made here, never during a capture
        self.grad_norm = torch.zeros(n, dtype=torch.float32, device=self.params.device)
        self._norm_ws = grad_norm_ws(P, n, self.params.device) if self.cfg.max_grad_norm > 0 else None
        # likewise a schedule's device table (cached by the schedule; hyper() finds it there)
        if self.cfg.schedule is not None:
            self.cfg.schedule.device_table(self.params.device)

    @torch.no_grad()
    def step(self, zero_grad: bool = False, fused=None) -> bool:
        """One step; ``zero_grad``: zero the gradient in the same launch (no separate fill
        before the next backward).  ``fused``: deferred stage backwards
        (``ops.mlp.ParamBackwardFusion.take()``): run in the same launch when their spans
        are exactly this optimizer's rows, else launched first.  Returns whether the
        gradient was zeroed (not when it had to be staged through a copy)."""
        # the kernel reads grad[i*P : (i+1)*P] only (the loss slots behind them are
        # read only with a loss log), so a contiguous [n, P] gradient is used in place
        n, P = self.params.shape
        sh = self.shadow
        fresh = sh is not None and sh._token == sh._current()  # else the next forward re-casts anyway
        if fused is not None:
            from .mlp import fused_rows_match

            if fresh or self.cfg.clips or not fused_rows_match(fused, self.params, self.grad):
                for p in fused:
                    p.launch()
                fused = None
        if self.grad.is_contiguous() and self.grad.device == self.params.device:
            buf = self.grad.view(-1)
        else:
            self._buf[: n * P].copy_(self.grad.reshape(-1))
            buf = self._buf
            zero_grad = False
        flat_optimizer_step(self.params, self.m, self.v, self.step_ctr, buf, self.cfg, slope=self.slope,
                            shadow=sh.buf if fresh else None, zero_grad=zero_grad, fused=fused,
                            norm_out=self.grad_norm, norm_ws=self._norm_ws)
        if fresh:
            sh.mark_fresh()
        return zero_grad

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.grad.zero_()

    def state_dict(self) -> dict:
        return {"m": self.m.cpu(), "v": self.v.cpu(), "step": self.step_ctr.cpu()}

    def load_state_dict(self, sd: dict) -> None:
        self.m.copy_(sd["m"])
        self.v.copy_(sd["v"])
        self.step_ctr.copy_(sd["step"])

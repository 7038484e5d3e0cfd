"""Held-out evaluation of n models of one shape: forward, per-sample loss and reduction.

On the GPU this is ONE launch of ``csrc/eval.hip`` for all models (rows past
``one_launch_rows()``: a partial launch and a one-workgroup finalize), stream-ordered, with
no host sync, and capturable into a hipGraph.  The result is the per-model SUM of the
fp32 per-sample losses (and, for cross-entropy, the number of correct argmax predictions)
accumulated in fp64 in a fixed order: a pure function of the arguments, so the sums of
several ranks' shards (``row0 = rank, row_stride = world``) add up to the whole set's with
no padding and no sample counted twice.  CPU tensors take the PyTorch reference of the
same sums.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from .. import _native as nat
from .mlp import MlpSpec, mlp_forward_ref, mlp_forward_ref_bf16


@dataclass
class EvalResult:
    """Per-model sums of :func:`evaluate` ([n_models, 2] float64) over ``count`` samples."""
    sums: torch.Tensor
    count: int
    out_features: int = 1
    loss: str = "mse"

    @property
    def mean_loss(self) -> torch.Tensor:
        """float32 [n_models]: torch's ``reduction='mean'`` value (MSE: over samples x outputs)."""
        d = self.count * (self.out_features if self.loss == "mse" else 1)
        return (self.sums[:, 0] / max(d, 1)).float()

    @property
    def accuracy(self) -> torch.Tensor | None:
        """float32 [n_models] fraction of correct predictions (cross-entropy only)."""
        if self.loss != "ce":
            return None
        return (self.sums[:, 1] / max(self.count, 1)).float()


def one_launch_rows(device=None) -> int:
    """Rows up to which the native evaluation is a single launch with no workspace."""
    return int(nat.require(device).dtp_mlp_eval_one_launch_rows())


def eval_ws(n: int, n_models: int, device) -> torch.Tensor | None:
    """The scratch :func:`evaluate` needs for ``n`` rows (None where one launch does it all)."""
    device = torch.device(device)
    if device.type != "cuda" or not nat.native_enabled():
        return None
    nbytes = int(nat.require(device).dtp_mlp_eval_ws_bytes(int(n), int(n_models)))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device) if nbytes else None


def shard_rows(rows: int, row0: int, row_stride: int) -> int:
    """Number of rows ``row0, row0 + row_stride, ...`` below ``rows``."""
    return 0 if row0 >= rows else (rows - row0 + row_stride - 1) // row_stride


def _evaluate_ref(params, spec, X, Y, loss, bf16, row0, row_stride, n, out):
    rows = row0 + row_stride * torch.arange(n, device=X.device)
    x = X.index_select(0, rows)
    y = Y.reshape(X.shape[0], -1).index_select(0, rows)
    fwd = mlp_forward_ref_bf16 if bf16 else mlp_forward_ref
    for i in range(params.shape[0]):
        o = fwd(params[i], spec, x).float()
        if n == 0:
            out[i].zero_()
        elif loss == "ce":
            cls = y.view(-1).long()
            out[i, 0] = F.cross_entropy(o, cls, reduction="none").double().sum()
            out[i, 1] = (o.argmax(1) == cls).sum().double()
        else:
            out[i, 0] = ((o - y.view_as(o)) ** 2).sum(1).double().sum()
            out[i, 1] = 0.0
    return out


@torch.no_grad()
def evaluate(params: torch.Tensor, spec: MlpSpec, X: torch.Tensor, Y: torch.Tensor, loss: str = "mse",
             bf16: bool = False, row0: int = 0, row_stride: int = 1, n: int | None = None,
             out: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> torch.Tensor:
    """``out[i] = (sum of model i's per-sample losses, correct predictions)`` over the rows
    ``row0 + k * row_stride`` (k < n; default: every such row of X) -> float64 [n_models, 2]
    on ``params``' device.

    ``params``: [n_models, P] (or [P]) flat fp32 rows in torch order; ``Y``: [rows, OUT]
    targets (``mse``: the sum over outputs of the squared error per sample) or [rows] /
    [rows, 1] class ids as float (``ce``).  ``bf16``: the bf16-compute forward the bf16
    engines train with (the loss itself stays fp32).  ``out`` / ``ws`` (:func:`eval_ws`):
    preallocated result and scratch for calls under graph capture."""
    if loss not in ("mse", "ce"):
        raise ValueError(f"loss {loss!r}: mse or ce")
    if spec.final_act:
        raise ValueError("evaluate: the model must end without an activation")
    if params.dim() == 1:
        params = params.view(1, -1)
    dev = params.device
    if params.dim() != 2 or params.shape[1] != spec.P or params.dtype != torch.float32 or not params.is_contiguous():
        raise ValueError(f"params must be contiguous float32 [n_models, {spec.P}], got {tuple(params.shape)} "
                         f"{params.dtype}")
    if X.dim() != 2 or X.shape[1] != spec.in_features:
        raise ValueError(f"X must be [rows, {spec.in_features}], got {tuple(X.shape)}")
    rows = X.shape[0]
    want = rows * (spec.out_features if loss == "mse" else 1)
    for name, t in (("X", X), ("Y", Y)):
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 tensor on {dev}")
    if Y.numel() != want:
        raise ValueError(f"Y must have {want} elements for loss {loss!r}, got {Y.numel()}")
    row0, row_stride = int(row0), int(row_stride)
    if row0 < 0 or row_stride < 1:
        raise ValueError("row0 >= 0 and row_stride >= 1")
    avail = shard_rows(rows, row0, row_stride)
    n = avail if n is None else int(n)
    if n < 0 or n > avail:
        raise ValueError(f"n = {n}: rows {row0}::{row_stride} of {rows} are {avail}")
    n_models = params.shape[0]
    if out is None:
        out = torch.empty(n_models, 2, dtype=torch.float64, device=dev)
    elif out.shape != (n_models, 2) or out.dtype != torch.float64 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be contiguous float64 [{n_models}, 2] on {dev}")
    if not (dev.type == "cuda" and nat.native_enabled()):
        return _evaluate_ref(params, spec, X, Y, loss, bf16, row0, row_stride, n, out)
    lib = nat.require(dev)
    if not (lib.dtp_mlp_supported_bf16(*spec.key) if bf16 else lib.dtp_mlp_supported(*spec.key)):
        raise NotImplementedError(f"no {'bf16 ' if bf16 else ''}eval kernel instantiated for {spec}")
    need = int(lib.dtp_mlp_eval_ws_bytes(n, n_models))
    if need and (ws is None or ws.numel() * ws.element_size() < need or ws.device != dev):
        ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    a = nat.EvalArgs(nat.ptr(X), nat.ptr(Y), nat.ptr(params), nat.ptr(out), nat.ptr(ws) if need else None,
                     row0, row_stride, n, n_models, nat.LOSS_CE if loss == "ce" else nat.LOSS_MSE, int(bool(bf16)),
                     spec.slope)
    nat.check(lib.dtp_mlp_eval(ctypes.byref(a), *spec.key[:4], nat.stream_ptr()), "dtp_mlp_eval")
    return out


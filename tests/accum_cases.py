"""Gradient accumulation inside the fused step (``csrc/accum_core.h``): the accumulation twins of
the several-lanes / split-batch update instances, one cell per twin, and the read-out protocol.

Shared by ``tests/test_fused_accum_gpu.py`` and ``tests/test_fused_accum_cpu.py``; CPU-only code
except :func:`run_accum_cell` and the other run helpers, which drive ``FusedTrainer`` engines on
whatever device they are given.  Data, initial weights, sampler seed, optimizers and the
gradient read-out through the optimizer state are those of ``tests/step_cases.py``.

**Semantics.**  Optimizer step ``t`` of an engine with ``accumulate = A`` consumes the micro-batches
``t A .. t A + A - 1`` of the rank's sampler order; its gradient is the mean over them of the
gradient of each one's mean loss (a ragged batch divided by its own count), its logged loss the
mean of their mean losses.

**Twins.**  ``TWINS`` is written out from ``lanes_fill()`` of ``csrc/mlp_train_lanes_kernel.h``
(the ``kAccum`` rows of ``LanesInst.lanes`` and ``LanesInst.grp``, the local modes), NOT derived
from the cells: 2 and 4 lanes of all eight families, and for the five split-batch families the run-time member count (``grp``) and
the constant 4 (``grp4``).

**Geometries**, the smallest that reach each path and put a ragged batch and an epoch edge inside
a window (read out: optimizer steps 0, 1, 2, one launch each):

* 4 lanes: n = 300, batch 64, A = 3 -- 5 batches per epoch, the last of 44 samples: windows
  (0 1 2) (3 4 | 0) (1 2 3);
* 2 lanes: n = 300, batch 100, A = 2 -- windows (0 1) (2 | 0) (1 2);
* split-batch, run-time count: n = 512, batch 192, 3 members, A = 2 -- the epoch's last batch has
  128 samples and leaves the third member empty: windows (0 1) (2 | 0) (1 2);
* split-batch with two members empty: n = 512, batch 200, A = 3 -- 4 members, so the dispatcher
  takes the constant-count instance and the cell names ``grp4``; the last batch has 112 samples;
* split-batch, constant 4: n = 512, batch 256, A = 2;
* the toy fp32 Adam 4-lanes cell once more at A = 8.

**Reference and bound** (:func:`evaluate_window`): ``step_cases.evaluate_step``'s several-ranks
rule with micro-batches in place of ranks -- the reference is the mean over the window's
micro-batches of fp64 autograd on ``step_indices(u)`` at the snapshot parameters (the loss: of
their mean losses); ``Y`` is fp32 CPU autograd per micro-batch, summed in fp32 in order, times
fp32 ``1 / A``; ``E <= max(4 Y, 8 * 2^-24)`` plus the CE margin for CE, and the bf16 rule for bf16.

**Conditions on the inputs** (``step_cases.check_conditions``), from the references alone along
the CPU engine's trajectory: ``tests/test_fused_accum_cpu.py``.  The seeds of ``step_cases`` (data
21, init 1, sampler 5) were the first tried for these cells.
"""
from __future__ import annotations

import functools
import json
import sys
from dataclasses import dataclass, replace
from typing import NamedTuple

import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream
from distributed_training_pytorch_amd.ops.optim import OptimConfig

from . import step_cases as sc
from .ref_train import torch_train

READOUT_STEPS = (0, 1, 2)


# ------------------------------------------------------------------------------ the twins
# DTP_LANES_FAMILIES as (shape, loss, optimizer, precision, has split-batch instances)
FAMILIES = [("T", "mse", "adam", "fp32", True), ("T", "mse", "sgd", "fp32", True), ("T", "mse", "adam", "bf16", True),
            ("C4", "ce", "adam", "fp32", True), ("C4", "ce", "sgd", "fp32", True),
            ("N3", "mse", "adam", "fp32", False), ("C4", "mse", "adam", "fp32", False), ("H15", "mse", "adam", "fp32", False)]


def _twins():
    """(shape, lanes, waves, loss, optimizer, precision, kind) of every accumulation twin of the
    local update modes; kind: lanes, grp (run-time member count), grp4."""
    out = []
    for L in (2, 4):  # LanesInst.lanes[kAccum][4 waves][L][local]
        out += [(s, L, 4, lo, o, p, "lanes") for s, lo, o, p, _ in FAMILIES]
    for kind in ("grp", "grp4"):  # LanesInst.grp[kAccum][0..1]
        out += [(s, 4, 4, lo, o, p, kind) for s, lo, o, p, g in FAMILIES if g]
    return out


TWINS = _twins()


@dataclass(frozen=True)
class AccumCell:
    cell: sc.Cell  # one rank (world = 1) or several: geometry, the instance the plain launch picks
    A: int

    @property
    def id(self) -> str:
        return f"{self.cell.id}-A{self.A}"

    @property
    def twin(self) -> tuple:
        shape, lanes, waves, loss, opt, prec, kind = self.cell.instance
        if kind == "grp" and self.cell.expect[2] == 4:
            kind = "grp4"
        return (shape, lanes, waves, loss, opt, prec, kind)


def _cells():
    out = []
    for s, lo, o, p, _ in FAMILIES:
        out.append(AccumCell(sc._lanes(s, o, lo, 64, 4, prec=p, n=300), 3))
    for s, lo, o, p, _ in FAMILIES:
        out.append(AccumCell(sc._lanes(s, o, lo, 100, 2, prec=p, n=300), 2))
    for s, lo, o, p, g in FAMILIES:
        if g:
            out.append(AccumCell(sc._grp(s, o, lo, 192, 3, prec=p), 2))
    out.append(AccumCell(sc._grp("T", "adam", "mse", 200, 4), 3))  # two members empty in the last batch
    for s, lo, o, p, g in FAMILIES:
        if g:
            out.append(AccumCell(sc._grp(s, o, lo, 256, 4, prec=p), 2))
    out.append(AccumCell(sc._lanes("T", "adam", "mse", 64, 4, n=300), 8))
    return out


CELLS = _cells()
BY_ID = {c.id: c for c in CELLS}
assert len(BY_ID) == len(CELLS), "duplicate cell ids"

LANES4 = BY_ID["T-adam-mse-fp32-b64-goff-n300-A3"]
GRP4 = BY_ID["T-adam-mse-fp32-b256-gon-A2"]

# several ranks on one GPU (the xGMI twins): world 2 on the split-batch twin (n = 512: a rank's 256
# samples are one batch of 256, so every window of 2 crosses an epoch), world 3 on a 4-lanes twin
# (n = 300: 100 samples per rank, batches of 64 and 36, a window is an epoch)
WORLD_CELLS = {
    2: AccumCell(replace(sc._grp("T", "adam", "mse", 256, 4), world=2), 2),
    3: AccumCell(replace(sc._lanes("T", "adam", "mse", 64, 4, n=300), world=3), 2),
}


# ------------------------------------------------------------------------------ windows
class WindowView:
    """Micro-batch j of every window of a rank's sampler order as an object with ``indices(t)``:
    ``ref_train.torch_train`` over the A views of a rank is the fp64 loop extended by
    accumulation (it takes the mean of its geoms' gradients and of their mean losses)."""

    def __init__(self, stream, A: int, j: int):
        self.stream, self.A, self.j = stream, A, j

    def indices(self, t: int) -> list[int]:
        return self.stream.indices(t * self.A + self.j)


def window_views(cell: sc.Cell, A: int, shift: int = 0) -> list:
    """The views of every rank and micro-batch, rank-major (``shift``: the data position moved by
    that many batches, for the tests of the tests)."""
    out = []
    for r in range(cell.world):
        stream = EpochIndexStream(sc.cell_geom(cell, r))
        if shift:
            stream = _Shifted(stream, shift)
        out += [WindowView(stream, A, j) for j in range(A)]
    return out


class _Shifted:
    def __init__(self, stream, shift):
        self.stream, self.shift = stream, shift

    def indices(self, u):
        return self.stream.indices(u + self.shift)


def window_indices(ac: AccumCell, t: int) -> list[list[int]]:
    """The index lists of optimizer step t: every rank's micro-batches, rank-major."""
    return [v.indices(t) for v in window_views(ac.cell, ac.A)]


def evaluate_window(ac: AccumCell, sg: sc.StepGradient, indices: list[list[int]], X, Y,
                    n_models: int = sc.N_MODELS) -> tuple[list[dict], list[str]]:
    """Records and failures of one read-out of an accumulating engine against the references:
    ``step_cases.evaluate_step``'s several-ranks rule over the window's (ranks x) micro-batches."""
    assert len(indices) == ac.cell.world * ac.A
    if len(indices) == 1:  # one rank, one micro-batch: the plain step's evaluation
        return sc.evaluate_step(replace(ac.cell, world=1), sg, indices[0], X, Y, n_models)
    return sc.evaluate_step(replace(ac.cell, world=len(indices)), sg, indices, X, Y, n_models)


def accum_optim(ac: AccumCell, **kw) -> OptimConfig:
    return replace(sc.ADAM if ac.cell.opt == "adam" else sc.SGD, **kw)


def make_trainer(ac: AccumCell, device, optim: OptimConfig | None = None, rank: int = 0, A: int | None = None, **cfg):
    """``step_cases.make_trainer`` with ``accumulate`` (and, optionally, another OptimConfig)."""
    from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer

    cell = ac.cell
    X, Y = sc.cell_data(cell)
    ecfg = EngineConfig(**{"steps_per_launch": sc.STEPS_PER_LAUNCH, "loss": cell.loss, "groups": cell.groups,
                           "cache_data": cell.cache, "precision": cell.prec, "accumulate": ac.A if A is None else A,
                           **cfg})
    return FusedTrainer(cell.spec, sc.N_MODELS, X.to(device), Y.to(device), sc.cell_geom(cell, rank),
                        optim or accum_optim(ac), ecfg, init_params=[p.to(device) for p in sc.cell_init(cell)])


# ------------------------------------------------------------------------------ a cell
def run_accum_cell(ac: AccumCell, device, expect_native: bool = True) -> tuple[list[dict], list[str]]:
    """The cell's read-outs at optimizer steps 0, 1, 2 (one launch each, the moments zeroed in
    between) on ``device`` against the references: (records, failures)."""
    cell = ac.cell
    X, Y = sc.cell_data(cell)
    tr = make_trainer(ac, device)
    recs, fails = [], []
    try:
        inst = (tr.lanes, tr.kernel_waves, tr.groups)
        if expect_native and (inst != cell.expect or not tr.accum_in_kernel):
            return [], [f"{ac.id}: the dispatcher picked (lanes, waves, groups) = {inst}, accum_in_kernel "
                        f"{tr.accum_in_kernel}; expected {cell.expect}, a twin"]
        for t in READOUT_STEPS:
            sg = sc.step_gradient(tr)
            assert sg.t == t and list(tr.micro_batches(t)) == list(range(t * ac.A, (t + 1) * ac.A))
            idx = [tr.step_indices(u) for u in tr.micro_batches(t)]
            assert idx == window_indices(ac, t)
            r, f = evaluate_window(ac, sg, idx, X, Y)
            for x in r:
                x["instance"], x["A"] = list(inst), ac.A
            if t == 0 and cell.prec == "bf16" and device.type == "cuda":
                tw = make_trainer(ac, device, precision="fp32")
                try:
                    g32 = sc.step_gradient(tw).grad
                finally:
                    tw.close()
                for i, x in enumerate(r):
                    if torch.equal(sg.grad[i], g32[i]):
                        f.append(f"{ac.id} model {i}: the bf16 read-out equals the fp32 twin's")
            recs += r
            fails += f
        tr.check_comm()
        if tr.step_ctr.tolist() != [tr.t] * sc.N_MODELS:
            fails.append(f"{ac.id}: step counters {tr.step_ctr.tolist()} != {tr.t}")
    finally:
        tr.close()
    if cell.prec == "bf16":
        fails += sc.check_bf16(cell, recs)
    return recs, fails


def loss_failures(ac: AccumCell, p_before: torch.Tensor, t: int, loss: torch.Tensor) -> list[str]:
    """The logged loss of optimizer step t (taken at parameters ``p_before``) against the reference
    by the read-out's loss bound."""
    cell = ac.cell
    X, Y = sc.cell_data(cell)
    sg = sc.StepGradient(t, p_before, None, loss, None)
    recs, _ = evaluate_window(ac, sg, window_indices(ac, t), X, Y)
    fails = []
    for i, r in enumerate(recs):
        views = window_views(cell, ac.A)
        if cell.prec == "bf16":
            from distributed_training_pytorch_amd.ops.mlp import mlp_forward_ref_bf16 as fwd
            bound = max(r["D"].values()) / 2
        else:
            from distributed_training_pytorch_amd.ops.mlp import mlp_forward_ref as fwd
            bound = r["bound_loss"]
        ls = []
        for v in views:
            ix = torch.tensor(v.indices(t), dtype=torch.long)
            ls.append(sc.autograd_gradient(cell.spec, p_before[i], X[ix], Y[ix], cell.loss, torch.float64, fwd)[1])
        ref = sum(ls) / len(ls)
        e = sc.rel(loss[i], ref)
        if not e <= bound:
            fails.append(f"{ac.id} t={t} model {i} loss: E {e:.3e} > bound {bound:.3e}")
    return fails


# ------------------------------------------------------------------------------ clipping bounds
class Bounds(NamedTuple):
    c_bind: float
    c_free: float
    c_val: float


@functools.lru_cache(maxsize=None)
def _bounds(shape, opt, loss, batch, n, A) -> Bounds:
    """``clip_step_cases.bounds`` for an accumulating cell, from the reference alone: the fp64
    norms of both models' window gradients at the read-out steps along the unclipped fp64 loop;
    half the smallest, twice the largest, the median of ``|g64|`` at step 0."""
    cell = sc.Cell(shape, opt, loss, batch, (0, 0, 0), "cpu", n=n)
    ac = AccumCell(cell, A)
    X, Y = sc.cell_data(cell)
    views = window_views(cell, A)
    norms, c_val = [], None
    for t in READOUT_STEPS:
        p, _ = torch_train(cell.spec, sc.cell_init(cell), X, Y, views, t, accum_optim(ac), loss)
        gs = []
        for i in range(sc.N_MODELS):
            g = None
            for v in views:
                ix = torch.tensor(v.indices(t), dtype=torch.long)
                gr, _ = sc.autograd_gradient(cell.spec, p[i], X[ix], Y[ix], loss, torch.float64)
                g = gr if g is None else g + gr
            gs.append(g / A)
        norms += [g.norm().item() for g in gs]
        if c_val is None:
            c_val = torch.cat(gs).abs().median().item()
    return Bounds(0.5 * min(norms), 2.0 * max(norms), c_val)


def bounds(ac: AccumCell) -> Bounds:
    c = ac.cell
    return _bounds(c.shape, c.opt, c.loss, c.batch, c.n, ac.A)


# ------------------------------------------------------------------------------ child processes
def twin_state(ac: AccumCell, device, A: int = 1) -> dict:
    """3 steps in one launch, then 3 one-step launches, of the cell's configuration at
    ``accumulate = A``: the state, the loss rows and the parameters before each of the last 3."""
    tr = make_trainer(ac, device, A=A)
    try:
        out = {"pick": [tr.lanes, tr.kernel_waves, tr.groups], "twin": bool(tr.accum_in_kernel), "before": []}
        tr.train(3)
        for _ in range(3):
            tr.synchronize()
            out["before"].append(tr.params.detach().cpu().clone())
            tr.train(1)
        tr.synchronize()
        out.update(params=tr.params.cpu(), m=tr.m.cpu(), v=tr.v.cpu(), step=tr.step_ctr.cpu(), t=tr.t,
                   losses=tr.losses(0, 6))
    finally:
        tr.close()
    return out


def main(argv: list[str]) -> int:
    """Child process of the forced-environment tests: ``python -m tests.accum_cases twin OUT.pt
    CELL_ID...`` runs :func:`twin_state` at A = 1 (under the caller's environment) on GPU 0;
    ``pick OUT.json CELL_ID`` reports what an accumulating engine of the cell resolves to."""
    what, out, ids = argv[0], argv[1], argv[2:]
    dev = torch.device("cuda", 0)
    if what == "twin":
        torch.save({cid: twin_state(BY_ID[cid], dev) for cid in ids}, out)
        return 0
    if what == "pick":
        res = {}
        for cid in ids:
            try:
                tr = make_trainer(BY_ID[cid], dev)
                try:
                    tr.train(1)
                    tr.synchronize()
                    res[cid] = {"error": None, "pick": [tr.lanes, tr.kernel_waves, tr.groups]}
                finally:
                    tr.close()
            except Exception as e:
                res[cid] = {"error": f"{type(e).__name__}: {e}"}
        with open(out, "w") as fh:
            json.dump(res, fh)
        return 0
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

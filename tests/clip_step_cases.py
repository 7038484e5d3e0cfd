"""Gradient clipping inside the fused step (``csrc/clip_core.h``): the clip twins of the update
instances, one cell per twin, the cells' clipping bounds and the read-out protocol.

Shared by ``tests/test_fused_clip_gpu.py`` and ``tests/test_fused_clip_cpu.py``; CPU-only code
except :func:`run_clip_cell` and :func:`world_rank`, which drive ``FusedTrainer`` engines on
whatever device they are given.  Cells, inputs and the gradient read-out through the optimizer
state are those of ``tests/step_cases.py``.

**Twins.**  ``TWINS`` is written out from the tables of ``csrc/mlp_train_one.hip`` (one_row():
the generic instance in the update modes) and ``csrc/mlp_train_lanes_kernel.h`` (lanes_fill():
the ``kClip`` rows of ``LanesInst.lanes`` and ``LanesInst.grp``), NOT derived from the cells.
A twin's cell is the first cell of
``step_cases.CELLS`` that runs its plain instance; a FAST cell stands for the generic twin of
its row (a clipped one-lane launch has no FAST instance).  The split-batch families have two
local twins: the run-time member count (``grp``) and the constant 4 (``grp4``).

**Bounds** (:func:`bounds`), from the reference alone: the fp64 autograd norms of both models at
the cell's ``readout_steps`` along the unclipped ``ref_train.torch_train`` trajectory;
``C_bind`` = half the smallest, ``C_free`` = twice the largest, ``c_val`` = the median of
``|g64|`` over both models at step 0.

**Protocol** (:func:`clip_readout`, :func:`evaluate_readout`).  Engine A is plain and walks the
trajectory; engine B has ``max_grad_norm = C_bind``.  At a read-out step B loads A's state, both
zero their moments and run one step.  ``gA = A.m`` is A's gradient bit for bit
(``step_cases``), and B -- the same source compiled with ``-ffp-contract=off`` -- must have formed
the same one, so:

* ``B.grad_norm[i]`` is ``float32(sqrt(sum(gA[i].double() ** 2)))`` or an adjacent float32: an
  fp64 sum of at most 782 exact squares is off by far less than 2^-24 relative, so only a
  double-rounding tie can move the result, by one float32;
* ``B.m[i] == gA[i] * coef`` under ``torch.equal`` with torch's own
  ``coef = (C / (n + 1e-6)).clamp(max=1)`` on the norm B reported, and ``coef < 1``;
* ``step_cases.applied_is_stored`` holds for B, and B's logged loss equals A's bitwise.

``C_free`` must leave ``m``, ``v``, the parameters and the loss those of A; by value
``B.m == gA.clamp(-c_val, c_val)`` with 10 % .. 90 % of the elements clamped.
"""
from __future__ import annotations

import functools
from dataclasses import replace
from typing import NamedTuple

import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.optim import OptimConfig

from . import step_cases as sc
from .ref_train import torch_train


# ------------------------------------------------------------------------------ the twins
def _twins():
    """(shape, lanes, waves, loss, optimizer, precision, kind) of every clip twin of the local
    update modes; kind: generic (one lane), lanes, grp (run-time member count), grp4."""
    out = []
    # DTP_ONE_SHAPES x OneInst.fn[kClip][ADAM, SGD]; the generic kernel takes the loss at run time
    for prec, shapes in (("fp32", ("T", "N3", "C4", "H15")), ("bf16", ("T", "C4"))):
        for s in shapes:
            out += [(s, 1, 4, "mse", "adam", prec, "generic"), (s, 1, 4, "mse", "sgd", prec, "generic")]
            if s == "C4":
                out += [(s, 1, 4, "ce", "adam", prec, "generic"), (s, 1, 4, "ce", "sgd", prec, "generic")]
    # DTP_LANES_FAMILIES x LanesInst.lanes[kClip][4 waves][L][local]: 4 waves only
    for L in (2, 4):
        out += [(s, L, 4, "mse", "adam", "fp32", "lanes") for s in ("T", "N3", "C4", "H15")]
        out += [("T", L, 4, "mse", "sgd", "fp32", "lanes"), ("C4", L, 4, "ce", "adam", "fp32", "lanes"),
                ("C4", L, 4, "ce", "sgd", "fp32", "lanes"), ("T", L, 4, "mse", "adam", "bf16", "lanes")]
    # LanesInst.grp[kClip][0..1] of the five split-batch families
    for kind in ("grp", "grp4"):
        out += [("T", 4, 4, "mse", "adam", "fp32", kind), ("T", 4, 4, "mse", "sgd", "fp32", kind),
                ("T", 4, 4, "mse", "adam", "bf16", kind), ("C4", 4, 4, "ce", "adam", "fp32", kind),
                ("C4", 4, 4, "ce", "sgd", "fp32", kind)]
    return out


TWINS = _twins()


def twin_of(cell: sc.Cell) -> tuple:
    """The clip twin a clipping engine runs on the cell's configuration."""
    shape, lanes, waves, loss, opt, prec, kind = cell.instance
    if kind == "fast":
        kind = "generic"
    if kind == "grp" and cell.expect[2] == 4:
        kind = "grp4"
    return (shape, lanes, waves, loss, opt, prec, kind)


def _first_cells():
    out = {}
    for c in sc.CELLS:
        out.setdefault(twin_of(c), c)
    return out


_FIRST = _first_cells()
# one cell per twin, in the table's order (a twin without a cell: test_fused_clip_cpu.py)
CLIP_CELLS = [_FIRST[t] for t in TWINS if t in _FIRST]
# one cell per kernel family for the C_free and by-value checks: one lane, 2 lanes, 4 lanes,
# split-batch with 4 members and with 3 (the third: 2 samples, none in the last batch), bf16
SUBSET_IDS = ["T-adam-mse-fp32-b256-goff", "T-sgd-mse-fp32-b128-goff", "C4-adam-ce-fp32-b50-goff",
              "T-adam-mse-fp32-b256-gon", "T-sgd-mse-fp32-b130-gon", "T-adam-mse-bf16-b128-goff"]

# several ranks on one GPU: the xGMI twins (W x members slots; per-rank batches)
_lanes, _one, _grp = sc._lanes, sc._one, sc._grp
WORLD_CELLS = {
    2: [replace(_grp("T", "adam", "mse", 256, 4), world=2),            # the split-batch xGMI twin, 2 x 4 slots
        replace(_lanes("T", "sgd", "mse", 128, 2), world=2)],          # the 2-lanes xGMI twin
    3: [replace(_lanes("C4", "adam", "ce", 64, 4), world=3),           # the 4-lanes xGMI twin
        replace(_one("N3", "sgd", "mse", 64, "generic"), world=3)],    # the generic one-lane xGMI twin
}
WORLD_BY_ID = {c.id: c for cs in WORLD_CELLS.values() for c in cs}


# ------------------------------------------------------------------------------ bounds
class Bounds(NamedTuple):
    c_bind: float
    c_free: float
    c_val: float
    norms: tuple     # fp64 norms [(model 0, model 1) per read-out step]
    clamped: tuple   # share of |g64| > c_val per read-out step


def clip_optim(cell: sc.Cell, **clip) -> OptimConfig:
    return replace(sc.ADAM if cell.opt == "adam" else sc.SGD, **clip)


@functools.lru_cache(maxsize=None)
def _bounds(shape, opt, loss, batch, n, world) -> Bounds:
    cell = sc.Cell(shape, opt, loss, batch, (0, 0, 0), "cpu", n=n, world=world)
    X, Y = sc.cell_data(cell)
    geoms = [EpochIndexStream(sc.cell_geom(cell, r)) for r in range(world)]
    norms, c_val, clamped = [], None, []
    for t in sc.readout_steps(cell):
        p, _ = torch_train(cell.spec, sc.cell_init(cell), X, Y, geoms, t, clip_optim(cell), loss)
        gs = []
        for i in range(sc.N_MODELS):
            g = None
            for ix in sc.cell_indices(cell, t):
                ix = torch.tensor(ix, dtype=torch.long)
                gr, _ = sc.autograd_gradient(cell.spec, p[i], X[ix], Y[ix], loss, torch.float64)
                g = gr if g is None else g + gr
            gs.append(g / world)
        norms.append(tuple(g.norm().item() for g in gs))
        a = torch.cat(gs).abs()
        if c_val is None:
            c_val = a.median().item()
        clamped.append((a > c_val).double().mean().item())
    flat = [x for row in norms for x in row]
    return Bounds(0.5 * min(flat), 2.0 * max(flat), c_val, tuple(norms), tuple(clamped))


def bounds(cell: sc.Cell) -> Bounds:
    """The cell's clipping bounds (module docstring); cells that differ only in instance, cache,
    groups or precision share them (the reference is the fp32 model in fp64)."""
    return _bounds(cell.shape, cell.opt, cell.loss, cell.batch, cell.n, cell.world)


# ------------------------------------------------------------------------------ engines
def make_clip_trainer(cell: sc.Cell, device, optim: OptimConfig, rank: int = 0, **cfg) -> FusedTrainer:
    """``step_cases.make_trainer`` with another OptimConfig."""
    X, Y = sc.cell_data(cell)
    ecfg = EngineConfig(**{"steps_per_launch": sc.STEPS_PER_LAUNCH, "loss": cell.loss, "groups": cell.groups,
                           "cache_data": cell.cache, "precision": cell.prec, **cfg})
    return FusedTrainer(cell.spec, sc.N_MODELS, X.to(device), Y.to(device), sc.cell_geom(cell, rank), optim, ecfg,
                        init_params=[p.to(device) for p in sc.cell_init(cell)])


class ClipReadout(NamedTuple):
    t: int
    params_before: torch.Tensor  # [n_models, P], CPU
    g_plain: torch.Tensor        # A.m: the step's gradient
    loss_plain: torch.Tensor
    m_plain: torch.Tensor        # A's state after the step
    v_plain: torch.Tensor
    params_plain: torch.Tensor
    m: torch.Tensor              # B's
    v: torch.Tensor
    params: torch.Tensor
    loss: torch.Tensor
    norm: torch.Tensor | None    # B.grad_norm


def clip_readout(A: FusedTrainer, Bs: dict) -> dict:
    """One read-out step of the protocol: every engine of ``Bs`` loads A's state, all zero their
    moments and run step ``A.t``.  Returns {name: ClipReadout}.  Several ranks: every rank calls
    this at the same step (a process-group barrier in front of every launch)."""
    import torch.distributed as dist

    world = A.world
    A.synchronize()
    sd = A.state_dict()
    t = A.t
    p0 = A.params.detach().cpu().clone()

    def one(tr):
        tr.m.zero_()
        tr.v.zero_()
        if world > 1:
            dist.barrier()
        tr.train(1)
        tr.synchronize()
        assert tr.t == t + 1
        return (tr.m.detach().cpu().clone(), tr.v.detach().cpu().clone(), tr.params.detach().cpu().clone(),
                tr.losses(t, t + 1)[0].clone())

    out = {}
    for name, B in Bs.items():
        B.load_state_dict(sd)
    mA, vA, pA, lA = one(A)
    for name, B in Bs.items():
        m, v, p, lo = one(B)
        norm = None if B.grad_norm is None else B.grad_norm.detach().cpu().clone()
        out[name] = ClipReadout(t, p0, mA, lA, mA, vA, pA, m, v, p, lo, norm)
    return out


def _adjacent(a: torch.Tensor, b: torch.Tensor) -> bool:
    """a is b or a float32 next to it."""
    inf = torch.tensor(float("inf"))
    return bool(a == b or a == torch.nextafter(b, inf) or a == torch.nextafter(b, -inf))


def evaluate_readout(cell: sc.Cell, ro: ClipReadout, kind: str, c: float) -> list[str]:
    """Failures of one read-out of a clipping engine (kind: bind | free | value; c: its bound)
    against the plain engine's, per the module docstring."""
    fails, tag = [], f"{cell.id} {kind} t={ro.t}"
    if not torch.equal(ro.loss, ro.loss_plain):
        fails.append(f"{tag}: the logged loss differs from the plain engine's")
    if kind == "free":
        for name in ("m", "v", "params"):
            if not torch.equal(getattr(ro, name), getattr(ro, name + "_plain")):
                fails.append(f"{tag}: {name} differs from the plain engine's under a bound that cannot bind")
        return fails
    if kind == "value":
        cl = ro.g_plain.clamp(-c, c)
        for i in range(ro.m.shape[0]):
            if not torch.equal(ro.m[i], cl[i]):
                fails.append(f"{tag} model {i}: m != gA.clamp(-c, c) at {int((ro.m[i] != cl[i]).sum())} elements")
        share = (ro.g_plain.abs() > c).double().mean().item()
        if not 0.1 <= share <= 0.9:
            fails.append(f"{tag}: {share:.2f} of the elements are clamped")
    else:
        if ro.norm is None:
            return fails + [f"{tag}: no grad_norm"]
        for i in range(ro.m.shape[0]):
            want = ro.g_plain[i].double().square().sum().sqrt().float()
            if not _adjacent(ro.norm[i], want):
                fails.append(f"{tag} model {i}: grad_norm {ro.norm[i].item():.9g}, the gradient's {want.item():.9g}")
            coef = (float(c) / (ro.norm[i] + 1e-6)).clamp(max=1.0)
            if not coef < 1:
                fails.append(f"{tag} model {i}: the bound does not bind (coef {coef.item()})")
            if not torch.equal(ro.m[i], ro.g_plain[i] * coef):
                bad = int((ro.m[i] != ro.g_plain[i] * coef).sum())
                fails.append(f"{tag} model {i}: m != gA * coef at {bad} elements")
    sg = sc.StepGradient(ro.t, ro.params_before, ro.m, ro.loss, ro.params)
    for i in range(ro.m.shape[0]):
        fails += [f"{tag} model {i}: {m}" for m in sc.applied_is_stored(cell, sg, i)]
    return fails


def run_clip_cell(cell: sc.Cell, device, subset: bool, expect_native: bool = True) -> tuple[list, list[str]]:
    """The protocol over the cell's read-out steps on ``device``: (read-outs, failures)."""
    b = bounds(cell)
    kinds = {"bind": ("max_grad_norm", b.c_bind)}
    if subset:
        kinds.update(free=("max_grad_norm", b.c_free), value=("clip_grad_value", b.c_val))
    A = sc.make_trainer(cell, device)
    Bs = {k: make_clip_trainer(cell, device, clip_optim(cell, **{f: c})) for k, (f, c) in kinds.items()}
    ros, fails = [], []
    try:
        if expect_native:
            for k, B in Bs.items():
                pick = (B.lanes, B.kernel_waves, B.groups)
                if not B.clip_in_kernel or pick != cell.expect:
                    fails.append(f"{cell.id} {k}: clip_in_kernel {B.clip_in_kernel}, pick {pick}, expected {cell.expect}")
            if fails:
                return ros, fails
        for t in sc.readout_steps(cell):
            if A.t < t:
                A.train(t - A.t)
            r = clip_readout(A, Bs)
            for k, ro in r.items():
                assert ro.t == t
                fails += evaluate_readout(cell, ro, k, kinds[k][1])
            ros.append(r)
        for tr in (A, *Bs.values()):
            tr.check_comm()
    finally:
        for tr in (A, *Bs.values()):
            tr.close()
    return ros, fails


# ------------------------------------------------------------------------------ several ranks
def run_world_cell(cell: sc.Cell, device, rank: int) -> dict:
    """One rank's part of the protocol on a cell of several ranks (raw; the parent evaluates)."""
    b = bounds(cell)
    out = {"cell": cell.id, "rank": rank, "readouts": [], "fails": []}
    A = sc.make_trainer(cell, device, rank=rank)
    B = make_clip_trainer(cell, device, clip_optim(cell, max_grad_norm=b.c_bind), rank=rank)
    try:
        out["pick"] = [B.lanes, B.kernel_waves, B.groups]
        out["comm"], out["fallback"], out["clip"] = B.comm, B.comm_fallback_reason, B.clip_in_kernel
        ok = B.comm == "xgmi" and A.comm == "xgmi" and tuple(out["pick"]) == cell.expect and B.clip_in_kernel
        if not sc._all_ranks(ok):
            return out
        import torch.distributed as dist

        for t in sc.readout_steps(cell):
            err = None
            try:
                if A.t < t:
                    dist.barrier()
                    A.train(t - A.t)
                out["readouts"].append(tuple(clip_readout(A, {"bind": B})["bind"]))
            except Exception as e:  # an exchange timeout, a launch error
                err = f"rank {rank} t={t}: {type(e).__name__}: {e}"
                out["fails"].append(err)
            if not sc._all_ranks(err is None):
                return out
        out["comm_after"], out["fallback_after"] = B.comm, B.comm_fallback_reason
    finally:
        A.close()
        B.close()
    return out


def world_rank(rank: int, world: int, cell_ids: list[str]) -> dict:
    """What one spawn runs on every rank: the cells in order, stopping at the first failure on
    any rank.  Nothing is retried."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"cells": {}, "stopped": None}
    for cid in cell_ids:
        err = None
        try:
            o = out["cells"][cid] = run_world_cell(WORLD_BY_ID[cid], dev, rank)
            if o["fails"] or len(o["readouts"]) != len(sc.readout_steps(WORLD_BY_ID[cid])):
                err = f"{cid} on rank {rank}: {o['fails'] or (o['comm'], o['fallback'], o['pick'], o['clip'])}"
        except Exception:
            import traceback

            err = f"{cid} on rank {rank}:\n{traceback.format_exc()}"
        if not sc._all_ranks(err is None):
            out["stopped"] = err or f"{cid}: a peer failed"
            return out
    return out


def evaluate_world_cell(cell: sc.Cell, res: dict) -> list[str]:
    """Failures of a cell of several ranks from ``res[rank]`` = :func:`run_world_cell`'s result."""
    fails, W = [], cell.world
    if sorted(res) != list(range(W)):
        return [f"{cell.id}: results of ranks {sorted(res)}, expected {W}"]
    steps = sc.readout_steps(cell)
    for r in range(W):
        o = res[r]
        fails += [f"{cell.id}: {m}" for m in o["fails"]]
        if o["comm"] != "xgmi" or o["fallback"] is not None:
            fails.append(f"{cell.id} rank {r}: comm {o['comm']!r} (fallback: {o['fallback']})")
        if tuple(o["pick"]) != cell.expect or not o["clip"]:
            fails.append(f"{cell.id} rank {r}: pick {tuple(o['pick'])}, clip_in_kernel {o['clip']}; expected {cell.expect}")
        if len(o["readouts"]) != len(steps):
            fails.append(f"{cell.id} rank {r}: {len(o['readouts'])} of {len(steps)} read-outs")
    if fails:
        return fails
    c = bounds(cell).c_bind
    for r in range(W):
        if res[r]["comm_after"] != "xgmi" or res[r]["fallback_after"] is not None:
            fails.append(f"{cell.id} rank {r}: comm {res[r]['comm_after']!r} after the steps")
    for k, t in enumerate(steps):
        ros = [ClipReadout(*res[r]["readouts"][k]) for r in range(W)]
        for r in range(W):
            fails += [f"rank {r}: {m}" for m in evaluate_readout(cell, ros[r], "bind", c)]
            for name in ("norm", "params", "m"):
                if not torch.equal(getattr(ros[r], name), getattr(ros[0], name)):
                    fails.append(f"{cell.id} t={t}: {name} of rank {r} differs from rank 0's")
    return fails

"""The fused step's gradient, read out exactly through the optimizer state, against fp64
autograd -- one cell per kernel instance the dispatcher of ``csrc/mlp_train.hip`` can pick from the
tables of ``csrc/mlp_train_one.hip`` and ``csrc/mlp_train_lanes.hip``.

Shared by ``tests/test_step_matrix_gpu.py``, ``tests/test_xgmi_matrix_gpu.py`` and
``tests/test_step_matrix_cpu.py``; CPU-only code except :func:`run_cell` and :func:`run_cell_rank`,
which drive a ``FusedTrainer`` on whatever device they are given.

**Read-out.**  ``adam_update`` forms ``m = fmaf(1 - b1, g - m, m)`` and ``sgd_update`` (momentum
!= 0, no weight decay) ``buf = g`` on the first step, ``fmaf(buf, mom, g)`` later
(``csrc/optim_core.h``).  With ``beta1 = 0`` / an all-zero moment both are ``g`` bit for bit, so
after zeroing ``tr.m`` and ``tr.v`` one ``train(1)`` leaves in ``tr.m[i]`` the gradient the step
formed for model i (``grad_scale`` is 1 on one rank).  Every launch reloads the moments from
``tr.m`` / ``tr.v`` in its prologue (``mlp_train_kernel``, ``mlp_train_lanes_kernel``: ``mr`` /
``vr``; the split-batch members all load them, the lead writes them back) through the pointers
the engine's argument block keeps, so zeroing the tensors in place between launches is seen by
the persistent engine.

**Metric.**  Per parameter tensor (each ``W_l``, ``b_l``) ``E = max|g - g64| / max|g64|``; for the
loss ``|l - l64| / |l64|``.  ``g64``: fp64 autograd at the snapshot parameters on
``tr.step_indices(t)``.

**fp32 bound.**  ``E <= max(4 Y, 8 * 2^-24)`` with ``Y`` the same metric of plain fp32 torch
autograd on the CPU for the same case: kernel and yardstick are fp32 evaluations of one
expression that differ in summation order and fma contraction over at most 512 terms.

**Cross-entropy margin** (:func:`ce_margin`).  The CE head calls the fast intrinsics:
``__expf(x)`` is ``v_exp_f32(x * log2(e))`` and ``__logf(x)`` is ``v_log_f32(x) * ln 2``, each
hardware op good to 1 ulp (the CDNA ISA's stated accuracy).  With ``u = 2^-24`` and
``x = h - max <= 0``:

* ``x`` itself carries ``u |x|`` from the subtraction, its product with ``log2(e)`` another
  ``u |x|`` (an absolute error of the exponent = a relative error of the result), the hardware
  exponential ``2 u``:  ``eps_exp(x) = (2 |x| + 2) u``.
* ``p_j = e_j / sum_i e_i``: ``eps_exp(x_j) + max_i eps_exp(x_i)`` plus ``8 u`` for the three
  additions, the reciprocal, the two products and the subtraction of the one-hot.
* So ``|delta dz_sj| <= p_sj delta_sj / bsz``, and with ``A = d out / d theta`` (fp64, exact)
  ``|delta g_k| <= sum_sj |A_sjk| p_sj delta_sj / bsz``.  The tensor's margin is the largest
  such bound over its elements over ``max|g64|``; it is ADDED to the fp32 bound.
* Loss: per sample ``eps_exp(max_i |x_i|) + 3 u`` (relative, on ``se``, hence absolute on
  ``log se``) ``+ 3 u |log se|`` (hardware log, its product with ln 2, the addition)
  ``+ u (|max| + |lse|)``; the mean over the batch over ``l64`` is the margin.

The margin is a function of the reference's own logits, never of the kernel's output.

**bf16 bound.**  The reference is ``mlp_forward_ref_bf16`` (the rounding model) in fp64; the
yardstick ``D`` is the metric between the rounding model's gradient and the fp32 model's, both
in fp64.  Required: ``max_t E_t <= max_t D_t / 2`` -- the kernel is nearer the bf16 recipe than
fp32 compute is -- and the read-out differs from the fp32 twin's.  (The rounding model keeps the
weight and bias gradients in fp32, as the kernels do; while it rounded them to bf16 these cells
stood at E = 2.4e-3 .. 3.8e-3 against D / 2 = 1.9e-3 .. 8e-3 and eight of them failed, and
against the mended model they stand at E = 6e-8 .. 7e-6.)

**Applied = stored.**  SGD: ``p1 = p0 - lr m`` (one fma: rtol 1e-6).  Adam: with ``v = 0`` before
the step, ``v1 = (1 - b2) m^2`` and ``dp = -lr m / (sqrt(v1 / bc2) + eps)``, ``bc2 = 1 - b2^(t+1)``;
asserted are the sign, ``|dp| <= lr c (1 + 1e-3)`` with ``c = sqrt(bc2 / (1 - b2))`` (1 at step 0,
where this is ``|dp| <= lr (1 + 1e-3)``; later steps of a freshly zeroed ``v`` are bias-corrected
by more than ``v`` holds) and the formula itself to rtol 1e-5.

**Several ranks** (``XGMI_CELLS``, ``tests/test_xgmi_matrix_gpu.py``).  Under
``DTP_MODE_XGMI_ADAM`` / ``_SGD`` every rank's step sums the W x members gradients in slot order
inside the kernel and the optimizer takes that sum times ``grad_scale = 1 / W``; every rank
zeroes its moments at the same step (:func:`step_gradient_world`), and the read-out is that
product -- the same bits on every rank, which is asserted.  Reference: the mean over the ranks
of fp64 autograd on each rank's ``step_indices(t)`` (loss: the mean of the ranks' mean losses);
``Y``: fp32 autograd per rank, summed in fp32 in rank order, times fp32 ``1 / W``; the CE margin
and the own margin are the means of the ranks' absolute margins (a bound of the mean's error),
``sum_chain`` counting the V slot additions.  Bounds and constants are those above.  The
conditions on the inputs are checked on the CPU along ``ref_train.torch_train``'s trajectory
(one geometry per rank; ``tests/test_step_matrix_cpu.py``); the seeds below were the first
tried for these cells and met them in every one, so no others were.  No cell of several ranks
needed ``own_margin``: the largest E / bound of the run kept in ``profiles/xgmi_matrix/`` is 0.49.
"""
from __future__ import annotations

import json
import math
import sys
from dataclasses import dataclass, replace
from typing import NamedTuple

import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream, SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.mlp import MlpSpec, mlp_forward_ref, mlp_forward_ref_bf16, unflatten
from distributed_training_pytorch_amd.ops.optim import OptimConfig

from .ref_train import loss_fn

U = 2.0 ** -24
SHAPES = {"T": MlpSpec(2, 10, 5, 1), "N3": MlpSpec(2, 10, 3, 1), "H15": MlpSpec(2, 15, 5, 1),
          "C4": MlpSpec(2, 10, 5, 4)}
ADAM = OptimConfig(lr=1e-2, betas=(0.0, 0.999))
SGD = OptimConfig("sgd", 5e-2, momentum=0.9)
N_MODELS = 2
STEPS_PER_LAUNCH = 3
# chosen so that the references alone meet the conditions on the inputs (check_conditions) in
# every cell: fp32 autograd's own error Y depends on the draw (other seeds reach 1e-5 .. 1e-3
# where a tensor's gradient nearly cancels over the batch)
DATA_SEED, INIT_SEED, SAMPLER_SEED = 21, 1, 5


# ------------------------------------------------------------------------------ the cells
@dataclass(frozen=True)
class Cell:
    shape: str                 # key of SHAPES
    opt: str                   # adam | sgd
    loss: str                  # mse | ce
    batch: int
    expect: tuple              # (lanes, waves, groups) the dispatcher must pick
    kind: str                  # fast | generic (one lane), lanes, grp
    groups: str = "off"        # EngineConfig.groups
    prec: str = "fp32"
    cache: bool = True         # EngineConfig.cache_data
    n: int = 512
    env: tuple = ()            # (("DTP_LANES", "2x8"),): a forced instance, run in a child process
    own_margin: bool = False   # the fp32 bound plus the running-error margin (fp32_margin)
    world: int = 1             # ranks (> 1: the xGMI modes, XGMI_CELLS below; all ranks share one GPU)

    @property
    def id(self) -> str:
        s = f"{self.shape}-{self.opt}-{self.loss}-{self.prec}-b{self.batch}-g{self.groups}"
        if self.world != 1:
            s = f"w{self.world}-" + s
        if not self.cache:
            s += "-nocache"
        if self.n != 512:
            s += f"-n{self.n}"
        for k, v in self.env:
            s += f"-{k}={v}"
        return s

    @property
    def spec(self) -> MlpSpec:
        return SHAPES[self.shape]

    @property
    def instance(self) -> tuple:
        """(shape, lanes, waves, loss, optimizer, precision, kind): the template instance."""
        return (self.shape, self.expect[0], self.expect[1], self.loss, self.opt, self.prec, self.kind)


def _one(shape, opt, loss, batch, kind, **kw):
    return Cell(shape, opt, loss, batch, (1, 4, 1), kind, **kw)


def _lanes(shape, opt, loss, batch, L, **kw):
    return Cell(shape, opt, loss, batch, (L, 4, 1), "lanes", **kw)


def _grp(shape, opt, loss, batch, members, **kw):
    return Cell(shape, opt, loss, batch, (4, 4, members), "grp", groups="on", **kw)


# The dispatcher is resolve_train() in csrc/mlp_train.hip.  A kernel instance added to
# DTP_ONE_SHAPES in csrc/mlp_train_one.hip (one lane: FAST or generic, per shape and precision)
# or to DTP_LANES_FAMILIES in csrc/mlp_train_lanes.hip (2 / 4 lanes, 4 or 8 waves; split-batch,
# the member count a constant at 4) needs a line in INSTANCES below and a cell here that runs it:
# tests/test_step_matrix_cpu.py::test_every_instance_has_a_cell compares the two.
CELLS = [
    # ---- one lane, groups="off".  FAST (Adam + MSE, cached data, batch <= 256)
    _one("T", "adam", "mse", 256, "fast"), _one("N3", "adam", "mse", 256, "fast"),
    _one("H15", "adam", "mse", 256, "fast"), _one("C4", "adam", "mse", 256, "fast"),
    _one("N3", "adam", "mse", 200, "fast"), _one("H15", "adam", "mse", 200, "fast"),  # last batch 112
    _one("C4", "adam", "mse", 200, "fast"),
    # generic Adam + MSE (cache_data=False: the data path reads global memory)
    _one("T", "adam", "mse", 256, "generic", cache=False), _one("N3", "adam", "mse", 256, "generic", cache=False),
    _one("H15", "adam", "mse", 256, "generic", cache=False), _one("C4", "adam", "mse", 200, "generic", cache=False),
    # SGD + MSE: lanes instances exist for the toy shape only, so N3 @64 and H15 @128 fall to one lane
    _one("N3", "sgd", "mse", 256, "generic"), _one("H15", "sgd", "mse", 200, "generic"),
    _one("C4", "sgd", "mse", 256, "generic"), _one("N3", "sgd", "mse", 64, "generic"),
    _one("H15", "sgd", "mse", 128, "generic"),
    # cross-entropy head
    _one("C4", "adam", "ce", 256, "generic"), _one("C4", "adam", "ce", 200, "generic"),
    _one("C4", "sgd", "ce", 256, "generic"),
    # chunked batches (> 256: the `for c0` loop of mlp_train_kernel; 300 = 256 + 44, last batch
    # 212; 513 of n = 1024: 256 + 256 + 1, last batch 511)
    _one("T", "adam", "mse", 300, "generic"), _one("T", "adam", "mse", 512, "generic"),
    _one("T", "adam", "mse", 513, "generic", n=1024), _one("T", "sgd", "mse", 300, "generic"),
    _one("C4", "adam", "ce", 300, "generic"), _one("H15", "adam", "mse", 300, "generic"),
    # bf16 (one lane at every batch for CE and SGD)
    _one("T", "adam", "mse", 256, "fast", prec="bf16"), _one("T", "adam", "mse", 200, "fast", prec="bf16"),
    _one("T", "adam", "mse", 300, "generic", prec="bf16"), _one("C4", "adam", "ce", 256, "generic", prec="bf16"),
    _one("T", "sgd", "mse", 256, "generic", prec="bf16"), _one("T", "sgd", "mse", 64, "generic", prec="bf16"),
    # the other instances of DTP_ONE_SHAPES' bf16 (2,10,5,4)
    _one("C4", "adam", "mse", 256, "fast", prec="bf16"), _one("C4", "adam", "mse", 200, "generic", prec="bf16", cache=False),
    _one("C4", "sgd", "mse", 200, "generic", prec="bf16"), _one("C4", "sgd", "ce", 256, "generic", prec="bf16"),
    # ---- two lanes (batch 65..128, groups="off")
    _lanes("T", "adam", "mse", 128, 2), _lanes("T", "adam", "mse", 100, 2),
    _lanes("T", "sgd", "mse", 128, 2, own_margin=True), _lanes("T", "sgd", "mse", 100, 2),
    _lanes("C4", "adam", "ce", 128, 2), _lanes("C4", "adam", "ce", 100, 2), _lanes("C4", "sgd", "ce", 128, 2),
    _lanes("T", "adam", "mse", 128, 2, prec="bf16"), _lanes("T", "adam", "mse", 100, 2, prec="bf16"),
    _lanes("N3", "adam", "mse", 100, 2), _lanes("H15", "adam", "mse", 100, 2), _lanes("C4", "adam", "mse", 100, 2),
    # ---- four lanes (batch <= 64)
    _lanes("T", "adam", "mse", 64, 4), _lanes("T", "adam", "mse", 50, 4),
    _lanes("T", "sgd", "mse", 50, 4, own_margin=True),
    _lanes("C4", "adam", "ce", 50, 4), _lanes("C4", "sgd", "ce", 64, 4), _lanes("T", "adam", "mse", 50, 4, prec="bf16"),
    _lanes("N3", "adam", "mse", 50, 4), _lanes("H15", "adam", "mse", 50, 4, own_margin=True),
    _lanes("C4", "adam", "mse", 50, 4),
    # ---- split-batch, groups="on": ceil(batch / 64) members of 64 samples
    _grp("T", "adam", "mse", 128, 2), _grp("T", "adam", "mse", 130, 3),  # the third member: 2 samples
    _grp("T", "adam", "mse", 256, 4),                                    # the constant-count instance
    _grp("T", "adam", "mse", 200, 4),                                    # last batch 112: a member left empty
    _grp("T", "sgd", "mse", 256, 4), _grp("T", "sgd", "mse", 130, 3),
    _grp("C4", "adam", "ce", 256, 4), _grp("C4", "adam", "ce", 130, 3),
    _grp("C4", "sgd", "ce", 128, 2), _grp("C4", "sgd", "ce", 256, 4),
    _grp("T", "adam", "mse", 256, 4, prec="bf16"), _grp("T", "adam", "mse", 130, 3, prec="bf16"),
    # batches above 256 never reach the split-batch step: fast_base_ok() (the FAST data path
    # every lanes / split-batch instance is built on) holds for min(batch, num_samples) <= 256
    # only, so groups="on" (and the policy) run the chunked one-lane kernel there.  The member
    # counts 5..8 that kGrpMax = 8 allows are unreachable on one rank; see docs/parity.md.
    Cell("T", "adam", "mse", 300, (1, 4, 1), "generic", groups="on"),
    Cell("T", "adam", "mse", 512, (1, 4, 1), "generic", groups="on"),
]

# forced instances: the environment is read once per process, so one child process per value
FORCED = [
    Cell("T", "adam", "mse", 256, (2, 8, 1), "lanes", groups="auto", env=(("DTP_LANES", "2x8"),)),
    Cell("T", "adam", "mse", 200, (2, 8, 1), "lanes", groups="auto", env=(("DTP_LANES", "2x8"),)),
    Cell("T", "adam", "mse", 128, (4, 8, 1), "lanes", groups="auto", env=(("DTP_LANES", "4x8"),)),
    Cell("T", "adam", "mse", 64, (1, 4, 1), "fast", groups="auto", env=(("DTP_LANES", "1"),)),
    Cell("H15", "adam", "mse", 64, (1, 4, 1), "fast", groups="auto", env=(("DTP_LANES", "1"),)),
    Cell("T", "adam", "mse", 256, (1, 4, 1), "generic", env=(("DTP_FAST", "0"),)),
    Cell("N3", "adam", "mse", 256, (1, 4, 1), "generic", env=(("DTP_FAST", "0"),)),
    Cell("T", "adam", "mse", 256, (4, 8, 2), "grp", groups="on", env=(("DTP_GRP_NW", "8"),)),
    Cell("T", "adam", "mse", 200, (4, 8, 2), "grp", groups="on", env=(("DTP_GRP_NW", "8"),)),
]

ALL_CELLS = CELLS + FORCED


# ---- the xGMI modes: W ranks, every rank's step summed inside the kernel through one of the
# exchanges of csrc/xgmi_core.h.  xgmi_allreduce_slots (2-float granules, a pending-mask bit
# r (GPT + 1) + k per slot r and granule k of a thread): the one-lane kernels and the 8-wave
# lanes instances.  xgmi_allreduce_g3 (3-float granules staged in LDS): the 4-wave lanes and
# split-batch instances, over V = W x members slots; its poll loop is one of four bodies picked
# by pi = ceil((V - 1) NG / 256), NG = ceil((P + 1) / 3) = 124 (T), 135 (C4), 261 (H15), 101 (N3):
# PI = 1, 2, min(4, MAXI), MAXI = ceil(7 NG / 256); its publish deals destination rank di to wave
# di % 4 (D = W - 1 destinations, W with members), so a wave takes a second one from W = 6.
# n = 512 over W ranks: 256 / 171 / 103 / 64 samples per rank, the list padded to 513 (W = 3) and
# 515 (W = 5) so that the last ranks' shares wrap to the head of the permutation.
def _w(world, *cells):
    return [replace(c, world=world) for c in cells]


XGMI_CELLS = (
    # ---- W = 2, one lane (batch 200 of 256 per rank; last batch 56): slots, V = 2
    _w(2, _one("T", "adam", "mse", 200, "fast"), _one("N3", "adam", "mse", 200, "fast"),      # NPT 2, 1
       _one("H15", "adam", "mse", 200, "fast"), _one("C4", "adam", "mse", 200, "fast"),      # NPT 4, 2
       _one("T", "sgd", "mse", 200, "generic"), _one("C4", "adam", "ce", 200, "generic"),
       _one("C4", "sgd", "ce", 200, "generic"), _one("T", "adam", "mse", 200, "fast", prec="bf16"),
       # the remaining one-lane instances of the two xGMI modes (XGMI_INSTANCES)
       _one("T", "adam", "mse", 200, "generic", cache=False), _one("N3", "adam", "mse", 200, "generic", cache=False),
       _one("H15", "adam", "mse", 200, "generic", cache=False), _one("C4", "adam", "mse", 200, "generic", cache=False),
       _one("H15", "sgd", "mse", 200, "generic"), _one("C4", "sgd", "mse", 200, "generic"),
       _one("T", "adam", "mse", 200, "generic", prec="bf16", cache=False), _one("T", "sgd", "mse", 200, "generic", prec="bf16"),
       _one("C4", "adam", "mse", 200, "fast", prec="bf16"), _one("C4", "adam", "mse", 200, "generic", prec="bf16", cache=False),
       _one("C4", "sgd", "mse", 200, "generic", prec="bf16"), _one("C4", "adam", "ce", 200, "generic", prec="bf16"),
       _one("C4", "sgd", "ce", 200, "generic", prec="bf16"),
       # split-batch: V = 2 x members slots of g3
       _grp("T", "adam", "mse", 256, 4),                                    # V = 8, pi = 4
       _grp("T", "sgd", "mse", 130, 3),                                     # V = 6, the third member: 2 samples
       _grp("C4", "adam", "ce", 128, 2), _grp("C4", "sgd", "ce", 128, 2),   # V = 4, pi = 2
       _grp("T", "adam", "mse", 256, 4, prec="bf16"))
    # ---- W = 3 (171 per rank): 2 lanes at batch 100 (last batch 71), g3 with V = 3
    + _w(3, _lanes("T", "adam", "mse", 100, 2), _lanes("T", "sgd", "mse", 100, 2), _lanes("C4", "sgd", "ce", 100, 2),
         _lanes("H15", "adam", "mse", 100, 2),                               # pi = 3: the PI = 4 body
         _lanes("N3", "adam", "mse", 100, 2), _lanes("C4", "adam", "mse", 100, 2), _lanes("C4", "adam", "ce", 100, 2),
         _lanes("T", "adam", "mse", 100, 2, prec="bf16"),
         _grp("T", "adam", "mse", 128, 2),                                   # V = 6, pi = 3; last batch 43: a member empty
         _one("N3", "sgd", "mse", 171, "generic"))                           # no N3 SGD lanes instance: slots, NPT 1
    # ---- W = 5 (103 per rank)
    + _w(5, _lanes("H15", "adam", "mse", 70, 2),                             # pi = 5: the MAXI = 8 body
         _lanes("T", "adam", "mse", 50, 4), _lanes("C4", "adam", "ce", 50, 4), _lanes("T", "adam", "mse", 50, 4, prec="bf16"),
         _lanes("N3", "adam", "mse", 50, 4))
    # ---- W = 8 (64 per rank): 4 lanes at batch 50 (last batch 14); publish round two (D = 7)
    + _w(8, _lanes("T", "adam", "mse", 50, 4),                               # pi = 4
         _lanes("H15", "adam", "mse", 50, 4),                                # pi = 8
         _lanes("C4", "adam", "mse", 50, 4), _lanes("C4", "sgd", "ce", 50, 4), _lanes("T", "sgd", "mse", 50, 4),
         _lanes("T", "adam", "mse", 50, 4, prec="bf16"), _lanes("N3", "adam", "mse", 50, 4),
         # one lane at n = 2048 (256 per rank; above kLaneData, so neither lanes nor split-batch): slots r <= 7
         _one("T", "adam", "mse", 256, "fast", n=2048), _one("H15", "adam", "mse", 200, "fast", n=2048),  # NPT 4, GPT 2
         _one("T", "sgd", "mse", 200, "generic", n=2048))
)
# forced 8-wave lanes instances (slots at 512 threads): one spawn per value
XGMI_FORCED = _w(2, Cell("T", "adam", "mse", 128, (4, 8, 1), "lanes", groups="auto", env=(("DTP_LANES", "4x8"),)),
                 Cell("T", "adam", "mse", 256, (2, 8, 1), "lanes", groups="auto", env=(("DTP_LANES", "2x8"),)))
ALL_XGMI = XGMI_CELLS + XGMI_FORCED
# the W = 8 check of launch="graph" against launch="persistent" (tests/test_xgmi_matrix_gpu.py)
XGMI_GRAPH_CELL = XGMI_CELLS[[c.id for c in XGMI_CELLS].index("w8-T-adam-mse-fp32-b50-goff")]

BY_ID = {c.id: c for c in ALL_CELLS + ALL_XGMI}
assert len(BY_ID) == len(ALL_CELLS) + len(ALL_XGMI), "duplicate cell ids"


def _xgmi_instances():
    """What the tables (DTP_ONE_SHAPES, DTP_LANES_FAMILIES) instantiate for DTP_MODE_XGMI_ADAM
    and DTP_MODE_XGMI_SGD, in the form of :func:`_instances` -- written out from the tables,
    NOT derived from XGMI_CELLS."""
    out = []
    # one_row(): XGMI_ADAM FAST, XGMI_ADAM, XGMI_SGD
    for prec, shapes in (("fp32", ("T", "N3", "C4", "H15")), ("bf16", ("T", "C4"))):
        for s in shapes:
            out += [(s, 1, 4, "mse", "adam", prec, "fast"), (s, 1, 4, "mse", "adam", prec, "generic"),
                    (s, 1, 4, "mse", "sgd", prec, "generic")]
            if s == "C4":
                out += [(s, 1, 4, "ce", "adam", prec, "generic"), (s, 1, 4, "ce", "sgd", prec, "generic")]
    # lanes_fill() / lanes_row(): every lanes instance has its xGMI twin
    for L in (2, 4):
        out += [(s, L, 4, "mse", "adam", "fp32", "lanes") for s in ("T", "N3", "C4", "H15")]
        out += [("T", L, 4, "mse", "sgd", "fp32", "lanes"), ("C4", L, 4, "ce", "adam", "fp32", "lanes"),
                ("C4", L, 4, "ce", "sgd", "fp32", "lanes"), ("T", L, 4, "mse", "adam", "bf16", "lanes"),
                ("T", L, 8, "mse", "adam", "fp32", "lanes")]
    # LanesInst.grp[2]: one instance per family (the member count is read at run time); DTP_GRP_NW=8 is
    # one-rank only
    out += [("T", 4, 4, "mse", "adam", "fp32", "grp"), ("T", 4, 4, "mse", "sgd", "fp32", "grp"),
            ("T", 4, 4, "mse", "adam", "bf16", "grp"), ("C4", 4, 4, "ce", "adam", "fp32", "grp"),
            ("C4", 4, 4, "ce", "sgd", "fp32", "grp")]
    return out


XGMI_INSTANCES = _xgmi_instances()


def _instances():
    """What the tables (DTP_ONE_SHAPES, DTP_LANES_FAMILIES) instantiate for the local optimizer
    modes, as (shape, lanes, waves, loss, optimizer, precision, kind) -- written out from the
    tables, NOT derived from CELLS.  (The xGMI modes: XGMI_INSTANCES; MODE_GRAD: other tests.)"""
    out = []
    # DTP_ONE_SHAPES: four shapes in fp32, two of them in bf16 too;
    # FAST = Adam + MSE; the generic kernel takes the loss at run time (CE: the 4-class head)
    for prec, shapes in (("fp32", ("T", "N3", "C4", "H15")), ("bf16", ("T", "C4"))):
        for s in shapes:
            out += [(s, 1, 4, "mse", "adam", prec, "fast"), (s, 1, 4, "mse", "adam", prec, "generic"),
                    (s, 1, 4, "mse", "sgd", prec, "generic")]
            if s == "C4":
                out += [(s, 1, 4, "ce", "adam", prec, "generic"), (s, 1, 4, "ce", "sgd", prec, "generic")]
    # DTP_LANES_FAMILIES: Adam + MSE for every shape; SGD + MSE toy; the CE head with Adam and SGD;
    # bf16 toy Adam + MSE; 8 waves: toy fp32 Adam + MSE
    for L in (2, 4):
        out += [(s, L, 4, "mse", "adam", "fp32", "lanes") for s in ("T", "N3", "C4", "H15")]
        out += [("T", L, 4, "mse", "sgd", "fp32", "lanes"), ("C4", L, 4, "ce", "adam", "fp32", "lanes"),
                ("C4", L, 4, "ce", "sgd", "fp32", "lanes"), ("T", L, 4, "mse", "adam", "bf16", "lanes"),
                ("T", L, 8, "mse", "adam", "fp32", "lanes")]
    # the split-batch families: toy fp32 Adam / SGD, toy bf16 Adam, the CE head Adam / SGD (each
    # with the run-time and the constant member count, LanesInst.grp[0..1]); DTP_GRP_NW=8: toy Adam
    out += [("T", 4, 4, "mse", "adam", "fp32", "grp"), ("T", 4, 4, "mse", "sgd", "fp32", "grp"),
            ("T", 4, 4, "mse", "adam", "bf16", "grp"), ("C4", 4, 4, "ce", "adam", "fp32", "grp"),
            ("C4", 4, 4, "ce", "sgd", "fp32", "grp"), ("T", 4, 8, "mse", "adam", "fp32", "grp")]
    return out


INSTANCES = _instances()
# the split-batch families whose 4-member instance is a separate template (LanesInst.grp[1])
GRP_CONST_FAMILIES = [("T", "mse", "adam", "fp32"), ("T", "mse", "sgd", "fp32"), ("T", "mse", "adam", "bf16"),
                      ("C4", "ce", "adam", "fp32"), ("C4", "ce", "sgd", "fp32")]


# ------------------------------------------------------------------------------ inputs
def cell_data(cell: Cell):
    """(X [n, 2], Y) on the CPU: the toy regression set; class ids for CE; for the 4-output
    MSE head four targets per sample (the toy target, scaled, negated, and the input)."""
    ds = ToyData(n=cell.n, seed=DATA_SEED, classes=4 if cell.loss == "ce" else 0)
    X, Y = ds.X, ds.Y
    if cell.loss == "mse" and cell.spec.out_features == 4:
        Y = torch.cat([Y, 0.5 * Y, -Y, X[:, :1]], 1).contiguous()
    return X, Y


def cell_init(cell: Cell):
    g = torch.Generator().manual_seed(INIT_SEED)
    return [torch.randn(cell.spec.P, generator=g) * 0.4 for _ in range(N_MODELS)]


def cell_geom(cell: Cell, rank: int = 0) -> SamplerGeometry:
    return SamplerGeometry(n=cell.n, world=cell.world, rank=rank, batch=cell.batch, seed=SAMPLER_SEED)


def cell_indices(cell: Cell, t: int) -> list[list[int]]:
    """Every rank's batch of step t, in rank order (the engine's default order: torch's
    DistributedSampler, the permutation padded by repeating from its start)."""
    return [EpochIndexStream(cell_geom(cell, r)).indices(t) for r in range(cell.world)]


def readout_steps(cell: Cell) -> list[int]:
    """Step 0, the last step of epoch 0 (the short batch where there is one), the first of epoch 1."""
    spe = cell_geom(cell).steps_per_epoch
    return sorted({0, spe - 1, spe})


def make_trainer(cell: Cell, device, prec: str | None = None, rank: int = 0, **cfg) -> FusedTrainer:
    X, Y = cell_data(cell)
    ecfg = EngineConfig(**{"steps_per_launch": STEPS_PER_LAUNCH, "loss": cell.loss, "groups": cell.groups,
                           "cache_data": cell.cache, "precision": prec or cell.prec, **cfg})
    return FusedTrainer(cell.spec, N_MODELS, X.to(device), Y.to(device), cell_geom(cell, rank),
                        ADAM if cell.opt == "adam" else SGD, ecfg, init_params=[p.to(device) for p in cell_init(cell)])


# ------------------------------------------------------------------------------ read-out
class StepGradient(NamedTuple):
    t: int
    params_before: torch.Tensor  # [n_models, P], CPU
    grad: torch.Tensor           # the step's gradient as the optimizer took it
    loss: torch.Tensor           # [n_models], the step's logged loss
    params_after: torch.Tensor


def step_gradient(tr: FusedTrainer) -> StepGradient:
    """Run step ``tr.t`` with zeroed moments and return the gradient it formed (module docstring)."""
    o = tr.optim
    assert (o.name == "adam" and o.betas[0] == 0.0) or (o.name == "sgd" and o.momentum != 0.0), o
    assert o.weight_decay == 0.0 and not o.clips and tr.world == 1
    tr.synchronize()
    p0 = tr.params.detach().cpu().clone()
    tr.m.zero_()
    tr.v.zero_()
    t = tr.t
    tr.train(1)
    tr.synchronize()
    assert tr.t == t + 1
    return StepGradient(t, p0, tr.m.detach().cpu().clone(), tr.losses(t, t + 1)[0].clone(),
                        tr.params.detach().cpu().clone())


def step_gradient_world(tr: FusedTrainer) -> StepGradient:
    """:func:`step_gradient` on every rank of a W-rank engine at the same step.  Under the
    xGMI modes the optimizer takes the slot-order fp32 sum of the members' gradients times
    ``grad_scale = 1 / W`` (the kernels' ``g[k] * a.hp.grad_scale``), so with zeroed
    moments ``tr.m[i]`` is that product bit for bit -- the same bits on every rank.  Every rank
    calls this at the same ``tr.t``; a process-group barrier lets the ranks enter the launch
    together (the exchange's wait is bounded by ``xgmi_timeout_us``)."""
    import torch.distributed as dist

    o = tr.optim
    assert (o.name == "adam" and o.betas[0] == 0.0) or (o.name == "sgd" and o.momentum != 0.0), o
    assert o.weight_decay == 0.0 and not o.clips and tr.comm == "xgmi"
    tr.synchronize()
    p0 = tr.params.detach().cpu().clone()
    tr.m.zero_()
    tr.v.zero_()
    t = tr.t
    dist.barrier()
    tr.train(1)
    tr.synchronize()
    assert tr.t == t + 1
    return StepGradient(t, p0, tr.m.detach().cpu().clone(), tr.losses(t, t + 1)[0].clone(),
                        tr.params.detach().cpu().clone())


# ------------------------------------------------------------------------------ references
def autograd_gradient(spec, p, x, y, loss: str, dtype, forward=mlp_forward_ref):
    """(gradient [P], loss) of one model by plain autograd in ``dtype`` on the CPU."""
    q = p.detach().to(dtype).clone().requires_grad_(True)
    tgt = y if loss == "ce" else y.to(dtype)
    lo = loss_fn(forward(q, spec, x.to(dtype)), tgt, loss)
    (g,) = torch.autograd.grad(lo, q)
    return g.detach(), lo.detach()


def tensor_names(spec) -> list[str]:
    return [f"{'W' if k % 2 == 0 else 'b'}{k // 2}" for k in range(2 * spec.n_layers)]


def metric(spec, g, g64) -> dict:
    """E per parameter tensor: max|g - g64| / max|g64|."""
    a, b = unflatten(g.double(), spec), unflatten(g64.double(), spec)
    return {n: ((x - y).abs().max() / y.abs().max()).item() for n, x, y in zip(tensor_names(spec), a, b)}


def rel(a, b) -> float:
    return abs(float(a) - float(b)) / abs(float(b))


def per_tensor(spec, bound, g64) -> dict:
    """An absolute per-element bound [P] as the metric's: its largest element over max|g64|, per tensor."""
    return {n: (b.max() / r.abs().max()).item()
            for n, b, r in zip(tensor_names(spec), unflatten(bound, spec), unflatten(g64, spec))}


def ce_margin(spec, p, x, y, g64) -> tuple[dict, float]:
    """The cross-entropy cells' margin (module docstring): per tensor, and for the loss."""
    bound, lbound = ce_margin_abs(spec, p, x, y)
    l64 = torch.nn.functional.cross_entropy(mlp_forward_ref(p.double(), spec, x.double()), y.view(-1).long())
    return per_tensor(spec, bound, g64), (lbound / l64.abs()).item()


def ce_margin_abs(spec, p, x, y) -> tuple[torch.Tensor, torch.Tensor]:
    """:func:`ce_margin` as absolute bounds: per gradient element [P], and of the loss.  (Several
    ranks: the mean of the ranks' bounds bounds the mean of their gradients.)"""
    p64, x64 = p.double(), x.double()
    out = mlp_forward_ref(p64, spec, x64)                            # [B, C]
    A = torch.func.jacrev(lambda q: mlp_forward_ref(q, spec, x64))(p64)  # [B, C, P]
    B = out.shape[0]
    mx = out.max(1, keepdim=True).values
    xs = (out - mx).abs()
    eps = (2 * xs + 2) * U
    delta = eps + eps.max(1, keepdim=True).values + 8 * U
    prob = torch.softmax(out, 1)
    bound = torch.einsum("sjk,sj->k", A.abs(), prob * delta) / B
    lse = torch.logsumexp(out, 1)
    logse = (lse - mx.view(-1)).abs()
    per = eps.max(1).values + 3 * U + 3 * U * logse + U * (mx.view(-1).abs() + lse.abs())
    return bound, per.mean()


def sum_chain(cell: Cell, bsz: int) -> int:
    """Longest chain of fp32 additions behind one dW element (an upper bound read from the
    kernels): a wave accumulates its samples' products on MFMA -- 64 / L samples per wave and
    256-sample chunk (``bk = gk (NW G) + wave G + ws`` with ``G = 64 / L`` in
    ``mlp_train_lanes_kernel``; one lane: ``c0 + tid`` over the chunks of ``mlp_train_kernel``)
    -- then the waves' tiles are summed, then the members', plus the two merges of the split
    accumulators (``a0 += a1``, ``wave_outer_acc``).  Several ranks: the members' sum is the
    exchange's, over its V = world x members slots."""
    lanes, waves, groups = cell.expect
    chunks = -(-bsz // 256) if lanes == 1 else 1
    return (64 // lanes) * chunks + waves + cell.world * groups + 2


LAMBDA = 6.0  # |sum c_i d_i| <= LAMBDA u sqrt(sum c_i^2) fails with probability <= 2 exp(-LAMBDA^2 / 2) = 3e-8


def fp32_margin(spec, p, x, y, n_sum: int) -> dict:
    """Error model of an fp32 evaluation of the MSE step's gradient, per tensor over
    ``max|g64|`` -- the own margin of the cells marked ``own_margin``.

    The standard model of rounding (every fp32 operation returns its exact result times
    ``1 + d``, ``|d| <= u = 2^-24``), to first order, with the ``d`` independent and of mean
    zero (Higham & Mary 2019): the error of gradient element k is ``sum_r c_kr d_r`` over the
    roundings r of the step, and ``|error_k| <= LAMBDA u sqrt(sum_r c_kr^2)`` but for a
    probability of 2 exp(-LAMBDA^2 / 2).  The ``c_kr`` are exact: the step is written out below
    with a perturbation at every rounding site, scaled by the magnitude it rounds, and
    differentiated (``torch.func.jacrev``) -- so a rounding of layer 1's pre-activation reaches
    W0's gradient through the true backward chain, cancellation over the batch included.  A dot
    product of k terms is one site of scale ``sqrt(k) u sum|terms|`` (k fma roundings of partial
    sums, each at most ``sum|terms|``).  Sites, as in ``mlp_lanes.h`` / ``mlp_core.h``:

    * forward  ``z = W h + b`` (k = I + 1), LeakyReLU ``max(z, slope z)`` (one product);
    * loss     ``dz = 2 (out - y) inv``: the subtraction, the product, ``inv`` itself;
    * backward ``dh = W^T dz`` (k = O), times the activation's slope;
    * ``dW = sum_s dz_s h_s^T`` (the bias: ``h = 1``): k = ``n_sum`` (:func:`sum_chain`).

    Where a tensor's gradient nearly cancels over the batch the model grows with the
    cancellation, as any fp32 evaluation's error does -- and there fp32 autograd's own error
    ``Y``, a single draw of this distribution, says little (seen down to 2e-9, a hundredth of
    ``u``, beside kernel errors of 13 u).  Not modelled: a pre-activation within its error of 0."""
    g64, _ = autograd_gradient(spec, p, x, y, "mse", torch.float64)
    return per_tensor(spec, fp32_margin_abs(spec, p, x, y, n_sum), g64)


def fp32_margin_abs(spec, p, x, y, n_sum: int) -> torch.Tensor:
    """:func:`fp32_margin` as an absolute bound per gradient element [P].  (Several ranks: the
    mean of the ranks' bounds bounds the mean of their gradients.)"""
    ps = [t.double() for t in unflatten(p.double(), spec)]
    NL, B = spec.n_layers, x.shape[0]
    x64, y64 = x.double(), y.double()
    inv = 1.0 / (B * spec.out_features)
    dims = spec.dims()
    # perturbation sites: z_l, h_l (forward), dz_out, then dh_l, dz_{l-1} (backward)
    sizes = [B * o for _, o in dims] + [B * o for l, (_, o) in enumerate(dims) if spec.act(l)] + [B * spec.out_features]
    sizes += [B * i for l, (i, _) in enumerate(dims) if l > 0] * 2
    final = {}

    def step(eps):
        off = [0]

        def site(val, scale):
            n = val.numel()
            e = eps[off[0]:off[0] + n].view(val.shape)
            off[0] += n
            return val + e * scale.detach()

        h, hs, ds = x64, [], []
        for l in range(NL):
            W, b = ps[2 * l], ps[2 * l + 1]
            hs.append(h)
            z = site(h @ W.T + b, math.sqrt(W.shape[1] + 1) * U * (h.abs() @ W.abs().T + b.abs()))
            if spec.act(l):
                d = torch.where(z.detach() > 0, one, one * spec.slope)
                h = z * d
                h = site(h, U * h.abs())
            else:
                d, h = torch.ones_like(z), z
            ds.append(d)
        dz = 2 * (h - y64.view_as(h)) * inv
        dz = site(dz, math.sqrt(3.0) * U * dz.abs())
        out = [None] * (2 * NL)
        for l in reversed(range(NL)):
            W = ps[2 * l]
            out[2 * l], out[2 * l + 1] = dz.T @ hs[l], dz.sum(0)
            final[2 * l] = math.sqrt(n_sum) * U * (dz.abs().T @ hs[l].abs()).detach()
            final[2 * l + 1] = math.sqrt(n_sum) * U * dz.abs().sum(0).detach()
            if l > 0:
                dh = site(dz @ W, math.sqrt(W.shape[0]) * U * (dz.abs() @ W.abs()))
                dz = dh * ds[l - 1]
                dz = site(dz, U * dz.abs())
        assert off[0] == eps.numel()
        return torch.cat([t.reshape(-1) for t in out])

    one = torch.ones((), dtype=torch.float64)
    eps0 = torch.zeros(sum(sizes), dtype=torch.float64)
    J = torch.func.jacrev(step)(eps0)                       # [P, sites]
    var = (J * J).sum(1) + torch.cat([final[k].reshape(-1) for k in range(2 * NL)]) ** 2
    g0 = step(eps0)
    g64, _ = autograd_gradient(spec, p, x, y, "mse", torch.float64)
    assert (g0 - g64).abs().max() <= 1e-12 * g64.abs().max(), "the written-out step is not the step"
    return LAMBDA * var.sqrt()


def evaluate_step(cell: Cell, sg: StepGradient, indices: list[int], X, Y,
                  n_models: int = N_MODELS) -> tuple[list[dict], list[str]]:
    """Records (one per model, ``n_models`` of them) and failures of one read-out against the references.

    A cell of several ranks (``cell.world > 1``) takes one index list per rank, in rank order
    (:func:`cell_indices`): the reference is the mean over the ranks of fp64 autograd on each
    rank's batch (the loss: of the ranks' mean losses), the yardstick ``Y`` fp32 autograd per
    rank summed in fp32 in rank order and multiplied by fp32 ``1 / W``, and a margin the mean of
    the ranks' absolute margins -- a bound of the mean's error."""
    spec, recs, fails = cell.spec, [], []
    per_rank = indices if cell.world > 1 else [indices]
    assert len(per_rank) == cell.world and all(len(ix) > 0 for ix in per_rank)
    W = len(per_rank)
    batches = [(X[torch.tensor(ix, dtype=torch.long)], Y[torch.tensor(ix, dtype=torch.long)]) for ix in per_rank]
    sizes = [len(ix) for ix in per_rank]
    bf = cell.prec == "bf16"

    def mean(dtype, forward=mlp_forward_ref):
        g, lo = None, None
        for x, y in batches:  # rank order
            gr, lr = autograd_gradient(spec, p, x, y, cell.loss, dtype, forward)
            g, lo = (gr, lr) if g is None else (g + gr, lo + lr)
        if W > 1:
            inv = torch.tensor(1.0 / W, dtype=dtype)
            g, lo = g * inv, lo * inv
        return g, lo

    for i in range(n_models):
        p = sg.params_before[i]
        g64, l64 = mean(torch.float64)
        g32, l32 = mean(torch.float32)
        Yt, Yl = metric(spec, g32, g64), rel(l32, l64)
        rec = {"cell": cell.id, "t": sg.t, "model": i, "bsz": sizes[0] if W == 1 else sizes, "Y": Yt, "Y_loss": Yl}
        big = max(t.abs().max().item() for t in unflatten(g64, spec))
        rec["min_tensor_max"] = min(t.abs().max().item() for t in unflatten(g64, spec)) / big
        if bf:
            gb, lb = mean(torch.float64, mlp_forward_ref_bf16)
            rec["D"], rec["D_loss"] = metric(spec, gb, g64), rel(lb, l64)
            ref_g, ref_l = gb, lb
        else:
            ref_g, ref_l = g64, l64
            bound = {n: max(4 * v, 8 * U) for n, v in Yt.items()}
            lbound = max(4 * Yl, 8 * U)
            if cell.loss == "ce":
                ab = [ce_margin_abs(spec, p, x, y) for x, y in batches]
                mt = per_tensor(spec, sum(b for b, _ in ab) / W, g64)
                ml = (sum(m for _, m in ab) / W / l64.abs()).item()
                rec["margin"], rec["margin_loss"] = mt, ml
                bound = {n: bound[n] + mt[n] for n in bound}
                lbound += ml
            if cell.own_margin:
                assert cell.loss == "mse"
                mt = per_tensor(spec, sum(fp32_margin_abs(spec, p, x, y, sum_chain(cell, max(sizes)))
                                          for x, y in batches) / W, g64)
                rec["margin"] = mt
                bound = {n: bound[n] + mt[n] for n in bound}
            rec["bound"], rec["bound_loss"] = bound, lbound
        if sg.grad is not None:
            E, El = metric(spec, sg.grad[i], ref_g), rel(sg.loss[i], ref_l)
            rec["E"], rec["E_loss"] = E, El
            rec["ratio"] = {n: E[n] / max(Yt[n], 2 * U) for n in E}  # E / Y (Y floored at the 8u / 4 of the bound)
            rec["ratio_loss"] = El / max(Yl, 2 * U)
            if not bf:
                for n in E:
                    if not E[n] <= rec["bound"][n]:
                        fails.append(f"{cell.id} t={sg.t} model {i} {n}: E {E[n]:.3e} > bound {rec['bound'][n]:.3e} "
                                     f"(Y {Yt[n]:.3e}, E/Y {E[n] / Yt[n]:.2f})")
                if not El <= rec["bound_loss"]:
                    fails.append(f"{cell.id} t={sg.t} model {i} loss: E {El:.3e} > bound {rec['bound_loss']:.3e}")
            fails += [f"{cell.id} t={sg.t} model {i}: {m}" for m in applied_is_stored(cell, sg, i)]
        recs.append(rec)
    return recs, fails


def applied_is_stored(cell: Cell, sg: StepGradient, i: int) -> list[str]:
    """The parameter change of the step agrees with the gradient read out (module docstring)."""
    p0, p1, m = sg.params_before[i].double(), sg.params_after[i].double(), sg.grad[i].double()
    out = []
    if cell.opt == "sgd":
        pred = p0 - SGD.lr * m
        bad = (p1 - pred).abs() > 1e-6 * pred.abs() + 1e-7 * SGD.lr * m.abs()
        if bad.any():
            out.append(f"SGD: p1 != p0 - lr m at {int(bad.sum())} elements")
        return out
    lr, b2, eps = ADAM.lr, ADAM.betas[1], ADAM.eps
    bc2 = 1.0 - b2 ** (sg.t + 1)
    dp = p1 - p0
    pred = -lr * m / ((1.0 - b2) ** 0.5 * m.abs() / bc2 ** 0.5 + eps)
    live = m.abs() > 1e-6
    if (torch.sign(dp[live]) != -torch.sign(m[live])).any():
        out.append("Adam: a parameter moved along its gradient")
    cap = lr * math.sqrt(bc2 / (1.0 - b2)) * (1 + 1e-3)
    if (dp.abs() > cap + 2 * U * p0.abs()).any():
        out.append(f"Adam: |dp| {dp.abs().max().item():.3e} > {cap:.3e}")
    bad = (dp - pred).abs() > 1e-5 * pred.abs() + 4 * U * torch.maximum(p0.abs(), p1.abs())
    if bad.any():
        out.append(f"Adam: dp is not the step of the gradient read out at {int(bad.sum())} elements")
    return out


def check_bf16(cell: Cell, recs: list[dict]) -> list[str]:
    """max_t E_t <= max_t D_t / 2 per read-out (and the loss by the same yardstick)."""
    fails = []
    for r in recs:
        if "E" not in r:
            continue
        e, d = max(r["E"].values()), max(r["D"].values())
        r["bound_bf16"] = d / 2
        if not e <= d / 2:
            fails.append(f"{cell.id} t={r['t']} model {r['model']}: max E {e:.3e} > max D / 2 = {d / 2:.3e}")
        if not r["E_loss"] <= d / 2:
            fails.append(f"{cell.id} t={r['t']} model {r['model']} loss: E {r['E_loss']:.3e} > max D / 2 = {d / 2:.3e}")
    return fails


def check_conditions(cell: Cell, recs: list[dict]) -> list[str]:
    """The conditions on the inputs: no tensor's gradient negligible, a small yardstick, and for
    bf16 a rounding model clearly apart from fp32 compute."""
    fails = []
    for r in recs:
        tag = f"{cell.id} t={r['t']} model {r['model']}"
        if not r["min_tensor_max"] >= 1e-4:
            fails.append(f"{tag}: a tensor's max|g64| is {r['min_tensor_max']:.2e} of the gradient's")
        ymax = max(max(r["Y"].values()), r["Y_loss"])
        if not ymax <= 2e-6:
            fails.append(f"{tag}: Y {ymax:.2e} > 2e-6")
        if cell.prec == "bf16" and not max(r["D"].values()) >= 100 * max(r["Y"].values()):
            fails.append(f"{tag}: max D {max(r['D'].values()):.2e} < 100 Y")
    return fails


# ------------------------------------------------------------------------------ a cell
def run_cell(cell: Cell, device, expect_instance: bool = True) -> tuple[list[dict], list[str]]:
    """The cell's read-outs on ``device`` against the references: (records, failures)."""
    X, Y = cell_data(cell)
    tr = make_trainer(cell, device)
    recs, fails = [], []
    try:
        inst = [tr.lanes, tr.kernel_waves, tr.groups]
        if expect_instance and tuple(inst) != cell.expect:
            return [], [f"{cell.id}: the dispatcher picked (lanes, waves, groups) = {tuple(inst)}, expected {cell.expect}"]
        for t in readout_steps(cell):
            if tr.t < t:
                tr.train(t - tr.t)
            sg = step_gradient(tr)
            assert sg.t == t
            r, f = evaluate_step(cell, sg, tr.step_indices(t), X, Y)
            for x in r:
                x["instance"] = inst
            if t == 0 and cell.prec == "bf16" and device.type == "cuda":
                tw = make_trainer(cell, device, prec="fp32")
                try:
                    g32 = step_gradient(tw).grad
                finally:
                    tw.close()
                for i, x in enumerate(r):
                    x["vs_fp32_twin"] = max(metric(cell.spec, sg.grad[i], g32[i]).values())
                    if torch.equal(sg.grad[i], g32[i]):
                        f.append(f"{cell.id} model {i}: the bf16 read-out equals the fp32 twin's")
            recs += r
            fails += f
        tr.check_comm()
        if tr.step_ctr.tolist() != [tr.t] * N_MODELS:
            fails.append(f"{cell.id}: step counters {tr.step_ctr.tolist()} != {tr.t}")
    finally:
        tr.close()
    if cell.prec == "bf16":
        fails += check_bf16(cell, recs)
    # (the conditions on the inputs are checked on the CPU engine's trajectory,
    # tests/test_step_matrix_cpu.py: Y at a snapshot a rounding apart is another draw)
    return recs, fails


# ------------------------------------------------------------------------------ a cell of W ranks
def _all_ranks(ok: bool) -> bool:
    """True on every rank iff ``ok`` on every rank: the ranks leave a cell together, whatever
    failed on one of them (no rank is left alone in a collective)."""
    import torch.distributed as dist

    flag = torch.tensor([0.0 if ok else 1.0])
    dist.all_reduce(flag)
    return flag.item() == 0.0


def run_cell_rank(cell: Cell, device) -> dict:
    """One rank's part of a cell of ``cell.world`` ranks (the process group is initialised, every
    rank calls this with the same cell): the read-outs of :func:`run_cell`, returned raw --
    ``evaluate_cell_world`` holds them to the references in the parent, once for all ranks.
    Nothing is retried; after an error the ranks agree to end the cell."""
    import torch.distributed as dist

    rank = dist.get_rank()
    out = {"cell": cell.id, "rank": rank, "readouts": [], "fails": []}
    tr = make_trainer(cell, device, rank=rank)
    try:
        out["pick"] = [tr.lanes, tr.kernel_waves, tr.groups]
        out["comm"], out["fallback"] = tr.comm, tr.comm_fallback_reason
        ok = tr.comm == "xgmi" and tuple(out["pick"]) == cell.expect
        if not _all_ranks(ok):
            return out
        for t in readout_steps(cell):
            err = None
            try:
                if tr.t < t:
                    dist.barrier()
                    tr.train(t - tr.t)
                sg = step_gradient_world(tr)
                assert sg.t == t
                out["readouts"].append(tuple(sg))
            except Exception as e:  # an exchange timeout (tr.synchronize), a launch error
                err = f"rank {rank} t={t}: {type(e).__name__}: {e}"
                out["fails"].append(err)
            if not _all_ranks(err is None):
                return out
            if t == 0 and cell.prec == "bf16":
                tw = make_trainer(cell, device, prec="fp32", rank=rank)
                try:
                    out["twin_grad"] = step_gradient_world(tw).grad
                finally:
                    tw.close()
        try:
            tr.check_comm()
        except Exception as e:
            out["fails"].append(f"rank {rank}: {e}")
        out["step_ctr"], out["t"] = tr.step_ctr.tolist(), tr.t
        out["comm_after"], out["fallback_after"] = tr.comm, tr.comm_fallback_reason
    finally:
        tr.close()
    return out


def evaluate_cell_world(cell: Cell, res: dict) -> tuple[list[dict], list[str]]:
    """(records, failures) of a cell of several ranks from ``res[rank]`` = :func:`run_cell_rank`'s
    result: the dispatcher's pick and the exchange in use on every rank, the step counters, the
    read-out, logged loss and parameters ``torch.equal`` across the ranks (rank-order sums: the
    protocol's replica guarantee), then rank 0's read-outs against the references."""
    W = cell.world
    recs, fails = [], []
    if sorted(res) != list(range(W)):
        return [], [f"{cell.id}: results of ranks {sorted(res)}, expected {W}"]
    steps = readout_steps(cell)
    for r in range(W):
        o = res[r]
        fails += [f"{cell.id}: {m}" for m in o["fails"]]
        if o["comm"] != "xgmi" or o["fallback"] is not None:
            fails.append(f"{cell.id} rank {r}: comm {o['comm']!r} (fallback: {o['fallback']})")
        if tuple(o["pick"]) != cell.expect:
            fails.append(f"{cell.id} rank {r}: the dispatcher picked (lanes, waves, groups) = {tuple(o['pick'])}, "
                         f"expected {cell.expect}")
        if len(o["readouts"]) != len(steps):
            fails.append(f"{cell.id} rank {r}: {len(o['readouts'])} of {len(steps)} read-outs")
    if fails:
        return recs, fails
    X, Y = cell_data(cell)
    for r in range(W):
        o = res[r]
        if o["comm_after"] != "xgmi" or o["fallback_after"] is not None:
            fails.append(f"{cell.id} rank {r}: comm {o['comm_after']!r} after the steps")
        if o["step_ctr"] != [steps[-1] + 1] * N_MODELS or o["t"] != steps[-1] + 1:
            fails.append(f"{cell.id} rank {r}: step counters {o['step_ctr']}, t = {o['t']}, expected {steps[-1] + 1}")
    for k, t in enumerate(steps):
        sgs = [StepGradient(*res[r]["readouts"][k]) for r in range(W)]
        for r in range(1, W):
            for name in ("params_before", "grad", "loss", "params_after"):
                if not torch.equal(getattr(sgs[r], name), getattr(sgs[0], name)):
                    fails.append(f"{cell.id} t={t}: {name} of rank {r} differs from rank 0's")
        assert sgs[0].t == t
        rc, f = evaluate_step(cell, sgs[0], cell_indices(cell, t), X, Y)
        for x in rc:
            x["instance"], x["world"] = list(cell.expect), W
        if t == 0 and cell.prec == "bf16":
            for i, x in enumerate(rc):
                g32 = res[0]["twin_grad"]
                x["vs_fp32_twin"] = max(metric(cell.spec, sgs[0].grad[i], g32[i]).values())
                if torch.equal(sgs[0].grad[i], g32[i]):
                    f.append(f"{cell.id} model {i}: the bf16 read-out equals the fp32 twin's")
        recs += rc
        fails += f
    if cell.prec == "bf16":
        fails += check_bf16(cell, recs)
    return recs, fails


def main(argv: list[str]) -> int:
    """Child process of the forced-instance tests: ``python -m tests.step_cases OUT.json CELL_ID...``
    runs the cells on GPU 0 and writes {"records": [...], "failures": [...]}."""
    out, ids = argv[0], argv[1:]
    recs, fails = [], []
    for cid in ids:
        r, f = run_cell(BY_ID[cid], torch.device("cuda", 0))
        recs += r
        fails += f
    with open(out, "w") as fh:
        json.dump({"records": recs, "failures": fails}, fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

"""Every stage kernel instance of ``csrc/mlp_stage.hip``, forward and backward, against fp64
autograd -- one cell per ``Stage<...>`` instantiation of a kernel family (``fwd``, ``fwd_multi``,
``bwd<WANT_DX=true>``, ``bwd<WANT_DX=false>``, ``bwd_opt``).

Shared by ``tests/test_stage_matrix_gpu.py`` and ``tests/test_stage_matrix_cpu.py``; CPU-only
code except the ``launch_*`` / ``run_*`` functions, which drive the kernels on the device they
are given.  Helpers and constants of the step matrix (``tests/step_cases.py``) are reused.

**Inputs** are coherent, not ``randn``: random-sign upstream gradients make every dW a
cancelling sum and the yardstick meaningless.  Data: the first B rows of
``ToyData(n=4096, seed=21)`` (``ToyData(n=B, seed=21)`` above 4096); parameters
``randn(P, seed 1) * 0.4``.

* Sub-stage shapes are layers a..b of the toy model (:data:`SUBSTAGE`): ``x`` is the toy
  model's fp64 activation entering layer a, ``grad_out`` the fp64 gradient of the toy MSE loss
  with respect to the output of layer b (after its activation), both rounded to fp32 as the
  layer-split pipeline hands them over; the parameters are the toy vector's ``param_range(a, b)``.
* Whole-model shapes: ``x`` is the data (IN = 4: ``[x, x * x]``), the targets those of
  ``step_cases.cell_data`` (OUT = 4: ``[y, y / 2, -y, x0]``, OUT = 2: ``[y, -y / 2]``) and
  ``grad_out = 2 (out64 - target) / numel``.
* The slope-0.2 cells of a FINAL_ACT stage replace the last ``KINK_ROWS`` rows of ``x`` by free
  draws: on the toy data some output columns never change sign (:func:`stage_inputs`).
* The models of a multi-model launch (``fwd_multi``, ``bwd_opt``) draw their parameters from
  consecutive seeds; the conditions below are asserted for each of them.

**Conditions on the inputs** (asserted from the references alone, on the CPU): ``Y <= 2e-6`` for
every parameter tensor and for ``out``, ``Y <= 4e-6`` for ``grad_in``, and every tensor's
``max|g64|`` at least 1e-2 of the gradient's.

**Metric.**  Per parameter tensor, for ``out``, for ``grad_in`` and per saved hidden layer
(``saved1`` ..): ``E = max|v - v64| / max|v64|``; ``v64`` is fp64 autograd on the same fp32 inputs.

**fp32 bound.**  ``E <= max(4 Y, 8 * 2^-24)``, ``Y`` the same metric of plain fp32 CPU autograd on
the same case (the step matrix's rule).  ``Y`` is a property of the CPU's BLAS as much as of the
case: one that sums the K = batch dimension of ``dz^T h`` in a single chain has Y = 1e-4 .. 3e-4
for a weight gradient at B = 263169 (seen on the GPU machine's host; 3e-7 where the conditions
were measured).  The conditions below are what the bound rests on, so ``Y`` enters the bound
capped at them (:func:`y_limit`): a poor yardstick never widens a bound.

**Reduction margin** (:func:`stage_margin`), added to the parameter tensors' bound of the
multi-block cells (B > 1024) and of cells marked ``own_margin``.  It is the reduction site of
``step_cases.fp32_margin`` with the upstream gradient taken as given (no loss site): a dW
element is a sum of ``dz_s h_s`` over the batch whose partial sums each round at most
``u sum|terms|``, so with the roundings independent and of mean zero its error is within
``LAMBDA u sqrt(n) sum_s |dz_s| |h_s|`` (plus ``|prefill|`` where the kernel adds into a
pre-filled buffer) but for a probability of 2 exp(-LAMBDA^2 / 2).  ``n`` is the longest chain of
additions behind one element, read from the kernel (:func:`chain_length`): 64 samples per wave
and 256-sample chunk, ``ceil(ceil(B / 256) / gridDim)`` chunks per block, 4 waves, ``gridDim``
atomic adds in free order, the ``acc0 + acc1`` merge and the accumulate add.  The per-sample
sites of ``fp32_margin`` (forward, dh) are left out: they are what ``Y`` itself samples, and
leaving them out only makes the margin smaller.  ``dz`` and ``h`` are the fp64 reference's: the
margin is a function of the reference's values only, never of the kernel's output.

**bf16 bound.**  The reference is the rounding model ``mlp_forward_ref_bf16`` in fp64
(:func:`forward_parts` with ``bf16=True`` is the same function that also returns the hidden
activations; ``tests/test_stage_matrix_cpu.py`` holds the two bitwise equal).  ``D`` is the metric
between that and the fp32 model, both in fp64.  Required per quantity (the parameter gradient:
the largest over its tensors, as in the step matrix; ``out``; ``grad_in``; ``saved``: the largest
over the layers): ``E <= D / 2`` -- the kernel is nearer the bf16 recipe than fp32 compute is --
with the precondition ``D >= 100 Y`` asserted on the CPU; ``out`` is bf16-representable and the
results differ from the fp32 twin's.  No rows are excluded.

**bwd_opt read-out**, as in the step matrix: with ``beta1 = 0`` and a zero moment ``opt_m`` is
the gradient bit for bit (``adam_update``: ``m = fmaf(1 - b1, g - m, m)``; ``sgd_update``: ``buf = g``
on the first step, ``fmaf(buf, mom, g)`` later), and without ``DTP_OPT_ZERO_GRAD`` ``grad_params``
holds it as well.  "Applied = stored" by ``step_cases.applied_is_stored``.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import re
from dataclasses import dataclass
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.ops.mlp import MlpSpec, bf16_round, unflatten

from . import step_cases as sc
from .step_cases import DATA_SEED, INIT_SEED, LAMBDA, U, tensor_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_training_pytorch_amd", "csrc")
DATA_ROWS = 4096
KINK_ROWS = 16

# ------------------------------------------------------------------------------ the shapes
# written out from csrc/mlp_shapes.h, NOT read from it: tests/test_stage_matrix_cpu.py compares
TOY = (2, 10, 5, 1, 0)
SUBSTAGE = {  # (IN, H, NL, OUT, FINAL_ACT) -> layers (a, b) of the toy model
    (2, 10, 4, 10, 1): (0, 3), (10, 10, 4, 1, 0): (1, 4), (2, 10, 3, 10, 1): (0, 2), (10, 10, 3, 10, 1): (1, 3),
    (10, 10, 3, 1, 0): (2, 4), (2, 10, 2, 10, 1): (0, 1), (10, 10, 2, 10, 1): (1, 2), (10, 10, 2, 1, 0): (3, 4),
    (2, 10, 1, 10, 1): (0, 0), (10, 10, 1, 10, 1): (1, 1), (10, 10, 1, 1, 0): (4, 4),
}
WHOLE = [TOY, (2, 10, 3, 1, 0), (2, 10, 5, 2, 0), (2, 10, 5, 4, 0), (2, 15, 5, 1, 0), (2, 15, 5, 4, 0), (4, 15, 5, 4, 0)]
FP32_SHAPES = [TOY] + list(SUBSTAGE) + WHOLE[1:]
BF16_SHAPES = [TOY, (2, 10, 5, 4, 0)]
MID, H15, IN4 = (10, 10, 3, 10, 1), (2, 15, 5, 4, 0), (4, 15, 5, 4, 0)
EDGE_SHAPES = [TOY, MID, H15, IN4]
EDGE_BATCHES = [1, 7, 63, 255, 256, 1023, 1024, 1025, 2049, 3000]
LARGE = 256 * 1024 + 1025  # 258 blocks capped to 256: two blocks take a second grid-stride round
K_BLOCK = 256              # csrc/dtp_common.h kBlock (tests/test_stage_matrix_cpu.py compares)
BLOCK_CAP = 256            # launch_stage_bwd


def spec_of(key, slope: float = 0.01) -> MlpSpec:
    return MlpSpec(key[0], key[1], key[2], key[3], bool(key[4]), slope)


def n_blocks(B: int) -> int:
    """gridDim of launch_stage_bwd: one block per 4 chunks of kBlock samples, at most 256."""
    return min(-(-B // (4 * K_BLOCK)), BLOCK_CAP)


def chain_length(B: int) -> int:
    """Longest chain of fp32 additions behind one dW element of the stage backward."""
    grid = n_blocks(B)
    chunks = -(-(-(-B // K_BLOCK)) // grid)
    return 64 * chunks + 4 + grid + 2


# ------------------------------------------------------------------------------ the cells
@dataclass(frozen=True)
class Cell:
    family: str                # fwd | bwd_dx | bwd_nodx | acc | fwd_multi | bwd_opt
    key: tuple                 # (IN, H, NL, OUT, FINAL_ACT)
    batch: int
    prec: str = "fp32"
    slope: float = 0.01
    n: int = 1                 # models in the launch (fwd_multi, bwd_opt)
    opt: str = ""              # bwd_opt: adam | sgd
    own_margin: bool = False   # a single-block cell given the reduction margin (README)

    @property
    def id(self) -> str:
        s = f"{self.family}-{'x'.join(str(k) for k in self.key)}-b{self.batch}-{self.prec}"
        if self.slope != 0.01:
            s += f"-s{self.slope}"
        if self.family in ("fwd_multi", "bwd_opt"):
            s += f"-n{self.n}"
        if self.opt:
            s += f"-{self.opt}"
        return s

    @property
    def spec(self) -> MlpSpec:
        return spec_of(self.key, self.slope)

    @property
    def multi_block(self) -> bool:
        return self.batch > 4 * K_BLOCK


def _cells():
    out = []
    # fwd and bwd with grad_in: every shape at 65 and 257, the four edge shapes at the batch edges
    for fam in ("fwd", "bwd_dx"):
        out += [Cell(fam, k, b) for k in FP32_SHAPES for b in (65, 257)]
        out += [Cell(fam, k, b) for k in EDGE_SHAPES for b in EDGE_BATCHES]
    # bwd without grad_in
    out += [Cell("bwd_nodx", k, 257) for k in FP32_SHAPES]
    out += [Cell("bwd_nodx", k, b) for k in EDGE_SHAPES for b in (1, 1024, 1025)]
    # above the block cap (not the toy shape: fp32 torch's own error on its 1-wide output
    # layer is 3.3e-5 at this size)
    out += [Cell("fwd", MID, LARGE), Cell("bwd_dx", MID, LARGE), Cell("fwd", IN4, LARGE), Cell("bwd_nodx", IN4, LARGE)]
    # accumulate into a pre-filled grad_params
    out += [Cell("acc", k, b) for k in (TOY, (10, 10, 1, 1, 0), IN4) for b in (256, 1024, 1025, 3000)]
    # bf16
    out += [Cell(fam, k, b, prec="bf16") for fam in ("fwd", "bwd_dx", "bwd_nodx") for k in BF16_SHAPES
            for b in (7, 257, 1025)]
    # slope is a run-time argument
    out += [Cell(fam, k, 257, slope=0.2) for fam in ("fwd", "bwd_dx", "bwd_nodx") for k in (TOY, (10, 10, 2, 10, 1))]
    # several models in one launch
    out += [Cell("fwd_multi", k, 300, n=n) for k in (TOY, H15, (10, 10, 2, 1, 0)) for n in (1, 2, 3, 4)]
    out += [Cell("bwd_opt", k, b, n=n, opt=o) for k in (TOY, H15, IN4) for n in (1, 2, 4) for b in (1, 256, 257, 1024)
            for o in ("adam", "sgd")]
    # both families are instantiated for every DTP_STAGE_SHAPES row: the other shapes once each
    out += [Cell("fwd_multi", k, 300, n=2) for k in FP32_SHAPES if k not in (TOY, H15, (10, 10, 2, 1, 0))]
    out += [Cell("bwd_opt", k, 257, n=2, opt=("adam", "sgd")[i % 2]) for i, k in enumerate(FP32_SHAPES)
            if k not in (TOY, H15, IN4)]
    return out


CELLS = _cells()
BY_ID = {c.id: c for c in CELLS}
assert len(BY_ID) == len(CELLS), "duplicate cell ids"
MULTI_BATCHES = (300, 1, 257, 64)   # fwd_multi: model i's batch; the grid is sized by the largest
OPT_STEPS = (0, 5, 2, 7)            # bwd_opt: model i's step counter before the launch


def models_of(cell: Cell) -> list[tuple[int, int]]:
    """(model, batch) of every model the cell launches."""
    if cell.family == "fwd_multi":
        return [(i, MULTI_BATCHES[i]) for i in range(cell.n)]
    return [(i, cell.batch) for i in range(cell.n)]


# ------------------------------------------------------------------------------ the model
class _R(torch.autograd.Function):  # bf16 value, bf16 gradient
    @staticmethod
    def forward(ctx, t):
        return bf16_round(t)

    @staticmethod
    def backward(ctx, g):
        return bf16_round(g)


class _RP(torch.autograd.Function):  # a parameter: bf16 operand, fp32 gradient
    @staticmethod
    def forward(ctx, t):
        return bf16_round(t)

    @staticmethod
    def backward(ctx, g):
        return g


def forward_parts(flat, spec: MlpSpec, x, bf16: bool = False):
    """(out, [z_l], [h_{l+1}]): ``mlp_forward_ref`` / ``mlp_forward_ref_bf16`` with every layer's
    pre-activation and output kept."""
    ps = unflatten(flat, spec)
    r = _R.apply if bf16 else (lambda t: t)
    rp = _RP.apply if bf16 else (lambda t: t)
    h, zs, hs = r(x), [], []
    for l in range(spec.n_layers):
        z = r(F.linear(h, rp(ps[2 * l]), rp(ps[2 * l + 1])))
        h = r(F.leaky_relu(z, spec.slope)) if spec.act(l) else z
        zs.append(z)
        hs.append(h)
    return h, zs, hs


def reference(spec: MlpSpec, p, x, go, dtype, bf16: bool = False) -> dict:
    """Forward and backward of one stage by plain autograd in ``dtype`` on the CPU, the
    upstream gradient ``go`` given."""
    q = p.detach().to(dtype).clone().requires_grad_(True)
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    out, zs, hs = forward_parts(q, spec, xx, bf16)
    gr = torch.autograd.grad(out, [q, xx] + zs, grad_outputs=go.to(dtype))
    hid = [h.detach() for h in hs[:-1]]
    return {"out": out.detach(), "saved": torch.cat(hid, 1) if hid else None, "grad_params": gr[0], "grad_in": gr[1],
            "dz": list(gr[2:]), "h_in": [xx.detach()] + hid}


# ------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def toy_rows(n: int):
    ds = ToyData(n=n, seed=DATA_SEED)
    return ds.X, ds.Y


def init_params(P: int, model: int = 0) -> torch.Tensor:
    """Model 0 is the issue's vector; the further models of a multi-model launch draw theirs
    from the next seeds."""
    return torch.randn(P, generator=torch.Generator().manual_seed(INIT_SEED + model)) * 0.4


def stage_inputs(key, B: int, slope: float = 0.01, model: int = 0):
    """(spec, params [P], x [B, IN], grad_out [B, OUT]), fp32 on the CPU (module docstring)."""
    spec = spec_of(key, slope)
    X, Y = toy_rows(DATA_ROWS if B <= DATA_ROWS else B)
    X, Y = X[:B], Y[:B]
    if key in SUBSTAGE:
        a, b = SUBSTAGE[key]
        toy = spec_of(TOY, slope)
        pt = init_params(toy.P, model)
        out, _, hs = forward_parts(pt.double(), toy, X.double())
        leaf = hs[b].detach().requires_grad_(True)
        h = leaf
        for l in range(b + 1, toy.n_layers):
            W, bias = unflatten(pt.double(), toy)[2 * l: 2 * l + 2]
            h = F.linear(h, W, bias)
            if toy.act(l):
                h = F.leaky_relu(h, slope)
        (go,) = torch.autograd.grad(F.mse_loss(h, Y.double()), leaf)
        assert torch.equal(h.detach(), out)
        x = X.double() if a == 0 else hs[a - 1].detach()
        lo, hi = toy.param_range(a, b)
        assert hi - lo == spec.P and toy.substage(a, b).key == spec.key
        x = x.float().contiguous()
        if slope != 0.01 and spec.final_act:
            # the slope cells: on the toy data some output columns of a mid-network stage never
            # change sign, and leaky_grad_from_out(out) must see both; the last KINK_ROWS rows
            # of x are free draws (their upstream gradient rows stay), which puts a negative
            # and a positive output into every column (asserted on the reference, CPU)
            x[-KINK_ROWS:] = torch.randn(KINK_ROWS, spec.in_features, generator=torch.Generator().manual_seed(INIT_SEED))
        return spec, pt[lo:hi].clone(), x, go.float().contiguous()
    p = init_params(spec.P, model)
    x = torch.cat([X, X * X], 1).contiguous() if spec.in_features == 4 else X
    tgt = {1: Y, 2: torch.cat([Y, -0.5 * Y], 1), 4: torch.cat([Y, 0.5 * Y, -Y, X[:, :1]], 1)}[spec.out_features]
    out, _, _ = forward_parts(p.double(), spec, x.double())
    go = 2.0 * (out - tgt.double()) / out.numel()
    return spec, p, x.contiguous(), go.float().contiguous()


class Case:
    """One stage on one batch: the inputs and the fp64 / fp32 / rounding-model references."""

    def __init__(self, key, B, slope, model, bf16):
        self.key, self.batch, self.bf16 = key, B, bf16
        self.spec, self.p, self.x, self.go = stage_inputs(key, B, slope, model)
        self.r64 = reference(self.spec, self.p, self.x, self.go, torch.float64)
        self.Y = errors(self.spec, reference(self.spec, self.p, self.x, self.go, torch.float32), self.r64)
        self.rb = self.D = None
        if bf16:
            self.rb = reference(self.spec, self.p, self.x, self.go, torch.float64, bf16=True)
            self.D = errors(self.spec, self.rb, self.r64)

    @property
    def ref(self) -> dict:
        return self.rb if self.bf16 else self.r64


@functools.lru_cache(maxsize=None)
def _small_case(key, B, slope, model, bf16) -> Case:
    return Case(key, B, slope, model, bf16)


@functools.lru_cache(maxsize=1)
def _large_case(key, B, slope, model, bf16) -> Case:  # hundreds of MB of fp64: only the last one is kept
    return Case(key, B, slope, model, bf16)


def get_case(key, B: int, slope: float = 0.01, model: int = 0, bf16: bool = False) -> Case:
    """The case, computed once (its references are shared by the cells and left unchanged)."""
    return (_small_case if B <= DATA_ROWS else _large_case)(key, B, slope, model, bf16)


def cases_of(cell: Cell) -> list[Case]:
    return [get_case(cell.key, b, cell.slope, i, cell.prec == "bf16") for i, b in models_of(cell)]


# ------------------------------------------------------------------------------ metric, bounds
def saved_names(spec) -> list[str]:
    return [f"saved{l}" for l in range(1, spec.n_layers)]


def errors(spec, got: dict, ref: dict, offset=None) -> dict:
    """E per quantity present in ``got``: max|v - v64| / max|v64| (``offset``: a pre-filled
    ``grad_params`` the kernel added into; the norm stays the gradient's)."""
    E = {}

    def put(name, v, r):
        E[name] = ((v.detach().cpu().double() - r.double()).abs().max() / r.double().abs().max()).item()

    if got.get("grad_params") is not None:
        g = got["grad_params"].detach().cpu().double()
        if offset is not None:
            g = g - offset.double()
        for n, a, b in zip(tensor_names(spec), unflatten(g, spec), unflatten(ref["grad_params"].double(), spec)):
            put(n, a, b)
    for name in ("out", "grad_in"):
        if got.get(name) is not None:
            put(name, got[name], ref[name])
    if got.get("saved") is not None:
        H = spec.hidden
        for l, n in enumerate(saved_names(spec)):
            put(n, got["saved"][:, l * H:(l + 1) * H], ref["saved"][:, l * H:(l + 1) * H])
    return E


def y_limit(name: str) -> float:
    """The condition on the inputs for quantity ``name`` (``saved`` as ``out``): the most ``Y``
    may be, here and in the bound."""
    return 4e-6 if name == "grad_in" else 2e-6


def stage_margin(case: Case, n_sum: int, prefill=None) -> dict:
    """The reduction margin per parameter tensor over ``max|g64|`` (module docstring)."""
    spec, r = case.spec, case.r64
    mags = []
    for l in range(spec.n_layers):
        dz, h = r["dz"][l].abs(), r["h_in"][l].abs()
        mags += [(dz.T @ h).reshape(-1), dz.sum(0)]
    mag = torch.cat(mags)
    if prefill is not None:
        mag = mag + prefill.double().abs()
    bound = LAMBDA * math.sqrt(n_sum) * U * mag
    return {n: (b.max() / g.abs().max()).item()
            for n, b, g in zip(tensor_names(spec), unflatten(bound, spec), unflatten(r["grad_params"], spec))}


def evaluate(cell: Cell, case: Case, got: dict, model: int = 0, prefill=None, calls: int = 1, what: str = "") -> tuple:
    """(record, failures) of one result against the references.  ``prefill``: what
    ``grad_params`` held before ``calls`` accumulating launches (the reference is then
    ``prefill + calls * g64``, each launch's error adding)."""
    spec = case.spec
    Yc = {n: min(v, y_limit(n)) for n, v in case.Y.items()}
    rec = {"cell": cell.id, "family": cell.family, "model": model, "batch": case.batch, "Y": case.Y,
           "Y_capped": [n for n, v in case.Y.items() if v > y_limit(n)]}
    fails, tag = [], f"{cell.id}{' ' + what if what else ''} model {model}"
    off = None
    if prefill is not None:
        off = prefill.double() + (calls - 1) * case.ref["grad_params"].double()
    E = errors(spec, got, case.ref, off)
    rec["E"] = E
    if what:
        rec["what"] = what
    params = [n for n in tensor_names(spec) if n in E]
    if not case.bf16:
        bound = {n: max(4 * Yc[n], 8 * U) for n in E}
        if params and (case.batch > 4 * K_BLOCK or cell.own_margin):
            mt = stage_margin(case, chain_length(case.batch), prefill)
            rec["margin"] = mt
            for n in params:
                bound[n] = calls * (bound[n] + mt[n])
        elif params and prefill is not None:
            # one block: the one rounding of `grad_params[p] + g`, at most u |prefill + g|
            tot = unflatten(off + case.r64["grad_params"], spec)
            g64 = unflatten(case.r64["grad_params"], spec)
            for n, a, b in zip(tensor_names(spec), tot, g64):
                bound[n] = calls * (bound[n] + U * (a.abs().max() / b.abs().max()).item())
        rec["bound"] = bound
        rec["ratio"] = {n: E[n] / max(Yc[n], 2 * U) for n in E}
        for n in E:
            if not E[n] <= bound[n]:
                fails.append(f"{tag} {n}: E {E[n]:.3e} > bound {bound[n]:.3e} (Y {case.Y[n]:.3e}, "
                             f"E/Y {E[n] / max(case.Y[n], 1e-300):.2f})")
    else:
        rec["D"] = {n: case.D[n] for n in E}
        groups = {"grad_params": params, "out": ["out"], "grad_in": ["grad_in"], "saved": saved_names(spec)}
        rec["bound"], rec["ratio"] = {}, {}
        for q, names in groups.items():
            names = [n for n in names if n in E]
            if not names:
                continue
            e, d = max(E[n] for n in names), max(case.D[n] for n in names)
            rec["bound"][q], rec["ratio"][q] = d / 2, e / d
            if not e <= d / 2:
                fails.append(f"{tag} {q}: E {e:.3e} > D / 2 = {d / 2:.3e}")
        if got.get("out") is not None and not torch.equal(bf16_round(got["out"]), got["out"]):
            fails.append(f"{tag}: out is not bf16-representable")
    return rec, fails


def check_conditions(case: Case) -> list[str]:
    """The conditions on the inputs, from the references alone."""
    spec, Y, fails = case.spec, case.Y, []
    tag = f"{case.key} b{case.batch}"
    names = tensor_names(spec)
    lim = {n: y_limit(n) for n in names + ["out", "grad_in"]}
    for n, v in lim.items():
        if not Y[n] <= v:
            fails.append(f"{tag}: Y[{n}] {Y[n]:.2e} > {v:.0e}")
    mx = [t.abs().max().item() for t in unflatten(case.r64["grad_params"], spec)]
    if not min(mx) >= 1e-2 * max(mx):
        fails.append(f"{tag}: a tensor's max|g64| is {min(mx) / max(mx):.2e} of the gradient's")
    if case.bf16:
        for q, ns in (("grad_params", names), ("out", ["out"]), ("grad_in", ["grad_in"])):
            d, y = max(case.D[n] for n in ns), max(Y[n] for n in ns)
            if not d >= 100 * y:
                fails.append(f"{tag}: D[{q}] {d:.2e} < 100 Y = {100 * y:.2e}")
    return fails


def prefill_vector(P: int, model: int = 0) -> torch.Tensor:
    return (0.1 * torch.cos(torch.arange(P, dtype=torch.float64) + model)).float()


# ------------------------------------------------------------------------------ header
def header_shapes(macro: str) -> list[tuple]:
    """The X(...) rows of a shape macro of csrc/mlp_shapes.h."""
    with open(os.path.join(CSRC, "mlp_shapes.h")) as fh:
        text = fh.read()
    m = re.search(r"#define\s+%s\(X\)(.*?)(?:\n[ \t]*\n|\Z)" % re.escape(macro), text, re.S)
    assert m, macro
    rows = re.findall(r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(true|false)\)", m.group(1))
    return [(int(a), int(b), int(c), int(d), int(f == "true")) for a, b, c, d, f in rows]


# ------------------------------------------------------------------------------ launches
def guarded(t: torch.Tensor, fill: float, rows_after: int = K_BLOCK) -> tuple:
    """A copy of ``t`` as a view into a larger buffer: 64 floats of ``fill`` before it and
    ``rows_after`` rows (at least 64 floats) after it -- a whole chunk of rows, so that a lane
    past ``batch`` that did touch memory would still stay inside the buffer.
    Returns (buffer, view, numel of the view's offset)."""
    row = t.shape[1] if t.dim() == 2 else 1
    tail = max(64, rows_after * row)
    buf = torch.full((64 + t.numel() + tail,), fill, device=t.device, dtype=t.dtype)
    view = buf[64:64 + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def canary_intact(buf: torch.Tensor, view: torch.Tensor, fill: float) -> bool:
    n = view.numel()
    return bool((buf[:64] == fill).all() and (buf[64 + n:] == fill).all())


def launch_fwd(spec, x, p, out, saved, out_peer=None, bf16=False, batch=None, key=None) -> int:
    """dtp_mlp_stage_fwd on the caller's buffers; returns its return code."""
    from distributed_training_pytorch_amd import _native as nat

    lib = nat.require(x.device)
    a = nat.StageArgs(nat.ptr(x), nat.ptr(p), nat.ptr(out), nat.ptr(saved), None, None, None, nat.ptr(out_peer),
                      x.shape[0] if batch is None else batch, spec.slope, 0, int(bf16))
    return lib.dtp_mlp_stage_fwd(ctypes.byref(a), *(key or spec.key), nat.stream_ptr())


def launch_bwd(spec, x, p, out, saved, go, grad_in, gp, accumulate=False, bf16=False, batch=None, key=None) -> int:
    """dtp_mlp_stage_bwd on the caller's buffers (``gp`` zeroed by the caller where the launch
    has more than one block); returns its return code."""
    from distributed_training_pytorch_amd import _native as nat

    lib = nat.require(x.device)
    a = nat.StageArgs(nat.ptr(x), nat.ptr(p), nat.ptr(out), nat.ptr(saved), nat.ptr(go), nat.ptr(grad_in), nat.ptr(gp),
                      None, x.shape[0] if batch is None else batch, spec.slope, int(accumulate), int(bf16))
    return lib.dtp_mlp_stage_bwd(ctypes.byref(a), *(key or spec.key), nat.stream_ptr())


def stage_args(spec, x, p, out, saved, go=None, grad_in=None, gp=None, accumulate=False, bf16=False, batch=None):
    from distributed_training_pytorch_amd import _native as nat

    return nat.StageArgs(nat.ptr(x), nat.ptr(p), nat.ptr(out), nat.ptr(saved), nat.ptr(go), nat.ptr(grad_in),
                         nat.ptr(gp), None, x.shape[0] if batch is None else batch, spec.slope, int(accumulate),
                         int(bf16))


def launch_fwd_multi(key, stages) -> int:
    from distributed_training_pytorch_amd import _native as nat

    m = nat.StageMulti()
    m.n = len(stages)
    for i, s in enumerate(stages[:nat.STAGE_MULTI_MAX]):
        m.stage[i] = s
    return nat.require(None).dtp_mlp_stage_fwd_multi(ctypes.byref(m), *key, nat.stream_ptr())


def opt_config(name: str):
    return sc.ADAM if name == "adam" else sc.SGD


def launch_bwd_opt(key, stages, params, m, v, step, grad, opt: str, flags: int = 0, n=None, P=None, slope=0.01) -> int:
    """dtp_mlp_stage_bwd_opt: the stages' backwards and the optimizer's rows in one launch."""
    from distributed_training_pytorch_amd import _native as nat

    M = nat.StageMulti()
    M.n = len(stages) if n is None else n
    for i, s in enumerate(stages[:nat.STAGE_MULTI_MAX]):
        M.stage[i] = s
    cfg = opt_config(opt)
    o = nat.OptArgs(nat.ptr(params), nat.ptr(m), nat.ptr(v), nat.ptr(step), nat.ptr(grad), None, 0, M.n,
                    params.shape[1] if P is None else P, cfg.kind, 1.0, flags, cfg.hyper(slope, 1.0), None, 0, 0.0, 0.0,
                    None, None)
    return nat.require(params.device).dtp_mlp_stage_bwd_opt(ctypes.byref(M), ctypes.byref(o), *key, nat.stream_ptr())


def run_stage(cell: Cell, case: Case, dev, prec=None) -> dict:
    """The cell's kernels through ``ops.mlp.stage_forward`` / ``stage_backward``: what the
    family produces, on the CPU."""
    from distributed_training_pytorch_amd.ops.mlp import stage_backward, stage_forward

    bf = (prec or cell.prec) == "bf16"
    spec = case.spec
    x, p, go = case.x.to(dev), case.p.to(dev), case.go.to(dev)
    out, saved = stage_forward(x, p, spec, bf16=bf)
    assert (saved is None) == (spec.n_layers == 1)
    if cell.family == "fwd":
        got = {"out": out, "saved": saved}
    else:
        gin, gp = stage_backward(x, p, spec, out, saved, go, need_grad_in=cell.family != "bwd_nodx", bf16=bf)
        assert (gin is None) == (cell.family == "bwd_nodx")
        got = {"grad_params": gp, "grad_in": gin}
    torch.cuda.synchronize()
    return {k: (None if t is None else t.cpu()) for k, t in got.items()}


def run_cell(cell: Cell, dev) -> tuple[list[dict], list[str]]:
    """A fwd / bwd_dx / bwd_nodx cell on ``dev`` against the references: (records, failures)."""
    (case,) = cases_of(cell)
    got = run_stage(cell, case, dev)
    rec, fails = evaluate(cell, case, got)
    for k, t in got.items():
        if t is not None and not torch.isfinite(t).all():
            fails.append(f"{cell.id}: {k} is not finite")
    if cell.prec == "bf16":
        twin = run_stage(cell, case, dev, prec="fp32")
        for k, t in got.items():
            if t is not None and torch.equal(t, twin[k]):
                fails.append(f"{cell.id}: the bf16 {k} equals the fp32 twin's")
    return [rec], fails


def applied_is_stored(opt: str, t: int, p0, grad, p1) -> list[str]:
    """``step_cases.applied_is_stored`` for one row [P] whose counter stood at ``t``."""
    sg = sc.StepGradient(t, p0.view(1, -1), grad.view(1, -1), None, p1.view(1, -1))
    return sc.applied_is_stored(SimpleNamespace(opt=opt), sg, 0)

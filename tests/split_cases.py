"""The layer-split engines' gradient, read out exactly through the optimizer state, against fp64
autograd -- one cell per way ``parallel/layer_split.py:FusedLayerSplit`` can run a stage instance
of ``csrc/split_train.hip`` (one workgroup per stage) or ``csrc/split_lanes.hip`` (M member
workgroups per stage).

Shared by ``tests/test_split_matrix_gpu.py`` and ``tests/test_split_matrix_cpu.py``; CPU-only
code except :func:`run_cell` and :func:`run_cell_rank`.  Metric, bounds, constants, seeds and the
evaluation are those of ``tests/step_cases.py`` (``evaluate_step`` with ``n_models=1``: the
engine trains one model); a :class:`SplitCell` has the fields of ``step_cases.Cell`` that the
evaluation reads.

**Read-out.**  Every launch reloads each stage's moments from ``a.opt_m`` / ``a.opt_v`` in its
prologue -- ``split_stage_body_v1`` and ``split_stage_body_pipe`` (``mr[k] = own ? a.opt_m[p] :
0``, ``vr[k]`` likewise under Adam) and ``split_lanes_body`` (the same two lines; every member
loads them, the lead writes them back) -- and ``a.opt_m`` / ``a.opt_v`` are the pointers of
``eng.m[s]`` / ``eng.v[s]`` kept in the launch block.  All three bodies hand the optimizer
``g[k] * a.hp.grad_scale`` through ``adam_update`` / ``sgd_update`` of ``csrc/optim_core.h``, so
the argument of ``step_cases``' docstring holds: with ``beta1 = 0`` (Adam) or a zero buffer
(SGD, momentum 0.9: ``buf = g`` at step 0, ``fmaf(0, mom, g)`` later) the moment after one
step is the gradient bit for bit.  :func:`step_gradient`: ``eng.synchronize()``, zero every
``eng.m[s]`` and ``eng.v[s]`` in place, ``torch.cuda.synchronize()`` (the launches run on the
split streams), ``eng.train(1)``; ``torch.cat([m.cpu() for m in eng.m])`` is then the whole
model's gradient in torch order.  With W ranks it is the slot-order sum over the W x members
slots times ``grad_scale = 1 / W``, the same bits on every rank.

**Bounds.**  Per parameter tensor and for the logged loss ``E <= max(4 Y, 8 * 2^-24)`` against
fp64 autograd on the step's indices (the engine's ``EpochIndexStream`` order; several ranks: the
mean over the ranks' batches); ``applied_is_stored`` on the concatenated parameters; every
``eng.step[s] == eng.t`` and a clean ``check_comm()``.

**Own margin** (``own_margin=True``: ``fp32_margin_abs`` added to the bound).  Its ``sum_chain``,
the longest chain of fp32 additions behind one dW element, is read from the two ``.hip`` files
(:func:`split_sum_chain`):

* one workgroup per stage: one lane per sample, four waves of 64; a wave's 64 samples are the
  K dimension of its ``v_mfma_f32_16x16x4_f32`` tile (``mlp_backward`` / ``wave_outer_acc`` in
  v1, the ``Scal`` tiles of ``mlp_pipe.h`` in the pipelined body: 16 K-steps over two
  accumulators merged once), the four waves' tiles are added in wave order
  (``sum_partial_tiles`` / the ``for ww`` loop), the W ranks' in slot order
  (``xgmi_allreduce_slots``): 64 + 4 + W + 2;
* members: four lanes per sample, four waves of 16 samples (``SLCfg``: ``G = 16``, ``TS = 4``
  K-steps, two accumulators), the waves' parked tiles added in wave order (``s_ +=
  sm.red[ww][tp[k]]``), then the M members' (``grp_allreduce_split3``) or the W x M slots'
  (``xgmi_allreduce_g3``): 16 + 4 + W M + 2.

Both are ``step_cases.sum_chain`` at ``expect`` = (1, 4, 1) and (4, 4, M), which is what
:attr:`SplitCell.expect` hands the evaluation (``tests/test_split_matrix_cpu.py`` holds the two
to each other).  A cell takes the margin only where its excess comes from ``Y`` being an
unusually small draw, shown from the reference's own numbers in
``profiles/split_matrix/README.md``; the margin is a function of the reference only.

**Instances.**  :data:`INSTANCES` is written out from ``DTP_SPLIT_SHAPES`` of
``csrc/split_shapes.h`` (twelve stage shapes; both engines expand the one list, so the ids are
shared).  ``split_stage_body()``
runs a one-layer stage on ``split_stage_body_v1`` and a stage of >= 2 layers on
``split_stage_body_pipe`` while its dataset slice ``n (XW + YW)`` fits ``kSplitCache`` = 8192
floats, else on v1 (:func:`stage_body`).  A middle stage gathers nothing (0 <= 8192), so the
middle shapes of >= 2 layers (ids 6, 7) reach v1 only in a ``DTP_SPLIT_PIPE=0`` build and are
left out.  The members engine has one body; its launch refuses a dataset slice past ``kSLData`` =
4096 floats.
"""
from __future__ import annotations

import json
from dataclasses import dataclass

import torch

from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC, MlpSpec

from .step_cases import (ADAM, DATA_SEED, INIT_SEED, SAMPLER_SEED, SGD, U, StepGradient,  # noqa: F401
                         applied_is_stored, autograd_gradient, cell_data, cell_geom, cell_indices, cell_init,
                         check_conditions, evaluate_step, fp32_margin_abs, metric, per_tensor, readout_steps, rel)

K_SPLIT_CACHE = 8192   # kSplitCache (csrc/split_train.hip)
K_SL_DATA = 4096       # kSLData (csrc/split_lanes.hip)
K_SL_MAX_M = 8         # kSLMaxM
TIMEOUT_US = 500_000   # a dead link ends as the engine's RuntimeError within half a second
NL = TOY_SPEC.n_layers

# (IN, H, NL, OUT, FINAL_ACT, FIRST): DTP_SPLIT_SHAPES (csrc/split_shapes.h), id = position
SHAPES = [
    (2, 10, 5, 1, False, 1),
    (2, 10, 1, 10, True, 1), (2, 10, 2, 10, True, 1), (2, 10, 3, 10, True, 1), (2, 10, 4, 10, True, 1),
    (10, 10, 1, 10, True, 0), (10, 10, 2, 10, True, 0), (10, 10, 3, 10, True, 0),
    (10, 10, 1, 1, False, 0), (10, 10, 2, 1, False, 0), (10, 10, 3, 1, False, 0), (10, 10, 4, 1, False, 0),
]


def _instances():
    """(engine, body, shape id) of every stage instance a default build can run -- written out
    from the X-macro list, NOT derived from the cells."""
    out = [("lanes", "lanes", i) for i in range(12)]                 # split_lanes_kernel: one body per shape
    out += [("one", "pipe", i) for i in (0, 2, 3, 4, 6, 7, 9, 10, 11)]  # >= 2 layers, dataset slice cached
    out += [("one", "v1", i) for i in (1, 5, 8)]                      # the one-layer shapes
    out += [("one", "v1", i) for i in (0, 2, 3, 4, 9, 10, 11)]        # gathering, >= 2 layers, past the cache
    return out


INSTANCES = _instances()


def stage_shape(a: int, b: int) -> tuple:
    """The X-macro row of the stage of layers a..b of the toy model."""
    first, last = a == 0, b == NL - 1
    return (2 if first else 10, 10, b - a + 1, 1 if last else 10, not last, int(first))


def stage_body(engine: str, a: int, b: int, n: int) -> str:
    """The body ``split_stage_body()`` picks: ``n (XW + YW) <= 8192`` or the round-3 body."""
    if engine == "lanes":
        return "lanes"
    if b == a:
        return "v1"
    xw, yw = (2 if a == 0 else 0), (1 if b == NL - 1 else 0)
    return "pipe" if n * (xw + yw) <= K_SPLIT_CACHE else "v1"


# ------------------------------------------------------------------------------ the cells
@dataclass(frozen=True)
class SplitCell:
    part: tuple                # ((first layer, last layer), ...): the stages
    opt: str                   # adam | sgd
    batch: int                 # per rank
    members: int = 0           # 0: split_train.hip; M >= 1: split_lanes.hip with M members per stage
    auto: bool = False         # members="auto" must pick ``members``
    links: str = "auto"        # auto (device links: the stages share one GPU) | remote
    launch: str = "per_device"
    n: int = 512
    world: int = 1             # ranks (all on one GPU)
    own_margin: bool = False

    shape = "T"
    loss = "mse"
    prec = "fp32"

    @property
    def spec(self) -> MlpSpec:
        return TOY_SPEC

    @property
    def engine(self) -> str:
        return "lanes" if self.members else "one"

    @property
    def id(self) -> str:
        s = ("w%d-" % self.world if self.world != 1 else "") + (f"m{self.members}" if self.members else "one")
        s += ("a" if self.auto else "") + f"-{self.opt}-b{self.batch}-" + "_".join(f"{a}{b}" for a, b in self.part)
        if self.n != 512:
            s += f"-n{self.n}"
        if self.links != "auto":
            s += "-" + self.links
        if self.launch != "per_device":
            s += "-" + self.launch
        return s

    @property
    def expect(self) -> tuple:
        """(lanes, waves, groups) as ``step_cases.sum_chain`` counts them (module docstring)."""
        return (4, 4, self.members) if self.members else (1, 4, 1)

    @property
    def shape_ids(self) -> list[int]:
        return [SHAPES.index(stage_shape(a, b)) for a, b in self.part]

    @property
    def instances(self) -> list[tuple]:
        return [(self.engine, stage_body(self.engine, a, b, self.n), SHAPES.index(stage_shape(a, b)))
                for a, b in self.part]


def split_sum_chain(cell: SplitCell) -> int:
    """Longest chain of fp32 additions behind one dW element (module docstring)."""
    if cell.members:
        return 16 + 4 + cell.world * cell.members + 2
    return 64 + 4 + cell.world + 2


def part(text: str) -> tuple:
    """"01|24" -> ((0, 1), (2, 4))."""
    return tuple((int(s[0]), int(s[-1])) for s in text.split("|"))


def all_partitions() -> list[tuple]:
    """The 16 contiguous partitions of the 5 layers."""
    out = []
    for cuts in range(1 << (NL - 1)):
        st, a = [], 0
        for l in range(NL):
            if l == NL - 1 or (cuts >> l) & 1:
                st.append((a, l))
                a = l + 1
        out.append(tuple(st))
    return sorted(out)


REF = part("01|24")  # the reference's split
# the 8 partitions that cover all 12 shapes
COVER = [part(p) for p in ("04", "0|14", "01|24", "02|34", "03|4", "0|1|24", "0|12|34", "0|13|4")]


def _cells() -> list[SplitCell]:
    C = SplitCell
    out = []
    # 1. every partition, Adam, batch 200 (batches 200, 112, 200), both engines; members="auto": 4
    # members of 50 samples, on the 112-sample batch 50 / 50 / 12 / none
    for p in all_partitions():
        out += [C(p, "adam", 200), C(p, "adam", 200, members=4, auto=True)]
    # 2. SGD on the partitions that cover all 12 shapes: one workgroup at batch 256; 3 members at
    # batch 130 (slices of ceil(130 / 3) = 44: 44 / 44 / 42; the last batch of 122: 44 / 44 / 34)
    for p in COVER:
        out += [C(p, "sgd", 256), C(p, "sgd", 130, members=3, auto=True)]
    # 3. remote links: the 7 of those with a link, both engines, Adam at batch 200; one SGD cell
    # per engine; the reference's split with one launch per stage (a 2-GPU node's launch shape)
    for p in COVER[1:]:
        out += [C(p, "adam", 200, links="remote"), C(p, "adam", 200, members=4, auto=True, links="remote")]
    out += [C(REF, "sgd", 256, links="remote"), C(REF, "sgd", 130, members=3, auto=True, links="remote")]
    out += [C(REF, "adam", 200, links="remote", launch="per_stage"),
            C(REF, "adam", 200, members=4, auto=True, links="remote", launch="per_stage")]
    # 4. past the LDS cache (one workgroup, batch 256).  n = 4097: the first stage uncached, the
    # last cached, the epoch's last batch one sample; n = 8200: both uncached, last batch 8
    for p in ("04", "01|24", "02|34", "03|4", "0|14"):
        out += [C(part(p), "adam", 256, n=4097), C(part(p), "adam", 256, n=8200)]
    out.append(C(REF, "sgd", 256, n=8200))
    # 5. cache edges.  One workgroup: 4096 x 2 = 8192 exactly full; the whole model at 2730 x 3 =
    # 8190 (cached) and 2731 x 3 = 8193 (uncached).  Members: 2048 x 2 = 4096 exactly full; the
    # whole model at 1365 x 3 = 4095
    out += [C(REF, "adam", 256, n=4096), C(part("04"), "adam", 256, n=2730), C(part("04"), "adam", 256, n=2731),
            C(REF, "adam", 256, members=4, auto=True, n=2048), C(part("04"), "adam", 256, members=4, auto=True, n=1365)]
    # 6. member counts on the reference's split
    for m, b in ((1, 64), (1, 50), (2, 128), (2, 100), (3, 130), (4, 256), (5, 256), (6, 256), (7, 256), (8, 256),
                 (5, 200), (8, 200)):
        out.append(C(REF, "adam", b, members=m, auto=m == -(-b // 64)))
    out += [C(REF, "sgd", 64, members=1, auto=True), C(REF, "sgd", 256, members=5), C(REF, "sgd", 256, members=8)]
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


CELLS = _cells()

# 7. data parallel: W ranks on one GPU, one spawn per world size
WORLD_CELLS = [
    # W = 2 (256 samples per rank)
    SplitCell(part("01|23|4"), "sgd", 100, world=2),
    SplitCell(REF, "adam", 128, members=2, auto=True, world=2),                    # V = 4
    SplitCell(REF, "adam", 200, members=4, auto=True, world=2),                    # V = 8
    SplitCell(REF, "adam", 128, members=2, auto=True, world=2, links="remote"),
    # W = 3 (171 per rank, the list padded to 513)
    SplitCell(REF, "sgd", 100, world=3),
    SplitCell(REF, "adam", 100, members=2, auto=True, world=3),                    # V = 6
    # W = 4 (128 per rank; the 28-sample batch leaves member 1 of every rank empty)
    SplitCell(REF, "adam", 100, world=4),
    SplitCell(REF, "adam", 100, members=2, auto=True, world=4),                    # V = 8
    # W = 8 (64 per rank)
    SplitCell(REF, "adam", 50, world=8),
    SplitCell(REF, "adam", 50, members=1, auto=True, world=8),                     # V = 8
]
WORLDS = sorted({c.world for c in WORLD_CELLS})
ALL_CELLS = CELLS + WORLD_CELLS
BY_ID = {c.id: c for c in ALL_CELLS}
assert len(BY_ID) == len(ALL_CELLS), "duplicate cell ids"


# ------------------------------------------------------------------------------ engine and read-out
def make_engine(cell: SplitCell, device, rank: int = 0):
    from distributed_training_pytorch_amd.parallel.layer_split import FusedLayerSplit

    X, Y = cell_data(cell)
    members = 0 if not cell.members else ("auto" if cell.auto else cell.members)
    return FusedLayerSplit(TOY_SPEC, [device] * len(cell.part), X, Y, cell_geom(cell, rank),
                           ADAM if cell.opt == "adam" else SGD, cell_init(cell)[0], boundaries=list(cell.part),
                           timeout_us=TIMEOUT_US, launch=cell.launch, members=members, links=cell.links)


def check_engine(cell: SplitCell, eng) -> list[str]:
    """What the cell claims to run, asserted before it trains."""
    fails = []
    if eng.members != cell.members:
        fails.append(f"{cell.id}: {eng.members} members, expected {cell.members}")
    want = [cell.links == "auto"] * (len(cell.part) - 1)
    if list(eng.link_local) != want:
        fails.append(f"{cell.id}: link_local {eng.link_local}, expected {want}")
    ids = [int(eng.lib.dtp_split_shape_id(i, h, nl, o, int(f), fi))
           for i, h, nl, o, f, fi in (stage_shape(a, b) for a, b in cell.part)]
    launched = {s: int(L.shape_id[j]) for k, L in eng._launch.items() for j, s in enumerate(eng.groups[k])}
    if ids != cell.shape_ids or [launched[s] for s in range(len(cell.part))] != ids:
        fails.append(f"{cell.id}: shape ids {ids} (launched {launched}), expected {cell.shape_ids}")
    if len(eng._launch) != (len(cell.part) if cell.launch == "per_stage" else 1):
        fails.append(f"{cell.id}: {len(eng._launch)} launches")
    return fails


def step_gradient(eng, barrier=None) -> StepGradient:
    """Run step ``eng.t`` with zeroed moments and return the gradient it formed (module docstring),
    as a ``StepGradient`` of one model.  ``barrier``: called before the launch (several ranks)."""
    o = eng.optim
    assert (o.name == "adam" and o.betas[0] == 0.0) or (o.name == "sgd" and o.momentum != 0.0), o
    assert o.weight_decay == 0.0 and not o.clips
    eng.synchronize()
    p0 = eng.flat_params_cpu().clone()
    for m, v in zip(eng.m, eng.v):
        m.zero_()
        v.zero_()
    torch.cuda.synchronize()  # the split streams' next launches start after the zeroing
    t = eng.t
    if barrier is not None:
        barrier()
    eng.train(1)
    eng.synchronize()
    assert eng.t == t + 1
    g = torch.cat([m.detach().cpu() for m in eng.m])
    return StepGradient(t, p0[None], g[None], eng.losses(t, t + 1).view(1).clone(), eng.flat_params_cpu().clone()[None])


def evaluate(cell: SplitCell, sg: StepGradient) -> tuple[list[dict], list[str]]:
    """One read-out against the references on the engine's indices of step ``sg.t``."""
    X, Y = cell_data(cell)
    idx = cell_indices(cell, sg.t)
    recs, fails = evaluate_step(cell, sg, idx if cell.world > 1 else idx[0], X, Y, n_models=1)
    for r in recs:
        r["instances"] = [list(i) for i in cell.instances]
    return recs, fails


def table_line(r: dict) -> dict:
    """One read-out as its ``SPLIT_MATRIX`` line: E and Y in units of u = 2^-24 and E / Y (Y
    floored at 2 u), per tensor in torch order (W0, b0, .. W4, b4) and then of the loss, and the
    largest E / bound; two digits."""
    names = list(r["E"])
    sig = lambda x: float(f"{x:.2g}")  # noqa: E731
    return {"cell": r["cell"], "t": r["t"], "bsz": r["bsz"],
            "E_u": [sig(r["E"][n] / U) for n in names] + [sig(r["E_loss"] / U)],
            "Y_u": [sig(r["Y"][n] / U) for n in names] + [sig(r["Y_loss"] / U)],
            "E_over_Y": [sig(r["ratio"][n]) for n in names] + [sig(r["ratio_loss"])],
            "E_over_bound": sig(max(max(r["E"][n] / r["bound"][n] for n in names), r["E_loss"] / r["bound_loss"]))}


def report(recs: list[dict]) -> None:
    for r in recs:
        print("SPLIT_MATRIX " + json.dumps(table_line(r), separators=(",", ":")))


def run_cell(cell: SplitCell, device) -> tuple[list[dict], list[str]]:
    """The cell's three read-outs on ``device`` against the references: (records, failures)."""
    assert cell.world == 1
    eng = make_engine(cell, device)
    recs, fails = [], []
    try:
        fails += check_engine(cell, eng)
        if fails:
            return recs, fails
        for t in readout_steps(cell):
            if eng.t < t:
                eng.train(t - eng.t)
            sg = step_gradient(eng)
            assert sg.t == t
            r, f = evaluate(cell, sg)
            recs += r
            fails += f
        eng.check_comm()
        steps = [int(s.item()) for s in eng.step]
        if steps != [eng.t] * len(cell.part):
            fails.append(f"{cell.id}: step counters {steps} != {eng.t}")
    finally:
        eng.close()
    return recs, fails


# ------------------------------------------------------------------------------ a cell of W ranks
def _all_ranks(ok: bool) -> bool:
    """True on every rank iff ``ok`` on every rank: the ranks leave a cell together."""
    import torch.distributed as dist

    flag = torch.tensor([0.0 if ok else 1.0])
    dist.all_reduce(flag)
    return flag.item() == 0.0


def run_cell_rank(cell: SplitCell, device) -> dict:
    """One rank's part of a cell of ``cell.world`` ranks: the read-outs, returned raw
    (:func:`evaluate_world` holds them to the references in the parent).  Nothing is retried;
    after an error the ranks agree to end the cell."""
    import torch.distributed as dist

    rank = dist.get_rank()
    out = {"cell": cell.id, "rank": rank, "readouts": [], "fails": [], "done": False}
    eng = make_engine(cell, device, rank=rank)
    try:
        out["fails"] += check_engine(cell, eng)
        if not _all_ranks(not out["fails"]):
            return out
        for t in readout_steps(cell):
            err = None
            try:
                if eng.t < t:
                    dist.barrier()
                    eng.train(t - eng.t)
                sg = step_gradient(eng, barrier=dist.barrier)
                assert sg.t == t
                out["readouts"].append(tuple(sg))
            except Exception as e:  # a link or exchange timeout (eng.synchronize), a launch error
                err = f"rank {rank} t={t}: {type(e).__name__}: {e}"
                out["fails"].append(err)
            if not _all_ranks(err is None):
                return out
        try:
            eng.check_comm()
        except Exception as e:
            out["fails"].append(f"rank {rank}: {e}")
        out["steps"], out["t"] = [int(s.item()) for s in eng.step], eng.t
        out["done"] = True
    finally:
        eng.close()
    return out


def world_rank(rank: int, world: int, cell_ids: list[str]) -> dict:
    """The rank function of one spawn: that world's cells in order; the ranks stop together at the
    first cell that did not finish on every rank."""
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"cells": {}, "stopped": None}
    for cid in cell_ids:
        cell = BY_ID[cid]
        assert cell.world == world
        try:
            o = run_cell_rank(cell, device)
        except Exception as e:  # noqa: BLE001 - reported by every test of the spawn
            res["stopped"] = f"rank {rank} {cid}: {type(e).__name__}: {e}"
            break
        res["cells"][cid] = o
        if not o["done"]:
            res["stopped"] = f"rank {rank} {cid}: " + "; ".join(o["fails"])
            break
    return res


def evaluate_world(cell: SplitCell, res: dict) -> tuple[list[dict], list[str]]:
    """(records, failures) of a cell of several ranks from ``res[rank]`` = :func:`run_cell_rank`'s
    result: read-out, logged loss and parameters ``torch.equal`` across the ranks, the step
    counters, then rank 0's read-outs against the mean of fp64 autograd over the ranks' batches."""
    W = cell.world
    recs, fails = [], []
    if sorted(res) != list(range(W)):
        return [], [f"{cell.id}: results of ranks {sorted(res)}, expected {W}"]
    steps = readout_steps(cell)
    for r in range(W):
        o = res[r]
        fails += [f"{cell.id}: {m}" for m in o["fails"]]
        if len(o["readouts"]) != len(steps) or not o["done"]:
            fails.append(f"{cell.id} rank {r}: {len(o['readouts'])} of {len(steps)} read-outs")
    if fails:
        return recs, fails
    last = steps[-1] + 1
    for r in range(W):
        o = res[r]
        if o["steps"] != [last] * len(cell.part) or o["t"] != last:
            fails.append(f"{cell.id} rank {r}: step counters {o['steps']}, t = {o['t']}, expected {last}")
    for k, t in enumerate(steps):
        sgs = [StepGradient(*res[r]["readouts"][k]) for r in range(W)]
        for r in range(1, W):
            for name in ("params_before", "grad", "loss", "params_after"):
                if not torch.equal(getattr(sgs[r], name), getattr(sgs[0], name)):
                    fails.append(f"{cell.id} t={t}: {name} of rank {r} differs from rank 0's")
        assert sgs[0].t == t
        rc, f = evaluate(cell, sgs[0])
        for x in rc:
            x["world"] = W
        recs += rc
        fails += f
    return recs, fails

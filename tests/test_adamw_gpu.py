"""AdamW (decoupled weight decay, csrc/optim_core.h: decoupled_decay_step, adamw_update_v) through
every device code path that carries the optimizer update: the flat optimizer's branches and
launch shapes, the one-lane / lanes / split-batch fused steps with their clip and accumulation
twins, the layer-split stage kernels, the stage backward fused with the optimizer.

Two kinds of check.  *Exact read-outs*: with a gradient that is exactly zero Adam's term is
exactly zero and m = v = 0, so the parameters must be bitwise ``p0 * d_0 * ... * d_{n-1}``, each
``d_t = (float)(1 - lr_t * weight_decay)`` -- coupled Adam fails them (g = wd * p != 0), and so
does a decay formed from the base rate under a schedule.  *Trajectories*: 12 steps against fp64
autograd + torch.optim.AdamW at the tolerances of tests/test_optim_hyper_gpu.py; that the
yardstick tells AdamW from its twins at those tolerances is checked on the CPU
(tests/test_adamw_cpu.py).  Inputs: tests/adamw_cases.py."""
import ctypes
import dataclasses
import functools
import os
import subprocess
import sys

import pytest
import torch

from distributed_training_pytorch_amd import _native as nat
from distributed_training_pytorch_amd.data.sampler import EpochIndexStream, SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC
from distributed_training_pytorch_amd.ops.optim import OptimConfig, flat_optimizer_step
from distributed_training_pytorch_amd.parallel.layer_split import FusedLayerSplit

from . import adamw_cases as A
from . import sched_cases as C
from .dist_utils import run_ranks
from .ref_train import torch_train
from .test_loss_optim_gpu import _rank_job
from .test_module_path_gpu import _train_flat
from .test_optim_hyper_gpu import FLAT_CASES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the flat optimizer's branches and launch shapes: FLAT_CASES' Adam rows without their hyperparameter
# and grad_scale repeats -- 2x372, 4x371, 3x3, the bf16-shadow pair branch, the offset-gradient element
# branch, several blocks, the grid-stride loop, more models than a wavefront has lanes
FLAT_SHAPES = [(i, n, P, kw) for i, n, P, c, kw in FLAT_CASES
               if c == "all" and "grad_scale" not in kw and not (P == 372 and kw)]
assert [s[0] for s in FLAT_SHAPES] == ["f4-2x372", "f4-4x371", "f4-3x3", "pair-2x371", "elem-2x371", "blocks-3x20001",
                                       "stride-1x270003", "models-65x4100"]
FLAT_IDS = [s[0] for s in FLAT_SHAPES]
FLAT_ARGS = [s[1:] for s in FLAT_SHAPES]
FLAT_OPTS = {"plain": A.ADAMW, "ramp": A.ADAMW_RAMP}


def _flat_buffers(n, P, shadow=False, offset_grad=False, seed=0):
    gen = torch.Generator().manual_seed(1000 * n + P + seed)
    p0 = torch.randn(n, P, generator=gen)
    params = p0.to(DEV)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step = torch.zeros(n, dtype=torch.int32, device=DEV)
    sh = torch.full((n, -(-P // 256) * 256), float("nan"), dtype=torch.bfloat16, device=DEV) if shadow else None
    store = torch.zeros(n * P + n + 1, device=DEV)
    buf = store[1:] if offset_grad else store[:-1]
    assert (buf.data_ptr() - params.data_ptr()) % 16 == (4 if offset_grad else 0)
    return gen, p0, params, m, v, step, sh, buf


# ----------------------------------------------------------------------------------------
# 1. exact decay read-out, the flat optimizer

@pytest.mark.parametrize("sched", ["plain", "ramp"])
@pytest.mark.parametrize("n,P,kw", FLAT_ARGS, ids=FLAT_IDS)
def test_flat_optimizer_zero_gradient_is_the_decay_products(n, P, kw, sched):
    """All-zero gradients: after 8 steps p is bitwise p0 * d_0 * ... * d_7 formed step by step on
    the host, m and v exactly 0 -- eager, and as one captured step replayed 8 times (the kernel
    reads the step counter, and under the ramp the rate, on the device: no recapture)."""
    cfg = FLAT_OPTS[sched]
    steps = 8
    res = {}
    for mode in ("eager", "graph"):
        _, p0, params, m, v, step, sh, buf = _flat_buffers(n, P, **kw)
        run = lambda *t: flat_optimizer_step(*(t or (params, m, v, step)), buf, cfg, shadow=sh)  # noqa: E731
        if mode == "graph":
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):  # warm-up outside the capture on untouched copies
                run(params.clone(), m.clone(), v.clone(), step.clone())
            torch.cuda.current_stream().wait_stream(s)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                run()
            for _ in range(steps):
                gr.replay()
        else:
            for _ in range(steps):
                run()
        torch.cuda.synchronize()
        assert step.tolist() == [steps] * n
        assert not m.any() and not v.any()
        if sh is not None:
            assert torch.equal(sh[:, :P], params.to(torch.bfloat16))
        res[mode] = params.cpu()
        assert torch.equal(res[mode], A.decay_products(p0, cfg, steps)), mode
    assert torch.equal(res["eager"], res["graph"])
    assert not torch.equal(res["eager"], p0)


# ----------------------------------------------------------------------------------------
# 2. exact decay read-out, the fused families and the layer-split stages

# id -> (batch, EngineConfig keywords, OptimConfig keywords, (lanes, groups), variant)
ZERO_CELLS = {**{f: (v[0], v[1], {}, v[3], 0) for f, v in C.FAMILIES.items()},
              "lanes4-clip": (64, {}, dict(max_grad_norm=1.0), (4, 1), 1),
              "grp4-clip": (256, dict(groups="on"), dict(max_grad_norm=1.0), (4, 4), 1),
              "lanes4-accum2": (64, dict(accumulate=2), {}, (4, 1), 2),
              "lanes4-bf16": (64, dict(precision="bf16"), {}, (4, 1), 0)}


def _variant(tr) -> int:
    rec = nat.StepPick()
    assert nat.load().dtp_train_engine_pick(tr._engine_handle(), ctypes.byref(rec)) == 0
    return rec.variant


@pytest.mark.parametrize("sched", ["plain", "ramp"])
@pytest.mark.parametrize("cell", list(ZERO_CELLS))
def test_fused_step_zero_gradient_is_the_decay(cell, sched):
    """Targets 0.5 and a last layer of W = 0, b = 0.5: the first step's gradient is exactly zero
    (fp32 and bf16), so after one step params == p0 * d_0 bitwise, m == v == 0 and the logged
    loss is 0.  Under the ramp d_0 = (float)(1 - (1e-2 / 12) 0.5): a decay formed from the base
    rate fails.  The clip twins see a zero norm (coefficient 1), the accumulation twin sums two
    zero gradients."""
    batch, ekw, okw, inst, variant = ZERO_CELLS[cell]
    cfg = dataclasses.replace(FLAT_OPTS[sched], **okw)
    X, Y, init = A.zero_gradient_problem()
    tr = FusedTrainer(TOY_SPEC, 2, X.to(DEV), Y.to(DEV), SamplerGeometry(n=512, batch=batch, seed=11), cfg,
                      EngineConfig(steps_per_launch=5, **ekw), init_params=[p.to(DEV) for p in init])
    try:
        assert (tr.lanes, tr.groups) == inst, (tr.lanes, tr.groups)
        assert _variant(tr) == variant
        tr.train(1)
        tr.synchronize()
        assert tr.step_ctr.tolist() == [1, 1]
        assert tr.losses(0, 1).abs().max().item() == 0.0
        assert not tr.m.any() and not tr.v.any()
        assert torch.equal(tr.params.cpu(), A.decay_products(torch.stack(init), cfg, 1))
    finally:
        tr.close()


SPLIT_ZERO = [(0, 2, "auto", None), (0, 5, "auto", None), ("auto", 2, "auto", 4), (0, 2, "remote", None)]


@pytest.mark.parametrize("sched", ["plain", "ramp"])
@pytest.mark.parametrize("members,K,links,want", SPLIT_ZERO, ids=[f"m{m}-K{K}-{l}" for m, K, l, _ in SPLIT_ZERO])
def test_layer_split_zero_gradient_is_the_decay(members, K, links, want, sched):
    """The one-workgroup stages (split_train.hip: K = 2 the pipelined multi-layer kernel, K = 5
    the one-layer one), the split-batch stages (split_lanes.hip, four members) and remote links."""
    cfg = FLAT_OPTS[sched]
    X, Y, init = A.zero_gradient_problem(n=1)
    eng = FusedLayerSplit(TOY_SPEC, [DEV] * K, X, Y, SamplerGeometry(n=512, batch=256, seed=11), cfg, init[0],
                          members=members, links=links)
    try:
        if want is not None:
            assert eng.members == want
        else:
            assert not eng.members
        eng.train(1)
        eng.synchronize()
        assert [int(s.item()) for s in eng.step] == [1] * K
        assert eng.losses(0, 1).abs().max().item() == 0.0
        assert torch.equal(eng.flat_params_cpu(), A.decay_products(init[0], cfg, 1))
        sd = eng.state_dict()
        assert not sd["m"].any() and not sd["v"].any()
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------
# 3. trajectories against fp64 autograd + torch.optim.AdamW

@pytest.mark.parametrize("sched", ["plain", "ramp"])
@pytest.mark.parametrize("n,P,kw", FLAT_ARGS, ids=FLAT_IDS)
def test_flat_optimizer_matches_fp64_adamw(n, P, kw, sched):
    """12 steps on random gradients next to torch.optim.AdamW over double parameters (under the
    ramp: + LambdaLR), at the flat optimizer's tolerance."""
    cfg = FLAT_OPTS[sched]
    gen, p0, params, m, v, step, sh, buf = _flat_buffers(n, P, **kw)
    ps = [torch.nn.Parameter(p0[i].double()) for i in range(n)]
    opt, lam = C.torch_optimizer(cfg, ps)
    assert type(opt) is torch.optim.AdamW
    for _ in range(A.STEPS):
        g = torch.randn(n, P, generator=gen)
        for i in range(n):
            ps[i].grad = g[i].double()
        opt.step()
        if lam is not None:
            lam.step()
        buf[: n * P].copy_(g.reshape(-1))
        flat_optimizer_step(params, m, v, step, buf, cfg, shadow=sh)
    assert step.tolist() == [A.STEPS] * n
    torch.testing.assert_close(params.cpu().double(), torch.stack([p.detach() for p in ps]), **A.FLAT_TOL)
    # the decay is in neither moment
    st = opt.state[ps[0]]
    torch.testing.assert_close(m[0].cpu().double(), st["exp_avg"], **A.FLAT_TOL)
    torch.testing.assert_close(v[0].cpu().double(), st["exp_avg_sq"], **A.FLAT_TOL)


def _trainer(loss, batch, ekw, cfg, launch="persistent", spl=5, inst=None):
    spec = A.CE_SPEC if loss == "ce" else TOY_SPEC
    X, Y = A._data(loss).device_tensors(DEV)
    tr = FusedTrainer(spec, 2, X, Y, SamplerGeometry(n=512, batch=batch, seed=11), cfg,
                      EngineConfig(launch=launch, steps_per_launch=spl, loss=loss, **ekw),
                      init_params=[p.to(DEV) for p in A._init(spec)])
    if inst is not None:
        assert (tr.lanes, tr.groups) == inst, (tr.lanes, tr.groups)
    return tr


def _run(tr, steps):
    try:
        tr.train(steps)
        tr.synchronize()
        assert tr.step_ctr.tolist() == [steps] * 2
        return tr.params.cpu(), tr.m.cpu(), tr.v.cpu(), tr.losses(0, steps)
    finally:
        tr.close()


@pytest.mark.parametrize("sched", ["adamw", "ramp"])
@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_fused_step_matches_fp64_adamw(family, sched):
    batch, ekw, _, inst, tol = C.FAMILIES[family]
    p, _, _, l = _run(_trainer("mse", batch, ekw, A.CONFIGS[sched], inst=inst), A.STEPS)
    rp, rl = A.reference("mse", batch, sched)
    print(f"max |dl| {(l - rl).abs().max().item():.3e}  max |dp| {(p - rp).abs().max().item():.3e}")
    torch.testing.assert_close(l, rl, **A.LOSS_TOL)
    torch.testing.assert_close(p, rp, **tol)


@pytest.mark.parametrize("sched", ["adamw", "ramp"])
@pytest.mark.parametrize("batch,ekw,inst", [(64, {}, (4, 1)), (256, dict(groups="on"), (4, 4))], ids=["b64", "b256-on"])
def test_fused_step_cross_entropy_matches_fp64_adamw(batch, ekw, inst, sched):
    p, _, _, l = _run(_trainer("ce", batch, ekw, A.CONFIGS[sched], inst=inst), A.STEPS)
    rp, rl = A.reference("ce", batch, sched)
    torch.testing.assert_close(l, rl, **A.LOSS_TOL)
    torch.testing.assert_close(p, rp, **A.PARAM_TOL_LOOSE)


@pytest.mark.parametrize("sched", ["adamw", "ramp"])
@pytest.mark.parametrize("batch,ekw,inst", [(256, dict(groups="off"), (1, 1)), (64, {}, (4, 1))], ids=["fast", "lanes4"])
def test_bf16_fused_step_matches_fp64_adamw(batch, ekw, inst, sched):
    """Against autograd through the bf16 rounding model, at tests/sched_cases.py's bf16 tolerances."""
    p, _, _, l = _run(_trainer("mse", batch, dict(precision="bf16", **ekw), A.CONFIGS[sched], inst=inst), A.STEPS)
    rp, rl = A.reference("mse", batch, sched, bf16=True)
    torch.testing.assert_close(l, rl, **C.BF16_LOSS_TOL)
    torch.testing.assert_close(p, rp, **C.BF16_PARAM_TOL)


@pytest.mark.parametrize("sched", ["adamw", "ramp"])
@pytest.mark.parametrize("kind", ["clip", "accum2"])
def test_fused_twins_match_fp64_adamw(kind, sched):
    """The clip twin (max_grad_norm binds at every step: clipping does not see the decay, the
    decay does not see the clipping) and the accumulation twin (two batches per step: the decay
    and, under the ramp, its rate once per optimizer step) of the 4-lanes step, 12 steps on
    non-zero gradients against fp64 autograd + clip_grad_norm_ + torch.optim.AdamW."""
    cfg = A.CONFIGS[sched]
    ekw = {}
    if kind == "clip":
        cfg = dataclasses.replace(cfg, max_grad_norm=A.CLIP_NORM)
    else:
        ekw = dict(accumulate=2)
    tr = _trainer("mse", 64, ekw, cfg, inst=(4, 1))
    assert _variant(tr) == (1 if kind == "clip" else 2)
    p, _, _, l = _run(tr, A.STEPS)
    rp, rl, _ = A.reference_twin(kind, sched)
    print(f"max |dl| {(l - rl).abs().max().item():.3e}  max |dp| {(p - rp).abs().max().item():.3e}")
    torch.testing.assert_close(l, rl, **A.LOSS_TOL)
    torch.testing.assert_close(p, rp, **A.PARAM_TOL)


@functools.lru_cache(maxsize=None)
def _split_ref(sched):
    ds = ToyData(n=512, seed=3)
    geoms = [EpochIndexStream(SamplerGeometry(n=512, batch=256, seed=11))]
    cfg = A.CONFIGS[sched]
    train = torch_train if cfg.schedule is None else C.torch_train_sched
    p, l = train(TOY_SPEC, A._init(TOY_SPEC, n=1), ds.X, ds.Y, geoms, A.STEPS, cfg, "mse")
    return p[0], l[:, 0]


@pytest.mark.parametrize("sched", ["adamw", "ramp"])
@pytest.mark.parametrize("members,K", [(0, 2), (0, 5), ("auto", 2)], ids=["m0-K2", "m0-K5", "auto-K2"])
def test_layer_split_matches_unsplit_fp64_adamw(members, K, sched):
    ds = ToyData(n=512, seed=3)
    eng = FusedLayerSplit(TOY_SPEC, [DEV] * K, ds.X, ds.Y, SamplerGeometry(n=512, batch=256, seed=11),
                          A.CONFIGS[sched], A._init(TOY_SPEC, n=1)[0], members=members)
    try:
        if members == "auto":
            assert eng.members == 4
        eng.train(5)
        eng.train(A.STEPS - 5)
        eng.synchronize()
        p, l = eng.flat_params_cpu(), eng.losses(0, A.STEPS)
        assert [int(s.item()) for s in eng.step] == [A.STEPS] * K
    finally:
        eng.close()
    rp, rl = _split_ref(sched)
    torch.testing.assert_close(l, rl, **A.LOSS_TOL)
    torch.testing.assert_close(p, rp, **A.PARAM_TOL)


@pytest.mark.parametrize("sched", ["adamw", "ramp"])
def test_stage_backward_fused_with_optimizer_matches_fp64_adamw(sched):
    """The module engine's stage backward + flat optimizer in one launch (mlp_stage.hip): bitwise
    the two separate launches, and the same loop on a double twin under torch.optim.AdamW."""
    import copy

    from distributed_training_pytorch_amd.models.toy import ToyModel

    cfg = A.CONFIGS[sched]
    rec = {}
    ref, n0 = _train_flat(False, cfg, steps=A.STEPS, record=rec)
    got, n1 = _train_flat(True, cfg, steps=A.STEPS)
    assert n0 == 0 and n1 == A.STEPS
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    twin = copy.deepcopy(ToyModel().layers).double()
    torch.nn.utils.vector_to_parameters(rec["init"].double().view(-1), twin.parameters())
    opt, lam = C.torch_optimizer(cfg, list(twin.parameters()))
    assert type(opt) is torch.optim.AdamW
    for x, y in rec["xy"]:
        opt.zero_grad()
        torch.nn.functional.mse_loss(twin(x.double()), y.double()).backward()
        opt.step()
        if lam is not None:
            lam.step()
    want = torch.nn.utils.parameters_to_vector(twin.parameters()).detach()
    torch.testing.assert_close(got[0].view(-1).cpu().double(), want, **A.PARAM_TOL)
    # and the loop tells AdamW from coupled Adam with the same numbers
    coupled, _ = _train_flat(True, dataclasses.replace(cfg, decoupled_weight_decay=False), steps=A.STEPS)
    assert (A.share(got[0].view(1, -1).cpu(), coupled[0].view(1, -1).cpu(), **A.PARAM_TOL) >= 0.5).all()


def test_stage_backward_fused_with_optimizer_follows_the_ramp_across_graph_replays():
    """One iteration -- zero_grad, forward, the stage backward fused with the AdamW step -- captured
    once and replayed 12 times on fresh batches under the ramp: bitwise the 12 eager iterations.
    The kernel reads the step counter, and with it the step's rate and d_t, on the device."""
    from distributed_training_pytorch_amd.models.toy import ToyModel
    from distributed_training_pytorch_amd.ops.loss import mse_loss
    from distributed_training_pytorch_amd.ops.mlp import ParamBackwardFusion
    from distributed_training_pytorch_amd.ops.optim import FlatOptimizer
    from distributed_training_pytorch_amd.parallel.ddp import FlatDDP

    cfg = A.ADAMW_RAMP
    eager, taken = _train_flat(True, cfg, steps=A.STEPS)
    assert taken == A.STEPS
    torch.manual_seed(5)
    m = ToyModel().cuda()
    ddp = FlatDDP(m)
    opt = FlatOptimizer(ddp.flat_params, ddp.flat_grad, cfg)
    x, y = torch.zeros(200, 2, device="cuda"), torch.zeros(200, 1, device="cuda")
    fused = []

    def iteration():
        ddp.zero_grad()
        with ParamBackwardFusion() as fus:
            mse_loss(ddp(x), y).backward()
            pend = fus.take()
            fused.append(pend is not None)
            opt.step(zero_grad=True, fused=pend)

    state = [t.detach().clone() for t in (ddp.flat_params, opt.m, opt.v, opt.step_ctr, ddp.flat_grad)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture, then the state put back
        iteration()
    torch.cuda.current_stream().wait_stream(s)
    with torch.no_grad():
        for dst, src in zip((ddp.flat_params, opt.m, opt.v, opt.step_ctr, ddp.flat_grad), state):
            dst.copy_(src)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        iteration()
    assert all(fused)
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(A.STEPS):
        x.copy_(torch.randn(200, 2, device="cuda", generator=g))
        y.copy_(torch.randn(200, 1, device="cuda", generator=g))
        gr.replay()
    torch.cuda.synchronize()
    assert opt.step_ctr.tolist() == [A.STEPS]
    for a, b in zip(eager, (ddp.flat_params, opt.m, opt.v, opt.step_ctr, ddp.flat_grad)):
        assert torch.equal(a, b.detach())


# ----------------------------------------------------------------------------------------
# 4. weight_decay = 0 with the flag is Adam, to the bit

WD0_CELLS = [("fast", {}), ("generic", {}), ("lanes2", {}), ("lanes4", {}), ("grp4", {}), ("grp3", {}),
             ("lanes4", dict(max_grad_norm=0.5)), ("lanes4", dict(accumulate=2))]


@pytest.mark.parametrize("family,extra", WD0_CELLS, ids=[f"{f}{'-' + next(iter(e)) if e else ''}" for f, e in WD0_CELLS])
def test_weight_decay_zero_with_the_flag_is_adam(family, extra):
    batch, ekw, _, inst, _ = C.FAMILIES[family]
    ekw = dict(ekw, **{k: v for k, v in extra.items() if k == "accumulate"})
    okw = {k: v for k, v in extra.items() if k != "accumulate"}
    runs = [_run(_trainer("mse", batch, ekw, OptimConfig(name, A.LR, **okw), inst=inst), A.STEPS)
            for name in ("adamw", "adam")]
    assert torch.isfinite(runs[0][0]).all()
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_flat_optimizer_weight_decay_zero_with_the_flag_is_adam():
    res = []
    for name in ("adamw", "adam"):
        gen, p0, params, m, v, step, sh, buf = _flat_buffers(3, 20001)
        for _ in range(5):
            buf[: 3 * 20001].copy_(torch.randn(3, 20001, generator=gen).reshape(-1))
            flat_optimizer_step(params, m, v, step, buf, OptimConfig(name, A.LR))
        res.append((params.cpu(), m.cpu(), v.cpu()))
    for x, y in zip(*res):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------------------
# 5. launch modes

@pytest.mark.parametrize("family", ["fast", "lanes4", "grp4"])
def test_launch_modes_agree_bitwise(family):
    """Persistent, eager and graph launches, no schedule: the same bits."""
    batch, ekw, _, inst, _ = C.FAMILIES[family]
    res = {launch: _run(_trainer("mse", batch, ekw, A.ADAMW, launch=launch, spl=spl, inst=inst), A.STEPS)
           for launch, spl in (("persistent", 5), ("eager", 1), ("graph", 4))}
    for k in ("eager", "graph"):
        for x, y in zip(res["persistent"], res[k]):
            assert torch.equal(x, y), k


@pytest.mark.parametrize("family", ["fast", "lanes4", "grp4"])
def test_one_long_launch_equals_one_step_launches_under_the_ramp(family):
    """The ramp extended to 1100 entries (weight_decay 0.5: d_t runs from 0.9996 down to 0.54):
    one 1100-step persistent launch -- it crosses the 1024-row refill of the per-step rows -- is
    bitwise 1100 one-step launches, whose decay is the first step's of each launch."""
    batch, ekw, _, inst, _ = C.FAMILIES[family]
    cfg = dataclasses.replace(A.ADAMW_RAMP, schedule=A.ramp(1100))
    long = _run(_trainer("mse", batch, ekw, cfg, spl=1100, inst=inst), 1100)
    ones = _run(_trainer("mse", batch, ekw, cfg, spl=1, inst=inst), 1100)
    assert torch.isfinite(long[0]).all() and torch.isfinite(long[3]).all()
    for x, y in zip(long, ones):
        assert torch.equal(x, y)


@pytest.mark.parametrize("members", [0, "auto"], ids=["stages", "split-batch"])
def test_layer_split_long_launch_equals_short_launches_under_the_ramp(members):
    """kSplitAdamTab = 1024 rows per fill: one 1100-step launch against launches of 100."""
    cfg = dataclasses.replace(A.ADAMW_RAMP, schedule=A.ramp(1100))
    ds = ToyData(n=512, seed=3)
    out = []
    for chunk in (1100, 100):
        eng = FusedLayerSplit(TOY_SPEC, [DEV] * 2, ds.X, ds.Y, SamplerGeometry(n=512, batch=256, seed=11), cfg,
                              A._init(TOY_SPEC, n=1)[0], members=members)
        try:
            for _ in range(1100 // chunk):
                eng.train(chunk)
            eng.synchronize()
            out.append((eng.flat_params_cpu(), eng.losses(1100 - 64, 1100)))
        finally:
            eng.close()
    assert torch.isfinite(out[0][0]).all()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ----------------------------------------------------------------------------------------
# 6. two ranks sharing the GPU, and the RCCL path

@pytest.mark.parametrize("sched", ["adamw", "ramp"])
@pytest.mark.parametrize("comm", ["xgmi", "host"])
def test_two_ranks_adamw(comm, sched):
    """Per-rank batch 128 through the in-kernel exchange and the host all-reduce, against the
    2-rank fp64 reference: the decay does not see grad_scale = 1/2."""
    res = run_ranks(_rank_job, 2, (comm, TOY_SPEC, "mse", A.CONFIGS[sched], A.STEPS, 128), timeout=300)
    rp, rl = A.reference("mse", 128, sched, world=2)
    for r in range(2):
        p, l, used = res[r]
        assert used == comm
        torch.testing.assert_close(l, rl, **A.LOSS_TOL)
        torch.testing.assert_close(p, rp, **A.PARAM_TOL)
    assert torch.equal(res[0][0], res[1][0]), "replicas diverged"


@pytest.mark.parametrize("sched", ["adamw", "ramp"])
def test_rccl_path_adamw_single_rank(sched):
    """grad kernel -> all_reduce -> flat optimizer kernel."""
    res = run_ranks(_rank_job, 1, ("rccl", TOY_SPEC, "mse", A.CONFIGS[sched], A.STEPS, 128), timeout=300, backend="nccl")
    rp, rl = A.reference("mse", 128, sched)
    p, l, used = res[0]
    assert used == "rccl"
    torch.testing.assert_close(l, rl, **A.LOSS_TOL)
    torch.testing.assert_close(p, rp, **A.PARAM_TOL)


# ----------------------------------------------------------------------------------------
# 7. the C API's refusals, resume, the demos

def _last_error() -> str:
    return (nat.load().dtp_last_error() or b"").decode()


def test_c_api_refuses_decoupled_sgd():
    """Every C entry point that takes a DtpHyper: -1 and a message for decoupled_wd under SGD,
    nothing written."""
    lib = nat.require(DEV)
    sgd = OptimConfig("sgd", 1e-2, momentum=0.9, weight_decay=0.1)
    # the flat optimizer
    n, P = 2, 371
    _, p0, params, m, v, step, _, buf = _flat_buffers(n, P)
    hp = sgd.hyper(0.01, 1.0, DEV)
    hp.decoupled_wd = 1
    a = nat.OptArgs(nat.ptr(params), nat.ptr(m), nat.ptr(v), nat.ptr(step), nat.ptr(buf), None, 0, n, P, nat.MODE_SGD,
                    1.0, 0, hp, None, 0, 0.0, 0.0, None, None)
    assert lib.dtp_flat_optimizer(ctypes.byref(a), nat.stream_ptr()) == -1 and "decoupled" in _last_error()
    a.kind = nat.MODE_ADAM  # the same block under Adam launches
    assert lib.dtp_flat_optimizer(ctypes.byref(a), nat.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert step.tolist() == [1, 1]
    # the fused step: a launch, the pick and the engine
    tr = _trainer("mse", 64, {}, sgd, inst=(4, 1))
    try:
        key = TOY_SPEC.key[:4]
        before = [t.clone() for t in (tr.params, tr.m, tr.step_ctr)]
        for mode in (nat.MODE_SGD, nat.MODE_XGMI_SGD):
            ta = tr._train_args(1, nat.MODE_SGD, None)
            ta.hp.decoupled_wd = 1
            assert lib.dtp_mlp_train(ctypes.byref(ta), *key, mode, nat.stream_ptr()) == -1
            assert "decoupled" in _last_error()
            rec = nat.StepPick(9, 9, 9, 9)
            assert lib.dtp_mlp_train_pick(ctypes.byref(ta), *key, mode, ctypes.byref(rec)) != 0
            assert not lib.dtp_train_engine_create(ctypes.byref(ta), *key, mode)
        torch.cuda.synchronize()
        for x, y in zip(before, (tr.params, tr.m, tr.step_ctr)):
            assert torch.equal(x, y)
    finally:
        tr.close()
    # the layer-split launches (through split_check_stage): the engine's own argument blocks, the
    # flag set behind the config's back
    ds = ToyData(n=512, seed=3)
    for members, fn in ((0, lib.dtp_split_launch), ("auto", lib.dtp_split_lanes_launch)):
        eng = FusedLayerSplit(TOY_SPEC, [DEV] * 2, ds.X, ds.Y, SamplerGeometry(n=512, batch=256, seed=11), sgd,
                              A._init(TOY_SPEC, n=1)[0], members=members)
        try:
            before = eng.flat_params_cpu()
            for L in eng._launch.values():
                for j in range(L.n):
                    L.stage[j].hp.decoupled_wd = 1
                assert fn(ctypes.byref(L), nat.stream_ptr()) == -1 and "decoupled" in _last_error(), _last_error()
                for j in range(L.n):
                    L.stage[j].hp.decoupled_wd = 0
            eng.synchronize()
            assert torch.equal(eng.flat_params_cpu(), before) and [int(x.item()) for x in eng.step] == [0, 0]
        finally:
            eng.close()


@pytest.mark.parametrize("family", ["lanes4", "grp4"])
def test_resume_is_a_bitwise_continuation(family):
    batch, ekw, _, inst, _ = C.FAMILIES[family]
    cfg = A.ADAMW_RAMP
    whole = _run(_trainer("mse", batch, ekw, cfg, inst=inst), A.STEPS)
    a = _trainer("mse", batch, ekw, cfg, inst=inst)
    a.train(7)
    a.synchronize()
    sd = a.state_dict()
    a.close()
    assert sd["optim"]["decoupled_weight_decay"] is True
    b = _trainer("mse", batch, ekw, cfg, inst=inst)
    try:
        b.load_state_dict(sd)
        b.train(A.STEPS - 7)
        b.synchronize()
        assert torch.equal(b.params.cpu(), whole[0]) and torch.equal(b.m.cpu(), whole[1]) and torch.equal(b.v.cpu(), whole[2])
    finally:
        b.close()


def _demo(script, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, WANDB_MODE="disabled")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, script, "--iters", "40", "--log_every", "20", "--steps_per_launch", "20",
                        "--no_progress", "--seed", "11", "--optimizer", "adamw", "--weight_decay", "0.1", "--lr", "0.01",
                        *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    from .test_clip_cpu import _summary

    return _summary(r.stdout)


def test_demo_adamw_engines_agree():
    """demo.py --optimizer adamw --weight_decay 0.1 on the fused, module and stock engines and the
    layer-split demo on its fused engine (it trains demo.py's first model): the final losses
    agree as in the existing demo tests."""
    outs = {eng: _demo("demo.py", "--engine", eng) for eng in ("stock", "module", "fused")}
    for eng, s in outs.items():
        assert s["optimizer"] == "adamw" and s["engine"] == eng and s["iters"] == 40, s
    for eng in ("module", "fused"):
        for a, b in zip(outs["stock"]["final_loss"], outs[eng]["final_loss"]):
            assert abs(a - b) <= 1e-4 * abs(a) + 1e-6, outs
    split = _demo("demo_one_model_multi_gpu.py", "--allow_shared_gpu")
    assert split["engine"] == "split-fused" and split["optimizer"] == "adamw", split
    a = outs["stock"]["final_loss"][0]
    assert abs(a - split["final_loss"]) <= 1e-4 * abs(a) + 1e-6, (outs, split)


def test_demo_adamw_with_a_cosine_schedule():
    """--lr_schedule cosine on top: the fused engine (d_t from the schedule's device table) ends
    where the stock engine (torch.optim.AdamW + LambdaLR) ends."""
    flags = ("--lr_schedule", "cosine", "--warmup_iters", "5", "--lr_min_ratio", "0.1")
    cos = {eng: _demo("demo.py", "--engine", eng, *flags) for eng in ("stock", "fused")}
    assert cos["fused"]["engine"] == "fused" and cos["fused"]["lr_schedule"] == "cosine", cos
    for a, b in zip(cos["stock"]["final_loss"], cos["fused"]["final_loss"]):
        assert abs(a - b) <= 1e-4 * abs(a) + 1e-6, cos

"""Learning-rate schedules in every device code path that applies the rate: the one-lane /
lanes / split-batch fused steps (csrc/mlp_train_one.hip, csrc/mlp_train_lanes.hip), the flat optimizer and the stage backward
fused with it (csrc/optim.hip, csrc/mlp_stage.hip), the layer-split stages
(csrc/split_train.hip, csrc/split_lanes.hip).  The flat optimizer, the stage backward and the
layer-split stages read ``DtpHyper::lr_tab`` by the step counter they hold on the device; the
fused steps read the host-formed per-step rows (``ops.optim.adam_bias_table``), SGD by that
counter or the host's step number, Adam by the host's step number only.  Inputs, yardstick (fp64 autograd + torch.optim +
LambdaLR) and tolerances: tests/sched_cases.py; the condition that the yardstick tells every
schedule from the constant rate is checked on the CPU (tests/test_lr_schedule_cpu.py)."""
import dataclasses

import pytest
import torch

from distributed_training_pytorch_amd import _native as nat
from distributed_training_pytorch_amd.data.sampler import EpochIndexStream
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC
from distributed_training_pytorch_amd.ops.optim import flat_optimizer_step
from distributed_training_pytorch_amd.ops.schedule import LrSchedule
from distributed_training_pytorch_amd.parallel.layer_split import FusedLayerSplit

from . import sched_cases as C
from . import step_cases as SC
from .dist_utils import run_ranks
from .test_module_path_gpu import _train_flat

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _trainer(family, ocfg, launch="persistent", spl=5, precision="fp32", world=1, rank=0, comm="auto"):
    batch, kw, _, inst, _ = C.FAMILIES[family]
    X, Y = C.data().device_tensors(DEV)
    tr = FusedTrainer(TOY_SPEC, 2, X, Y, C.geom(batch, world, rank), ocfg,
                      EngineConfig(launch=launch, steps_per_launch=spl, precision=precision, comm=comm, **kw),
                      init_params=[p.to(DEV) for p in C.init(batch)])
    if world == 1:
        assert (tr.lanes, tr.groups) == inst, (tr.lanes, tr.groups)
    return tr


def _run(tr, steps, graphs=None):
    tr.train(steps)
    tr.synchronize()
    assert tr.step_ctr.tolist() == [steps] * 2
    if graphs is not None:  # the steps really ran as replays of captured graphs (or really did not)
        assert bool(tr._graphs) == graphs
    out = (tr.params.clone(), tr.m.clone(), tr.v.clone(), tr.losses(0, steps))
    tr.close()
    return out


# ----------------------------------------------------------------------------------------
# 1. no schedule = a constant schedule, bitwise

def _constants(b):
    return [None, LrSchedule.from_values([b.lr]), LrSchedule.make("constant", b.lr)]


BITWISE_CELLS = [(f, o, "fp32") for f, o in C.FAMILY_CELLS] + [("fast", "adam", "bf16")]


@pytest.mark.parametrize("family,opt,prec", BITWISE_CELLS, ids=[f"{f}-{o}-{p}" for f, o, p in BITWISE_CELLS])
def test_constant_schedule_is_no_schedule_bitwise(family, opt, prec):
    """from_values([lr]) and make("constant", lr) give bitwise the parameters, moments and
    losses of schedule=None: 12 steps in launches of 5 on every fused-step instance family."""
    b = C.base(opt)
    runs = [_run(_trainer(family, dataclasses.replace(b, schedule=s), precision=prec), C.STEPS) for s in _constants(b)]
    assert torch.isfinite(runs[0][0]).all()
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert torch.equal(x, y)


def _flat_steps(n, P, cfg, steps=C.STEPS, graph=False, seed=0):
    """``steps`` flat-optimizer steps on a fixed sequence of random gradients; graph: ONE step
    captured once and replayed, its gradient buffer refilled between replays."""
    gen = torch.Generator().manual_seed(1000 * n + P + seed)
    p0 = torch.randn(n, P, generator=gen)
    grads = [torch.randn(n, P, generator=gen) for _ in range(steps)]
    params = p0.to(DEV)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step = torch.zeros(n, dtype=torch.int32, device=DEV)
    buf = torch.zeros(n * P + n, device=DEV)
    gr = None
    if graph:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up outside the capture on untouched copies
            flat_optimizer_step(params.clone(), m.clone(), v.clone(), step.clone(), buf, cfg)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            flat_optimizer_step(params, m, v, step, buf, cfg)
    for g in grads:
        buf[: n * P].copy_(g.reshape(-1).to(DEV))
        if gr is not None:
            gr.replay()
        else:
            flat_optimizer_step(params, m, v, step, buf, cfg)
    torch.cuda.synchronize()
    assert step.tolist() == [steps] * n
    return (params.cpu(), m.cpu(), v.cpu()), p0, grads


@pytest.mark.parametrize("opt", ["adam", "sgd"])
@pytest.mark.parametrize("P", [371, 4097])
def test_flat_optimizer_constant_schedule_is_no_schedule_bitwise(P, opt):
    """One block per row (371) and several blocks with the follow-up counter launch (4097)."""
    b = C.base(opt)
    runs = [_flat_steps(2, P, dataclasses.replace(b, schedule=s))[0] for s in _constants(b)]
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert torch.equal(x, y)


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_stage_backward_fused_with_optimizer_constant_schedule_bitwise(opt):
    b = C.base(opt)
    runs = []
    for s in _constants(b):
        got, taken = _train_flat(True, dataclasses.replace(b, schedule=s), steps=6)
        assert taken == 6
        runs.append(got)
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            assert torch.equal(x, y)


# ----------------------------------------------------------------------------------------
# 2. launch modes agree, bitwise, with a schedule

# SGD at batch 64 held at the 5-entry table's last rate (1.2 lr = 0.06, momentum 0.9) diverges
# within 50 steps -- on the CPU engine too: the trajectory, not a kernel -- and NaNs compare
# unequal, so the table that ends mid-launch runs on the other four cells
MODE_CELLS = [(f, o, 1100) for f, o in (("fast", "adam"), ("generic", "sgd"), ("lanes4", "adam"), ("lanes4", "sgd"),
                                         ("grp4", "adam"))] + \
             [(f, o, 5) for f, o in (("fast", "adam"), ("generic", "sgd"), ("lanes4", "adam"), ("grp4", "adam"))]


@pytest.mark.parametrize("family,opt,n_tab", MODE_CELLS, ids=[f"{f}-{o}-tab{n}" for f, o, n in MODE_CELLS])
def test_launch_modes_agree_bitwise_under_a_schedule(family, opt, n_tab):
    """One persistent launch of 1100 steps (it crosses the kernels' 1024-entry refill), short
    persistent launches, per-step eager launches and hipGraph replays run bitwise the same
    schedule: the table is indexed by the device counter (eager, graph) and by the host's
    step number (persistent) alike.  The table's neighbouring entries never coincide; the
    5-entry table ends inside the first launch.  launch="graph" under a schedule: SGD runs 3
    replays of one captured graph of 8 one-step launches, which read their step number from the
    device counters, and a tail of 6 one-step launches; Adam, whose host-formed table is indexed
    by the host's step number only, runs all 30 as one-step launches -- for the Adam cells the
    graph leg is a second eager leg (asserted below), and the capture itself is refused
    (test_scheduled_adam_engine_refuses_a_launch_without_the_step_number)."""
    b = C.base(opt)
    cfg = dataclasses.replace(b, schedule=C.zigzag(b.lr, n_tab))
    res = {}
    for name, launch, spl, steps in [("long", "persistent", 1100, 1100), ("short", "persistent", 100, 1100),
                                     ("one", "persistent", 1100, 30), ("eager", "eager", 1, 30),
                                     ("graph", "graph", 8, 30)]:
        res[name] = _run(_trainer(family, cfg, launch=launch, spl=spl), steps,
                         graphs=launch == "graph" and opt == "sgd")
    assert torch.isfinite(res["long"][0]).all() and torch.isfinite(res["long"][3]).all()
    for x, y in zip(res["long"], res["short"]):
        assert torch.equal(x, y)
    for k in ("eager", "graph"):
        for x, y in zip(res["one"], res[k]):
            assert torch.equal(x, y), k
    # and the schedule is applied at all: not the run of the table's first entry alone
    flat = _run(_trainer(family, dataclasses.replace(b, schedule=C.zigzag(b.lr, 1)), spl=1100), 30)
    assert not torch.equal(flat[0], res["one"][0])


@pytest.mark.parametrize("family", ["fast", "grp4"])
def test_scheduled_adam_engine_refuses_a_launch_without_the_step_number(family):
    """The native executor itself refuses what the Adam instances cannot do -- a scheduled
    launch that reads its step number on the device, hence a graph capture -- instead of
    training at the fixed rate; nothing ran, and the engine still steps with the number."""
    b = C.base("adam")
    tr = _trainer(family, dataclasses.replace(b, schedule=C.zigzag(b.lr, 5)), launch="graph", spl=4)
    try:
        with pytest.raises(RuntimeError, match="learning-rate schedule"):
            tr._graph_launch(4)
        e = tr._engine_handle()
        with pytest.raises(RuntimeError, match="learning-rate schedule"):
            nat.check(tr._engine_run(e, 1, -1, nat.raw_stream(tr._dev_index)), "dtp_train_engine_run")
        tr.synchronize()
        assert tr.step_ctr.tolist() == [0, 0] and not tr._graphs
        tr.train(3)
        tr.synchronize()
        assert tr.step_ctr.tolist() == [3, 3]
    finally:
        tr.close()


# ----------------------------------------------------------------------------------------
# 3. trajectory against the yardstick

@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("family,opt", C.FAMILY_CELLS, ids=[f"{f}-{o}" for f, o in C.FAMILY_CELLS])
def test_fused_step_follows_the_scheduled_yardstick(family, opt, kind):
    """12 steps in launches of 5 against fp64 autograd + torch.optim + LambdaLR."""
    batch, tol = C.FAMILIES[family][0], C.FAMILIES[family][4]
    p, _, _, l = _run(_trainer(family, C.config(opt, kind)), C.STEPS)
    rp, rl = C.reference(batch, opt, kind)
    print(f"max |dl| {(l - rl).abs().max().item():.3e}  max |dp| {(p.cpu() - rp).abs().max().item():.3e}")
    torch.testing.assert_close(l, rl, **C.LOSS_TOL)
    torch.testing.assert_close(p.cpu(), rp, **tol)


@pytest.mark.parametrize("kind", C.KINDS)
def test_bf16_fused_step_follows_the_scheduled_yardstick(kind):
    """The bf16 cell of the bitwise check (one-lane FAST, Adam) against autograd through the bf16
    rounding model in fp64 + torch.optim + LambdaLR, at the tolerances tests/test_bf16_gpu.py
    uses against that model.  At these tolerances the yardstick itself tells a schedule from
    the constant rate on only 0.3 - 12 % of the parameters (constant 0.04 / 0.003, linear 0.12 /
    0.09, cosine 0.12 / 0.09, step 0.06 / 0.05 per model; at the fp32 one-lane tolerance the
    same reference gives 0.79 - 0.96), under the 25 % the fp32 cells are held to: this cell
    catches a gross error only.  The rate the bf16 instance applies is pinned step by step at
    the fp32 optimizer's own tolerance in test_the_rate_applied_at_each_step."""
    p, _, _, l = _run(_trainer("fast", C.config("adam", kind), precision="bf16"), C.STEPS)
    rp, rl = C.reference(256, "adam", kind, bf16=True)
    print(f"max |dl| {(l - rl).abs().max().item():.3e}  max |dp| {(p.cpu() - rp).abs().max().item():.3e}")
    torch.testing.assert_close(l, rl, **C.BF16_LOSS_TOL)
    torch.testing.assert_close(p.cpu(), rp, **C.BF16_PARAM_TOL)


# ----------------------------------------------------------------------------------------
# 4. the rate actually applied, step by step

def _applied(opt, sg, lr_t):
    """step_cases.applied_is_stored's formulas with lr_t in place of lr (rtol 1e-5 Adam,
    1e-6 SGD), per model."""
    out = []
    for i in range(2):
        p0, p1, m = sg.params_before[i].double(), sg.params_after[i].double(), sg.grad[i].double()
        if opt == "sgd":
            pred = p0 - lr_t * m
            bad = (p1 - pred).abs() > 1e-6 * pred.abs() + 1e-7 * lr_t * m.abs()
        else:
            b2, eps = SC.ADAM.betas[1], SC.ADAM.eps
            bc2 = 1.0 - b2 ** (sg.t + 1)
            pred = -lr_t * m / ((1.0 - b2) ** 0.5 * m.abs() / bc2 ** 0.5 + eps)
            bad = ((p1 - p0) - pred).abs() > 1e-5 * pred.abs() + 4 * SC.U * torch.maximum(p0.abs(), p1.abs())
        if bad.any():
            out.append(f"t={sg.t} model {i}: the step is not lr_t = {lr_t:.6g} x the gradient read out "
                       f"at {int(bad.sum())} elements")
    return out


@pytest.mark.parametrize("family,opt,prec", [("fast", "adam", "fp32"), ("generic", "sgd", "fp32"),
                                             ("lanes2", "adam", "fp32"), ("lanes4", "sgd", "fp32"),
                                             ("grp4", "adam", "fp32"), ("grp3", "sgd", "fp32"),
                                             ("fast", "adam", "bf16")], ids=lambda v: str(v))
def test_the_rate_applied_at_each_step(family, opt, prec):
    """Zeroed-moment read-out (Adam betas = (0, 0.999); SGD with momentum): the parameter
    change of step t is lr_t x the gradient the step formed.  t = 0, W - 1, W, 4, N - 1, N, N + 3
    of a warm-up + linear decay whose neighbouring entries differ by >= 5 % (W = 3, N = 10,
    r = 0.1: steps of 12.9 % of lr).  The steps between the read-outs run in launches of up to
    4; every read-out step is a one-step launch of its own (step_cases.step_gradient), so it
    reads the first entry of a table window filled for step t.  The bf16 cell: the optimizer is
    fp32 there too, so the same formulas hold at the same tolerance."""
    b = SC.ADAM if opt == "adam" else SC.SGD
    sched = LrSchedule.make("linear", b.lr, warmup_iters=C.W, decay_iters=C.N, min_ratio=C.R)
    cfg = dataclasses.replace(b, schedule=sched)
    v = sched.values
    assert all(abs(v[i + 1] - v[i]) >= 0.05 * max(v[i], v[i + 1]) for i in range(len(v) - 1) if i != C.W - 1)
    tr = _trainer(family, cfg, spl=4, precision=prec)
    fails = []
    try:
        for t in (0, C.W - 1, C.W, 4, C.N - 1, C.N, C.N + 3):
            if tr.t < t:
                tr.train(t - tr.t)
            sg = SC.step_gradient(tr)
            assert sg.t == t
            fails += _applied(opt, sg, sched.lr(t))
            for u in (t - 1, t + 1):  # an index off by one (where the neighbour differs by >= 5 %)
                if 0 <= u and abs(sched.lr(u) - sched.lr(t)) >= 0.05 * sched.lr(t):
                    assert _applied(opt, sg, sched.lr(u)), (t, u)
    finally:
        tr.close()
    assert not fails, fails


@pytest.mark.parametrize("family,opt", [("lanes4", "adam"), ("generic", "sgd")], ids=lambda v: str(v))
def test_the_rate_applied_at_steps_1023_and_1024(family, opt):
    """The rows of steps 1023 and 1024 of the explicit table lr (1 + 0.1 ((3 t mod 7) - 3)), whose
    neighbours differ by >= 5 %, after one launch of 1023 steps.  Each read-out is a one-step
    launch (step_cases.step_gradient) whose prologue loads the window that starts at its step: it
    pins the table's indexing at these step numbers, not the in-launch refill.  The refill is
    pinned by test_launch_modes_agree_bitwise_under_a_schedule: one launch of 1100 steps, which
    refills at step 1024, equals bitwise eleven launches of 100, which never refill and whose
    windows all come from the prologue load read out here."""
    b = SC.ADAM if opt == "adam" else SC.SGD
    sched = C.zigzag(b.lr, 1100)
    cfg = dataclasses.replace(b, schedule=sched)
    v = sched.values
    assert all(abs(v[i + 1] - v[i]) >= 0.05 * max(v[i], v[i + 1]) for i in range(len(v) - 1))
    tr = _trainer(family, cfg, spl=1100)
    fails = []
    try:
        tr.train(1023)
        for t in (1023, 1024):
            sg = SC.step_gradient(tr)
            assert sg.t == t and torch.isfinite(sg.grad).all()
            fails += _applied(opt, sg, sched.lr(t))
            for u in (t - 1, t + 1):
                assert _applied(opt, sg, sched.lr(u)), (t, u)
    finally:
        tr.close()
    assert not fails, fails


# ----------------------------------------------------------------------------------------
# 5. the flat optimizer

@pytest.mark.parametrize("opt", ["adam", "sgd"])
@pytest.mark.parametrize("P", [371, 4097])
def test_flat_optimizer_graph_replays_follow_the_schedule(P, opt):
    """A graph of ONE step captured once and replayed 12 times equals 12 eager steps bitwise
    (the rate comes from the table by the device counter, not from the captured arguments),
    and both match torch.optim + LambdaLR at the flat optimizer's tolerance."""
    cfg = C.config(opt, "cosine")
    eager, p0, grads = _flat_steps(2, P, cfg)
    replay, _, _ = _flat_steps(2, P, cfg, graph=True)
    for x, y in zip(eager, replay):
        assert torch.equal(x, y)
    qs = [torch.nn.Parameter(p0[i].double()) for i in range(2)]
    pairs = [C.torch_optimizer(cfg, [q]) for q in qs]
    for g in grads:
        for q, gi, (o, s) in zip(qs, g, pairs):
            q.grad = gi.double()
            o.step()
            s.step()
    ref = torch.stack([q.detach() for q in qs])
    torch.testing.assert_close(eager[0].double(), ref, **C.FLAT_TOL)
    plain, _, _ = _flat_steps(2, P, C.base(opt))
    assert not torch.equal(plain[0], eager[0])


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_fused_backward_route_equals_the_unfused_one_under_a_schedule(opt):
    """The stage backward + optimizer in one launch (mlp_stage.hip's OPT instance) and the
    two separate launches, 12 steps of a cosine schedule: bitwise; and not the constant rate's."""
    cfg = C.config(opt, "cosine")
    ref, n0 = _train_flat(False, cfg, steps=C.STEPS)
    got, n1 = _train_flat(True, cfg, steps=C.STEPS)
    assert n0 == 0 and n1 == C.STEPS
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    plain, _ = _train_flat(True, C.base(opt), steps=C.STEPS)
    assert not torch.equal(plain[0], got[0])


# ----------------------------------------------------------------------------------------
# 6. engines

@pytest.mark.parametrize("family,opt", [("lanes4", "adam"), ("grp4", "sgd")], ids=lambda v: str(v))
def test_resume_continues_the_curve(family, opt):
    """7 steps, state_dict, a fresh trainer, 5 more steps = 12 steps, bitwise: the schedule is
    a function of the restored step counter."""
    cfg = C.config(opt, "cosine")
    whole = _run(_trainer(family, cfg), C.STEPS)
    a = _trainer(family, cfg)
    a.train(7)
    a.synchronize()
    sd = a.state_dict()
    a.close()
    b = _trainer(family, cfg)
    b.load_state_dict(sd)
    b.train(5)
    b.synchronize()
    assert b.step_ctr.tolist() == [C.STEPS] * 2
    assert torch.equal(b.params, whole[0]) and torch.equal(b.m, whole[1]) and torch.equal(b.v, whole[2])
    b.close()


def _two_rank_job(rank, world, opt, kind):
    torch.cuda.set_device(DEV)
    tr = _trainer("lanes2", C.config(opt, kind), spl=4, world=world, rank=rank, comm="xgmi")
    tr.train(C.STEPS)
    tr.synchronize()
    out = (tr.params.cpu(), tr.losses(0, C.STEPS), tr.comm)
    tr.close()
    return out


@pytest.mark.parametrize("opt,kind", [("adam", "cosine"), ("sgd", "step")])
def test_two_ranks_over_xgmi_follow_the_schedule(opt, kind):
    """Two ranks of per-rank batch 128 sharing the GPU through the in-kernel exchange, against
    the two-geometry yardstick."""
    res = run_ranks(_two_rank_job, 2, (opt, kind), timeout=300)
    rp, rl = C.reference(128, opt, kind, world=2)
    for r in range(2):
        p, l, used = res[r]
        assert used == "xgmi", f"rank {r} fell back to {used}"
        torch.testing.assert_close(l, rl, **C.LOSS_TOL)
        torch.testing.assert_close(p, rp, **C.PARAM_TOL)
    assert torch.equal(res[0][0], res[1][0]), "replicas diverged"
    far = C.share(rp, C.reference(128, opt, None, world=2)[0], **C.PARAM_TOL)
    assert (far >= 0.25).all(), far.tolist()


@pytest.mark.parametrize("members", [0, "auto"], ids=["stages", "split-batch"])
@pytest.mark.parametrize("opt,kind", [("adam", "cosine"), ("sgd", "linear")])
def test_layer_split_follows_the_schedule(opt, kind, members):
    """FusedLayerSplit, K = 2 (split_train.hip; members="auto": split_lanes.hip, four members
    per stage), 12 steps in two launches against the UNSPLIT scheduled yardstick."""
    cfg = C.config(opt, kind)
    ds = C.data()
    init = C.init(256, n=1)[0]
    eng = FusedLayerSplit(TOY_SPEC, [DEV] * 2, ds.X, ds.Y, C.geom(256), cfg, init, members=members)
    if members == "auto":
        assert eng.members == 4
    eng.train(5)
    eng.train(C.STEPS - 5)
    eng.synchronize()
    p, l = eng.flat_params_cpu(), eng.losses(0, C.STEPS)
    assert [int(s.item()) for s in eng.step] == [C.STEPS] * 2
    eng.close()
    geoms = [EpochIndexStream(C.geom(256))]
    rp, rl = C.torch_train_sched(TOY_SPEC, [init], ds.X, ds.Y, geoms, C.STEPS, cfg)
    cp, _ = C.torch_train_sched(TOY_SPEC, [init], ds.X, ds.Y, geoms, C.STEPS, C.base(opt))
    assert (C.share(rp, cp, **C.PARAM_TOL) >= 0.25).all()
    print(f"max |dl| {(l - rl[:, 0]).abs().max().item():.3e}  max |dp| {(p - rp[0]).abs().max().item():.3e}")
    torch.testing.assert_close(l, rl[:, 0], **C.LOSS_TOL)
    torch.testing.assert_close(p, rp[0], **C.PARAM_TOL)


# ----------------------------------------------------------------------------------------
# 6b. the Trainer: Lightning 1.5 configure_optimizers forms

@pytest.mark.parametrize("engine", ["module", "fused"])
@pytest.mark.parametrize("form", ["tuple-epoch", "dict-step"])
def test_trainer_scheduler_forms_match_the_torch_loop(tmp_path, form, engine):
    """([Adam, Adam], [StepLR, StepLR]) at epoch interval and the dict form at step interval,
    on the module path (hipGraph replays of the flat optimizer kernel, which reads the
    tabulated rates by its step counter: the rate changes with no recapture) and on the fused
    engine (fused_spec), 3 epochs of 4 batches, against a plain torch loop on fp64 twins that
    steps the schedulers at the same points (tolerance: tests/test_clip_gpu.py's Trainer
    comparison).  After fit the real schedulers' get_last_lr() is the loop's."""
    import copy
    import os

    from distributed_training_pytorch_amd.trainer import Trainer

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rtol, atol = 1e-4, 2e-5
    torch.manual_seed(0)
    dl = torch.utils.data.DataLoader(ToyData(seed=0), batch_size=C.TRAINER_BATCH)
    model = C.lit_model(form, root)
    init = [copy.deepcopy(model.model_X.layers), copy.deepcopy(model.model_Y.layers)]
    want, last = C.trainer_torch_loop(init, dl, form)
    plain, _ = C.trainer_torch_loop(init, dl, form, scheduled=False)
    tr = Trainer(gpus=1, max_epochs=C.TRAINER_EPOCHS, accelerator="gpu", log_every_n_steps=1,
                 default_root_dir=str(tmp_path), enable_progress_bar=False, engine=engine)
    tr.fit(model, dl)
    assert tr.global_step == 12 and tr.engine_used == engine, tr.fused_refused
    tabs = tr.lr_tables
    assert tabs[0] is not None and tabs[0] == tabs[1] and len(set(tabs[0])) >= 3
    if engine == "module":
        assert all(f is not None and f.table == tabs[0] and f.host_t == 12 for f in tr._flat_opts)
        assert tr.graph_replays > 0  # the rate moved under replays of one capture
    for m, w, pl, s, ll in zip((model.model_X, model.model_Y), want, plain, model.scheds, last):
        got = torch.nn.utils.parameters_to_vector(m.layers.parameters()).detach().cpu().double()
        far = (w - pl).abs() > 10 * (atol + rtol * pl.abs())
        assert far.double().mean() >= 0.25, far.double().mean()
        torch.testing.assert_close(got, w, rtol=rtol, atol=atol)
        assert s.get_last_lr() == ll
    ck = torch.load(tr.checkpoint_path, map_location="cpu", weights_only=True)
    assert [st["_last_lr"] for st in ck["lr_schedulers"]] == last


def test_trainer_declines_the_fused_engine_when_the_tables_differ(tmp_path):
    """Two optimizers whose schedulers tabulate to different values: the fused engine has one
    OptimConfig, so the fit runs on the module path with a fused_refused reason."""
    import os

    from distributed_training_pytorch_amd.trainer import Trainer

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = type(C.lit_model("tuple-epoch", root))

    class Lit(base):
        def configure_optimizers(self):
            opts = [torch.optim.Adam(m.parameters(), lr=C.TRAINER_LR) for m in (self.model_X, self.model_Y)]
            return opts, [torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=g) for o, g in zip(opts, (0.5, 0.7))]

    torch.manual_seed(0)
    dl = torch.utils.data.DataLoader(ToyData(seed=0), batch_size=C.TRAINER_BATCH)
    tr = Trainer(gpus=1, max_epochs=2, accelerator="gpu", default_root_dir=str(tmp_path), enable_progress_bar=False,
                 enable_checkpointing=False)
    tr.fit(Lit(), dl)
    assert tr.engine_used == "module" and "tables differ" in (tr.fused_refused or "")
    assert tr.lr_tables[0] != tr.lr_tables[1] and all(f.table is not None for f in tr._flat_opts)

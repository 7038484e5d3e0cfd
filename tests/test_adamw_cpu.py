"""AdamW without a GPU: the config and its normalisation, the conditions on the inputs of the
GPU tests (fp64 torch alone), the CPU branch of flat_optimizer_step and the CPU fused engine
against torch.optim.AdamW, the CLI, and the demos on gloo ranks."""
import dataclasses
import sys

import pytest
import torch

from distributed_training_pytorch_amd.data.sampler import SamplerGeometry
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC
from distributed_training_pytorch_amd.ops.optim import OptimConfig, flat_optimizer_step

from . import adamw_cases as A
from .test_launchers_cpu import COMMON, PY, ROOT, _free_port, _run
from .test_clip_cpu import _summary


# ------------------------------------------------------------------------------ the config
def test_config_normalises_adamw_and_keeps_the_positional_forms():
    aw = OptimConfig("adamw")
    assert aw == OptimConfig("adam", decoupled_weight_decay=True)
    assert aw.name == "adam" and aw.decoupled_weight_decay is True and aw.label == "adamw"
    assert aw.kind == OptimConfig("adam").kind and aw != OptimConfig("adam")
    assert OptimConfig().label == "adam" and OptimConfig("sgd", 1e-2).label == "sgd"
    assert not OptimConfig().decoupled_weight_decay
    # the positional forms existing tests build and compare with ==
    assert OptimConfig("adam", 3e-3, (0.8, 0.95), 1e-4, 1e-2, 0.0) == OptimConfig(
        name="adam", lr=3e-3, betas=(0.8, 0.95), eps=1e-4, weight_decay=1e-2, momentum=0.0)
    assert OptimConfig("sgd", 5e-2, weight_decay=1e-2, momentum=0.9).name == "sgd"
    # the flag is the last field: every earlier positional argument keeps its place
    assert [f.name for f in dataclasses.fields(OptimConfig)][-1] == "decoupled_weight_decay"
    # dataclasses.replace keeps the flag
    assert dataclasses.replace(A.ADAMW, lr=1.0).decoupled_weight_decay


def test_sgd_has_no_decoupled_form():
    with pytest.raises(ValueError, match="decoupled"):
        OptimConfig("sgd", 1e-2, decoupled_weight_decay=True)


def test_torch_optimizer_and_hyper():
    p = [torch.nn.Parameter(torch.zeros(3))]
    opt = A.ADAMW.torch_optimizer(p)
    assert type(opt) is torch.optim.AdamW
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["betas"], g["eps"]) == (A.LR, A.WD, (0.9, 0.999), 1e-8)
    assert type(A.COUPLED.torch_optimizer(p)) is torch.optim.Adam
    assert A.ADAMW.hyper().decoupled_wd == 1
    assert A.COUPLED.hyper().decoupled_wd == 0 and OptimConfig("sgd", 1e-2).hyper().decoupled_wd == 0
    assert A.ADAMW.hyper().weight_decay == A.WD


def test_a_state_dict_without_the_key_loads_as_coupled():
    ds = A._data("mse")
    tr = FusedTrainer(TOY_SPEC, 2, ds.X, ds.Y, SamplerGeometry(n=512, batch=64, seed=11), A.ADAMW, EngineConfig(),
                      init_params=A._init(TOY_SPEC))
    sd = tr.state_dict()["optim"]
    assert sd["decoupled_weight_decay"] is True and sd["name"] == "adam"
    assert OptimConfig(**sd) == A.ADAMW
    old = {k: v for k, v in sd.items() if k != "decoupled_weight_decay"}  # a checkpoint from before the flag
    assert OptimConfig(**old) == A.COUPLED


# ------------------------------------------------------------------------------ conditions on the inputs
SHARE_CONFIGS = [("mse", 256, 1, A.PARAM_TOL_LOOSE), ("mse", 64, 1, A.PARAM_TOL), ("mse", 128, 2, A.PARAM_TOL),
                 ("mse", 128, 1, A.PARAM_TOL), ("mse", 130, 1, A.PARAM_TOL), ("ce", 64, 1, A.PARAM_TOL_LOOSE),
                 ("ce", 256, 1, A.PARAM_TOL_LOOSE)]


@pytest.mark.parametrize("loss,batch,world,tol", SHARE_CONFIGS, ids=[f"{l}-b{b}-w{w}" for l, b, w, _ in SHARE_CONFIGS])
def test_reference_tells_adamw_from_both_twins(loss, batch, world, tol):
    """A condition on the inputs, not a tolerance: after the 12 fp64 steps at least half of every
    model's parameters differ by more than 10x the loosest tolerance a GPU test compares that
    configuration at, from coupled Adam with the same weight_decay and from Adam without decay."""
    got = A.reference(loss, batch, "adamw", world)[0]
    for twin in ("coupled", "plain"):
        share = A.share(got, A.reference(loss, batch, twin, world)[0], tol["rtol"], tol["atol"])
        print(f"{twin}: share of parameters moved by > 10 tolerances: {share.tolist()}")
        assert (share >= 0.5).all(), (twin, share.tolist())


@pytest.mark.parametrize("loss,batch,tol", [("mse", 256, A.PARAM_TOL_LOOSE), ("mse", 64, A.PARAM_TOL),
                                            ("mse", 128, A.PARAM_TOL), ("mse", 130, A.PARAM_TOL)],
                         ids=["b256", "b64", "b128", "b130"])
def test_reference_tells_the_scheduled_decay_from_the_base_rate(loss, batch, tol):
    """Under the ramp with weight_decay = 0.5, a decay formed from the base rate (d as a launch
    constant) ends more than 10 tolerances away on at least half of the parameters."""
    got = A.reference(loss, batch, "ramp")[0]
    share = A.share(got, A.reference_base_rate_decay(loss, batch), tol["rtol"], tol["atol"])
    print(f"share of parameters moved by > 10 tolerances: {share.tolist()}")
    assert (share >= 0.5).all(), share.tolist()


@pytest.mark.parametrize("which", ["adamw", "ramp"])
def test_twin_references_clip_at_every_step_and_differ_from_the_plain_step(which):
    """Conditions on the twins' trajectory cells: CLIP_NORM binds at every step (the norm before
    clipping is at least twice it), and the accumulated run is not the one-batch run."""
    cp, _, norms = A.reference_twin("clip", which)
    assert (norms >= 2 * A.CLIP_NORM).all(), norms.min().item()
    ap, _, _ = A.reference_twin("accum2", which)
    plain = A.reference("mse", 64, which)[0]
    assert (A.share(ap, plain, **A.PARAM_TOL) >= 0.5).all()
    print("clip vs plain share", A.share(cp, plain, **A.PARAM_TOL).tolist())


# ------------------------------------------------------------------------------ the CPU update
@pytest.mark.parametrize("which", ["adamw", "ramp"])
def test_flat_optimizer_step_cpu_is_torch_adamw_step_by_step(which):
    """The CPU branch of flat_optimizer_step (adam_update_ref) next to fp32 torch.optim.AdamW on
    the same gradients, compared after every step; under the ramp the param group's lr is set
    to the table's value before each step."""
    cfg = A.CONFIGS[which]
    n, P = 3, 37
    gen = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, P, generator=gen)
    qs = [torch.nn.Parameter(p0[i].clone()) for i in range(n)]
    opt = dataclasses.replace(cfg, schedule=None).torch_optimizer(qs)
    assert type(opt) is torch.optim.AdamW
    params, m, v = p0.clone(), torch.zeros(n, P), torch.zeros(n, P)
    step = torch.zeros(n, dtype=torch.int32)
    for t in range(A.STEPS):
        g = torch.randn(n, P, generator=gen)
        for i in range(n):
            qs[i].grad = g[i].clone()
        for grp in opt.param_groups:
            grp["lr"] = cfg.lr_at(t)
        opt.step()
        flat_optimizer_step(params, m, v, step, torch.cat([g.reshape(-1), torch.zeros(n)]), cfg)
        torch.testing.assert_close(params, torch.stack([q.detach() for q in qs]), **A.FLAT_TOL)
        st = opt.state[qs[0]]
        torch.testing.assert_close(m[0], st["exp_avg"], **A.FLAT_TOL)   # the decay is in neither moment
        torch.testing.assert_close(v[0], st["exp_avg_sq"], **A.FLAT_TOL)
    assert step.tolist() == [A.STEPS] * n
    # the coupled form of the same numbers ends somewhere else
    cp, cm, cv = p0.clone(), torch.zeros(n, P), torch.zeros(n, P)
    cstep = torch.zeros(n, dtype=torch.int32)
    gen = torch.Generator().manual_seed(9)
    torch.randn(n, P, generator=gen)
    for t in range(A.STEPS):
        g = torch.randn(n, P, generator=gen)
        flat_optimizer_step(cp, cm, cv, cstep, torch.cat([g.reshape(-1), torch.zeros(n)]),
                            dataclasses.replace(cfg, decoupled_weight_decay=False))
    assert (A.share(params, cp, **A.FLAT_TOL) >= 0.5).all()


def test_weight_decay_zero_with_the_flag_is_adam_on_the_cpu():
    n, P = 2, 37
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, P, generator=gen)
    gs = [torch.randn(n, P, generator=gen) for _ in range(5)]
    res = []
    for cfg in (OptimConfig("adamw", A.LR), OptimConfig("adam", A.LR)):
        params, m, v = p0.clone(), torch.zeros(n, P), torch.zeros(n, P)
        step = torch.zeros(n, dtype=torch.int32)
        for g in gs:
            flat_optimizer_step(params, m, v, step, torch.cat([g.reshape(-1), torch.zeros(n)]), cfg)
        res.append((params, m, v))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("which", ["adamw", "ramp"])
def test_cpu_fused_trainer_follows_the_yardstick_and_resumes(which):
    """The CPU engine (FusedTrainer's reference step) against fp64 autograd + AdamW, and
    resume: 7 steps, state_dict, a fresh trainer, 5 more steps is the 12-step run bitwise."""
    ds = A._data("mse")
    cfg = A.CONFIGS[which]
    assert cfg.decoupled_weight_decay and cfg.name == "adam"
    assert type(cfg.torch_optimizer([torch.nn.Parameter(torch.zeros(1))])) is torch.optim.AdamW

    def make():
        return FusedTrainer(TOY_SPEC, 2, ds.X, ds.Y, SamplerGeometry(n=512, batch=64, seed=11), cfg, EngineConfig(),
                            init_params=A._init(TOY_SPEC))

    tr = make()
    tr.train(A.STEPS)
    rp, rl = A.reference("mse", 64, which)
    torch.testing.assert_close(tr.losses(0, A.STEPS), rl, **A.LOSS_TOL)
    torch.testing.assert_close(tr.params, rp, **A.PARAM_TOL)
    a = make()
    a.train(7)
    b = make()
    b.load_state_dict(a.state_dict())
    b.train(A.STEPS - 7)
    assert torch.equal(b.params, tr.params) and torch.equal(b.m, tr.m) and torch.equal(b.v, tr.v)


# ------------------------------------------------------------------------------ the CLI and the demos
def test_stock_summary_reports_what_ran():
    """The stock loop runs the verbatim Adam(lr=1e-3) pair unless the run asks for AdamW."""
    from distributed_training_pytorch_amd.baselines.stock import StockLoop
    from distributed_training_pytorch_amd.data.toy_data import ToyData

    plain = StockLoop(ToyData(seed=0), torch.device("cpu"), batch=128, seed=3, ddp=False)
    assert type(plain.ox) is torch.optim.Adam and plain.ox.param_groups[0]["lr"] == 1e-3
    aw = StockLoop(ToyData(seed=0), torch.device("cpu"), batch=128, seed=3, ddp=False, optim=A.ADAMW)
    assert type(aw.ox) is torch.optim.AdamW and type(aw.oy) is torch.optim.AdamW
    assert aw.ox.param_groups[0]["lr"] == A.LR and aw.ox.param_groups[0]["weight_decay"] == A.WD


def test_parser_and_runner_carry_adamw():
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    import argument_parser
    from distributed_training_pytorch_amd.engine import runner

    a = argument_parser.get_args([])
    assert a.optimizer == "adam" and a.weight_decay == 0.0
    assert not runner._optim(a).decoupled_weight_decay
    a = argument_parser.get_args(["--optimizer", "adamw", "--weight_decay", "0.1", "--lr_schedule", "cosine"])
    cfg = runner._optim(a)
    assert cfg.label == "adamw" and cfg.name == "adam" and cfg.weight_decay == 0.1 and cfg.schedule is not None
    with pytest.raises(SystemExit):
        argument_parser.get_args(["--optimizer", "adamax"])
    assert "0.01" in argument_parser.build_parser().format_help()  # torch's AdamW default, named in the help


def _torchrun(script, *args):
    r = _run([PY, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2", "--master-addr",
              "127.0.0.1", "--master-port", str(_free_port()), script, "--torchrun", *COMMON, *args])
    assert r.returncode == 0, r.stderr[-3000:]
    return _summary(r.stdout)


ADAMW_FLAGS = ["--optimizer", "adamw", "--weight_decay", "0.1", "--lr", "0.01"]


def test_demo_adamw_two_gloo_ranks_engines_agree():
    """demo.py --optimizer adamw --weight_decay 0.1 on two gloo ranks: the module and fused
    engines (flat_optimizer_step's CPU branch) end where the stock engine (torch DDP + two
    torch.optim.AdamW) ends, at the tolerance of the existing stock-against-fused comparison
    (tests/test_launchers_cpu.py); coupled Adam with the same flags does not."""
    outs = {eng: _torchrun("demo.py", "--engine", eng, *ADAMW_FLAGS) for eng in ("stock", "module", "fused")}
    for eng, s in outs.items():
        assert s["optimizer"] == "adamw" and s["engine"] == eng and s["iters"] == 20, s
    for eng in ("module", "fused"):
        for a, b in zip(outs["stock"]["final_loss"], outs[eng]["final_loss"]):
            assert abs(a - b) <= 1e-4 * abs(a) + 1e-6, outs
    coupled = _torchrun("demo.py", "--engine", "module", "--optimizer", "adam", "--weight_decay", "0.1", "--lr", "0.01")
    assert coupled["optimizer"] == "adam"
    for a, b in zip(outs["stock"]["final_loss"], coupled["final_loss"]):
        assert abs(a - b) > 10 * (1e-4 * abs(a) + 1e-6), (outs, coupled)


def test_layer_split_demo_adamw_cpu():
    """demo_one_model_multi_gpu.py on CPU (two stages per process, two gloo ranks, the autograd
    engine with one FlatOptimizer per stage): it trains one model, the first of demo.py's two
    (same seed, same init, same batches), so its final loss is that run's lossX."""
    split = _torchrun("demo_one_model_multi_gpu.py", *ADAMW_FLAGS)
    assert split["optimizer"] == "adamw" and split["engine"] == "split-module" and split["iters"] == 20, split
    whole = _torchrun("demo.py", "--engine", "stock", *ADAMW_FLAGS)
    a, b = whole["final_loss"][0], split["final_loss"]
    print(f"stock lossX {a}  layer split {b}")
    assert abs(a - b) <= 1e-4 * abs(a) + 1e-6, (whole, split)

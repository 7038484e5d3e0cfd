"""Adam betas / eps / weight decay (and SGD weight decay) through every device code path
that carries the optimizer update (csrc/optim_core.h: adam_update, sgd_update): the flat
optimizer's four branches, the one-lane / lanes / split-batch fused steps, the layer-split
stage kernels and the stage backward fused with the optimizer (tests/test_module_path_gpu.py),
each against fp64 autograd + torch.optim.  Two CPU tests: the reference itself tells every
hyperparameter case from its default twin by far more than the GPU tolerances (else a
kernel ignoring the hyperparameter would pass), and the Trainer's torch.optim -> OptimConfig
mapping."""
import functools

import pytest
import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream, SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC, MlpSpec
from distributed_training_pytorch_amd.ops.optim import OptimConfig, adam_bias_table, flat_optimizer_step

from .dist_utils import run_ranks
from .ref_train import torch_train
from .test_loss_optim_gpu import _rank_job
from .test_split_fused_gpu import _engine as _split_engine
from .test_split_fused_gpu import _reference as _split_reference

gpu = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CE_SPEC = MlpSpec(2, 10, 5, 4)
STEPS = 12

CASES = {
    "wd": OptimConfig(lr=1e-2, weight_decay=1e-2),
    "eps": OptimConfig(lr=1e-2, eps=1e-3),
    "betas": OptimConfig(lr=1e-2, betas=(0.5, 0.9)),
    "b1zero": OptimConfig(lr=1e-2, betas=(0.0, 0.99)),
    "all": OptimConfig(lr=1e-2, betas=(0.8, 0.95), eps=1e-4, weight_decay=1e-2),
    "near1": OptimConfig(lr=1e-2, betas=(0.5, 0.9999999)),
    "sgd_wd": OptimConfig("sgd", 5e-2, momentum=0.9, weight_decay=1e-2),
    # the default-hyperparameter twins (never run on the GPU here: the share condition only)
    "adam_default": OptimConfig(lr=1e-2),
    "sgd_default": OptimConfig("sgd", 5e-2, momentum=0.9),
}
# rows of the host-built Adam scalar table (ops/optim.py:adam_bias_table); the fused kernels
# hold kAdamTab = 1024 rows at a time, so "betas" and "all" end inside the first fill
TAB_ROWS = {"wd": 37413, "eps": 37413, "betas": 357, "b1zero": 3726, "all": 731, "near1": None}

LOSS_TOL = dict(rtol=1e-4, atol=1e-5)
PARAM_TOL = dict(rtol=1e-4, atol=2e-5)       # the lanes / split-batch / layer-split steps
PARAM_TOL_LOOSE = dict(rtol=1e-3, atol=3e-5)  # the one-lane step and cross-entropy


def _twin(case):
    return "sgd_default" if CASES[case].name == "sgd" else "adam_default"


def _init(spec, seed=100, n=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(spec.P, generator=g) * 0.4 for _ in range(n)]


def _data(loss):
    return ToyData(n=512, seed=3, classes=4 if loss == "ce" else 0)


@functools.lru_cache(maxsize=None)
def _fused_ref(spec, loss, batch, case, world=1):
    """fp64 autograd + torch.optim over the fused tests' set-up: (params [2, P], losses
    [STEPS, 2]).  Shared by every test of that configuration; never modified."""
    ds = _data(loss)
    geoms = [EpochIndexStream(SamplerGeometry(n=512, world=world, rank=r, batch=batch, seed=11)) for r in range(world)]
    return torch_train(spec, _init(spec), ds.X, ds.Y, geoms, STEPS, CASES[case], loss)


@functools.lru_cache(maxsize=None)
def _split_ref(case):
    """The layer-split tests' unsplit fp64 reference (its own data / init seeds)."""
    return _split_reference(CASES[case], STEPS)


# ----------------------------------------------------------------------------------------
# 0. CPU: the reference tells every case from its default twin

# (set-up, spec, loss, batch, world, case, loosest parameter tolerance a GPU test compares
# that configuration at) for every configuration the GPU tests below use; batch 256 also
# runs the one-lane step (groups="off"), for "all" only
SHARE_CONFIGS = (
    [("fused", TOY_SPEC, "mse", 256, 1, c, PARAM_TOL_LOOSE if c == "all" else PARAM_TOL)
     for c in ("wd", "eps", "betas", "all", "near1", "sgd_wd")]
    + [("fused", TOY_SPEC, "mse", 64, 1, c, PARAM_TOL) for c in ("wd", "eps", "betas", "all", "near1", "b1zero")]
    + [("fused", TOY_SPEC, "mse", 128, 1, "all", PARAM_TOL), ("fused", TOY_SPEC, "mse", 200, 1, "all", PARAM_TOL),
       ("fused", TOY_SPEC, "mse", 128, 2, "all", PARAM_TOL),
       ("fused", CE_SPEC, "ce", 64, 1, "all", PARAM_TOL_LOOSE), ("fused", CE_SPEC, "ce", 256, 1, "all", PARAM_TOL_LOOSE)]
    + [("split", TOY_SPEC, "mse", 256, 1, c, PARAM_TOL) for c in ("all", "betas", "sgd_wd")])


def _share(p_case, p_default, rtol, atol):
    """Per model: the share of parameters the case moved by more than 10 tolerances."""
    far = (p_case - p_default).abs() > 10 * (atol + rtol * p_default.abs())
    return far.double().mean(dim=-1)


@pytest.mark.parametrize("setup,spec,loss,batch,world,case,tol", SHARE_CONFIGS,
                         ids=[f"{s}-{l}-b{b}-w{w}-{c}" for s, _, l, b, w, c, _ in SHARE_CONFIGS])
def test_reference_tells_the_case_from_its_default_twin(setup, spec, loss, batch, world, case, tol):
    """A condition on the inputs, not a tolerance: after the 12 reference steps at least
    half of every model's parameters differ between the case and its default-hyperparameter
    twin (Adam(lr=1e-2); SGD with weight_decay=0) by more than 10x what the GPU comparison
    of that configuration allows, so a kernel that ignored the hyperparameter cannot pass.
    sgd_wd holds at the issue's weight_decay=1e-2 (no need to raise it)."""
    if setup == "split":
        got, ref = _split_ref(case)[0], _split_ref(_twin(case))[0]
    else:
        got, ref = _fused_ref(spec, loss, batch, case, world)[0], _fused_ref(spec, loss, batch, _twin(case), world)[0]
    share = _share(got, ref, tol["rtol"], tol["atol"])
    print(f"share of parameters moved by > 10 tolerances: {share.tolist()}")
    assert (share >= 0.5).all(), share.tolist()


def test_adam_table_rows_of_the_cases():
    """The table lengths the cases are chosen for: "betas" and "all" shorter than the
    kernels' 1024-row window, "near1" without a host table (the kernel's own f64 fill)."""
    for case, rows in TAB_ROWS.items():
        tab = adam_bias_table(CASES[case])
        assert (None if tab is None else tab.shape[0]) == rows, case
    # the search ends at the first power-of-two row count >= max_len: the default betas'
    # 37413 rows are found within 65536, not within 32768
    assert adam_bias_table(OptimConfig(), max_len=32768) is None
    assert adam_bias_table(OptimConfig(), max_len=65536).shape[0] == 37413


# ----------------------------------------------------------------------------------------
# 1. the flat optimizer kernel (csrc/optim.hip) against fp64 torch.optim

def _flat_run(n, P, case, shadow=False, offset_grad=False, grad_scale=1.0, zero_grad=False, log_cap=0,
              loss_scale=1.0, steps=8, seed=0):
    """``steps`` flat-optimizer steps on random gradients next to ``cfg.torch_optimizer``
    over double CPU parameters fed the same gradients x grad_scale.  offset_grad: the
    gradient buffer is a view one float into its allocation, so its rows sit at another
    16-byte phase than the parameter rows (the element-wise Adam branch).  Checks the
    shadow, loss ring and zero_grad contracts after every step; returns (params, m, v)."""
    cfg = CASES[case]
    gen = torch.Generator().manual_seed(1000 * n + P + seed)
    p0 = torch.randn(n, P, generator=gen)
    ps = [torch.nn.Parameter(p0[i].double()) for i in range(n)]
    opt = cfg.torch_optimizer(ps)
    params = p0.to(DEV)
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    step = torch.zeros(n, dtype=torch.int32, device=DEV)
    sh = torch.full((n, -(-P // 256) * 256), float("nan"), dtype=torch.bfloat16, device=DEV) if shadow else None
    log = torch.full((log_cap, n), -7.0, device=DEV) if log_cap else None
    store = torch.zeros(n * P + n + 1, device=DEV)
    buf = store[1:] if offset_grad else store[:-1]
    assert (buf.data_ptr() - params.data_ptr()) % 16 == (4 if offset_grad else 0)
    for t in range(steps):
        g = torch.randn(n, P, generator=gen)
        losses = torch.randn(n, generator=gen)
        for i in range(n):
            ps[i].grad = g[i].double() * grad_scale
        opt.step()
        buf.copy_(torch.cat([g.reshape(-1), losses]))
        before = None if log is None else log.clone()
        flat_optimizer_step(params, m, v, step, buf, cfg, grad_scale=grad_scale, loss_log=log, loss_scale=loss_scale,
                            shadow=sh, zero_grad=zero_grad)
        if zero_grad:
            assert not buf[:n * P].any()  # exactly zero, every row
        else:
            assert torch.equal(buf[:n * P].cpu(), g.reshape(-1))
        assert torch.equal(buf[n * P:].cpu(), losses)  # the loss slots are never written
        if log is not None:
            before[t % log_cap] = (losses * loss_scale).to(DEV)
            assert torch.equal(log, before), t  # slot t % cap of model i: loss_scale x its loss slot
        if shadow:
            assert torch.equal(sh[:, :P], params.to(torch.bfloat16))
            assert torch.isnan(sh[:, P:].float()).all()  # the row padding is never written
    assert step.tolist() == [steps] * n
    ref = torch.stack([p.detach() for p in ps])
    torch.testing.assert_close(params.cpu().double(), ref, rtol=1e-5, atol=1e-6)
    return params, m, v


FLAT_CASES = [
    # float4 body: head peels of 0-3 elements, rows shorter than a head, with the shadow
    ("f4-2x372", 2, 372, "all", {}), ("f4-2x372-shadow", 2, 372, "all", dict(shadow=True)),
    ("f4-4x371", 4, 371, "all", {}), ("f4-3x3", 3, 3, "all", {}),
    ("f4-4x371-b1zero", 4, 371, "b1zero", {}), ("f4-4x371-near1", 4, 371, "near1", {}),
    # bf16-pair branch: a shadow over rows of odd length
    ("pair-2x371", 2, 371, "all", dict(shadow=True)),
    # element-wise Adam branch: gradient rows at another 16-byte phase than the parameters
    ("elem-2x371", 2, 371, "all", dict(offset_grad=True)), ("elem-2x371-b1zero", 2, 371, "b1zero", dict(offset_grad=True)),
    # SGD branch
    ("sgd-2x371", 2, 371, "sgd_wd", {}), ("sgd-2x371-shadow", 2, 371, "sgd_wd", dict(shadow=True)),
    # launch shapes: several blocks per model (P > 4096), the grid-stride loop past the
    # 1024-block cap, and several blocks with more models than one wavefront has lanes
    ("blocks-3x20001", 3, 20001, "all", {}), ("blocks-3x20001-sgd", 3, 20001, "sgd_wd", {}),
    ("stride-1x270003", 1, 270003, "all", {}), ("models-65x4100", 65, 4100, "all", {}),
    # grad_scale (the DDP 1/W averaging) on every branch
    ("f4-4x371-gs", 4, 371, "all", dict(grad_scale=0.25)), ("pair-2x371-gs", 2, 371, "all", dict(shadow=True, grad_scale=0.25)),
    ("elem-2x371-gs", 2, 371, "all", dict(offset_grad=True, grad_scale=0.25)),
    ("sgd-2x371-gs", 2, 371, "sgd_wd", dict(grad_scale=0.25)),
    ("blocks-3x20001-gs", 3, 20001, "all", dict(grad_scale=0.25)),
]


@gpu
@pytest.mark.parametrize("n,P,case,kw", [c[1:] for c in FLAT_CASES], ids=[c[0] for c in FLAT_CASES])
def test_flat_optimizer_hyperparameters_match_fp64_torch(n, P, case, kw):
    """Every branch of flat_optimizer_kernel and every launch shape with non-default betas,
    eps and weight decay, 8 steps against fp64 torch.optim at the flat optimizer's
    tolerance (rtol 1e-5, atol 1e-6); every model's step counter ends at 8.  65 x 4100 is
    the multi-block launch with more than 64 models: the follow-up launch that advances
    the step counters has to reach all of them, or models 64.. keep the step-1 bias
    correction."""
    _flat_run(n, P, case, **kw)


@gpu
@pytest.mark.parametrize("n,P,case,kw", [(4, 371, "all", {}), (2, 371, "all", dict(shadow=True)),
                                         (2, 371, "all", dict(offset_grad=True)), (2, 371, "sgd_wd", {}),
                                         (3, 20001, "all", {})],
                         ids=["f4", "pair", "elem", "sgd", "blocks"])
def test_flat_optimizer_loss_ring_and_zero_grad(n, P, case, kw):
    """loss_log / loss_scale: a 3-slot ring over 8 steps, slot t % 3 of model i = 0.5 x the
    loss slot of step t, the other slots untouched.  zero_grad: the gradient rows are
    exactly zero afterwards, the loss slots are not touched, and parameters and moments
    are bitwise those of the run without the flag (all asserted per step in _flat_run)."""
    plain = _flat_run(n, P, case, grad_scale=0.25, log_cap=3, loss_scale=0.5, **kw)
    zeroed = _flat_run(n, P, case, grad_scale=0.25, log_cap=3, loss_scale=0.5, zero_grad=True, **kw)
    for a, b in zip(plain, zeroed):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------
# 2. the fused step (FusedTrainer) against fp64 torch_train

# (batch, groups) -> the (lanes, groups) instance it must run
INSTANCE = {(256, "off"): (1, 1), (128, "off"): (2, 1), (64, None): (4, 1), (256, "on"): (4, 4), (200, "on"): (4, 4)}


def _fused_trainer(spec, loss, batch, groups, case, launch="persistent", spl=5):
    X, Y = _data(loss).device_tensors(DEV)
    geom = SamplerGeometry(n=512, batch=batch, seed=11)
    kw = {} if groups is None else {"groups": groups}
    tr = FusedTrainer(spec, 2, X, Y, geom, CASES[case], EngineConfig(launch=launch, steps_per_launch=spl, loss=loss, **kw),
                      init_params=[p.to(DEV) for p in _init(spec)])
    assert (tr.lanes, tr.groups) == INSTANCE[(batch, groups)]
    return tr


def _check_fused(spec, loss, batch, groups, case, launch):
    tr = _fused_trainer(spec, loss, batch, groups, case, launch)
    if CASES[case].name == "adam":
        rows = None if tr._adam_tab is None else tr._adam_tab.shape[0]
        assert rows == TAB_ROWS[case]  # near1: None, the kernel's own f64 fill runs
    tr.train(STEPS)
    tr.synchronize()
    p, l = tr.params.cpu(), tr.losses(0, STEPS)
    assert tr.step_ctr.tolist() == [STEPS, STEPS]
    tr.close()
    rp, rl = _fused_ref(spec, loss, batch, case)
    print(f"max |dl| {(l - rl).abs().max().item():.3e}  max |dp| {(p - rp).abs().max().item():.3e}")
    torch.testing.assert_close(l, rl, **LOSS_TOL)
    one_lane = INSTANCE[(batch, groups)][0] == 1
    torch.testing.assert_close(p, rp, **(PARAM_TOL_LOOSE if loss == "ce" or one_lane else PARAM_TOL))


FUSED_CASES = (
    [(256, "off", "all", l) for l in ("persistent", "graph", "eager")]
    + [(128, "off", "all", "persistent")]
    + [(64, None, c, "persistent") for c in ("wd", "eps", "betas", "all", "near1")]
    + [(256, "on", c, "persistent") for c in ("wd", "eps", "betas", "all", "near1", "sgd_wd")]
    + [(256, "on", "all", l) for l in ("graph", "eager")]
    + [(200, "on", "all", "persistent")])


@gpu
@pytest.mark.parametrize("batch,groups,case,launch", FUSED_CASES,
                         ids=[f"b{b}-{g or 'auto'}-{c}-{l}" for b, g, c, l in FUSED_CASES])
def test_fused_step_hyperparameters_match_fp64_torch(batch, groups, case, launch):
    """The one-lane step (batch 256, groups off), the 2-lanes (128) and 4-lanes (64) steps
    and the split-batch step (256 / 200 over 4 members; 200 leaves a short last batch), 12
    steps in launches of 5, against fp64 autograd + torch.optim.  near1 (beta2 = 0.9999999)
    has no host table: the persistent kernel fills its Adam scalars itself."""
    _check_fused(TOY_SPEC, "mse", batch, groups, case, launch)


@gpu
@pytest.mark.parametrize("batch,groups", [(64, None), (256, "on")], ids=["b64", "b256-on"])
def test_fused_step_cross_entropy_hyperparameters_match_fp64_torch(batch, groups):
    _check_fused(CE_SPEC, "ce", batch, groups, "all", "persistent")


# ----------------------------------------------------------------------------------------
# 3. a host table shorter than the kernel's window: the clamp inside a launch

@gpu
@pytest.mark.parametrize("batch,groups", [(64, None), (256, "on")], ids=["b64", "b256-on"])
def test_short_host_adam_table_bitwise_equals_kernel_fill(batch, groups):
    """betas = (0.5, 0.9): 357 table rows, fewer than the 1024 the persistent kernel loads
    per fill, so the clamp to the last row acts inside the first prologue load; one
    1100-step launch starts below the table's end, crosses it and refills at step 1024.
    Bitwise the launch that forms the scalars itself in f64 (its first 12 steps are checked
    against fp64 torch.optim above)."""
    res = []
    for host in (True, False):
        tr = _fused_trainer(TOY_SPEC, "mse", batch, groups, "betas", spl=1100)
        assert tr._adam_tab is not None and tr._adam_tab.shape[0] < 1024
        if not host:
            tr._adam_tab = None
        tr.train(1100)
        tr.synchronize()
        res.append((tr.params.clone(), tr.losses(0, 1100)))
        assert tr.step_ctr.tolist() == [1100, 1100]
        tr.close()
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1]).all()
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


# ----------------------------------------------------------------------------------------
# 4. two ranks (MODE_XGMI_ADAM: grad_scale = 0.5 with weight decay) and the RCCL path

@gpu
@pytest.mark.parametrize("comm", ["xgmi", "host"])
def test_two_ranks_adam_hyperparameters(comm):
    """Two ranks of per-rank batch 128 sharing the GPU, through the in-kernel exchange and
    the host all-reduce: weight decay applies to the gradient averaged over the ranks
    (p * wd is added after the 1/W scaling, not scaled with it)."""
    res = run_ranks(_rank_job, 2, (comm, TOY_SPEC, "mse", CASES["all"], STEPS, 128), timeout=300)
    rp, rl = _fused_ref(TOY_SPEC, "mse", 128, "all", world=2)
    for r in range(2):
        p, l, used = res[r]
        assert used == comm
        torch.testing.assert_close(l, rl, **LOSS_TOL)
        torch.testing.assert_close(p, rp, **PARAM_TOL)
    assert torch.equal(res[0][0], res[1][0]), "replicas diverged"


@gpu
def test_rccl_path_adam_hyperparameters_single_rank():
    """grad kernel -> all_reduce -> flat optimizer kernel, with every Adam hyperparameter."""
    res = run_ranks(_rank_job, 1, ("rccl", TOY_SPEC, "mse", CASES["all"], STEPS, 128), timeout=300, backend="nccl")
    rp, rl = _fused_ref(TOY_SPEC, "mse", 128, "all")
    p, l, used = res[0]
    assert used == "rccl"
    torch.testing.assert_close(l, rl, **LOSS_TOL)
    torch.testing.assert_close(p, rp, **PARAM_TOL)


# ----------------------------------------------------------------------------------------
# 5. the layer-split engines (FusedLayerSplit) against the unsplit fp64 reference

SPLIT_CASES = ([(0, K, c) for K in (2, 5) for c in ("all", "betas", "sgd_wd")]
               + [("auto", K, c) for K in (2, 1) for c in ("all", "betas")])


@gpu
@pytest.mark.parametrize("members,K,case", SPLIT_CASES, ids=[f"m{m}-K{K}-{c}" for m, K, c in SPLIT_CASES])
def test_layer_split_hyperparameters_match_unsplit_fp64(members, K, case):
    """members=0: the one-workgroup stages (split_train.hip; K=2 the multi-layer pipelined
    stage kernel, K=5 the one-layer one); members="auto": the split-batch stages
    (split_lanes.hip), four 64-sample members per stage.  12 steps in two launches."""
    eng, _ = _split_engine(K, CASES[case], members=members)
    if members == "auto":
        assert eng.members == 4
    eng.train(5)
    eng.train(STEPS - 5)
    eng.synchronize()
    rp, rl = _split_ref(case)
    p, l = eng.flat_params_cpu(), eng.losses(0, STEPS)
    print(f"max |dl| {(l - rl).abs().max().item():.3e}  max |dp| {(p - rp).abs().max().item():.3e}")
    torch.testing.assert_close(l, rl, **LOSS_TOL)
    torch.testing.assert_close(p, rp, **PARAM_TOL)
    assert [int(s.item()) for s in eng.step] == [STEPS] * K
    eng.close()


# ----------------------------------------------------------------------------------------
# 7. CPU: the Trainer's torch.optim -> OptimConfig mapping

def test_trainer_optim_mapping_and_cpu_round_trip():
    """_optim_config maps a plain Adam / SGD's hyperparameters field for field, refuses
    what the flat kernel cannot run, and the mapped config through flat_optimizer_step
    (CPU path) is that torch.optim instance."""
    from distributed_training_pytorch_amd.trainer.trainer import _optim_config

    def ps(n=1):
        return [torch.nn.Parameter(torch.randn(7)) for _ in range(n)]

    adam = _optim_config(torch.optim.Adam(ps(), lr=3e-3, betas=(0.8, 0.95), eps=1e-4, weight_decay=1e-2))
    assert adam == OptimConfig("adam", 3e-3, (0.8, 0.95), 1e-4, 1e-2, 0.0)
    sgd = _optim_config(torch.optim.SGD(ps(), lr=5e-2, momentum=0.9, weight_decay=1e-2))
    assert sgd == OptimConfig("sgd", 5e-2, weight_decay=1e-2, momentum=0.9)
    a, b = ps(2)
    refused = {
        "amsgrad": torch.optim.Adam(ps(), lr=1e-3, amsgrad=True),
        "adamw": torch.optim.AdamW(ps(), lr=1e-3),
        "nesterov": torch.optim.SGD(ps(), lr=1e-2, momentum=0.9, nesterov=True),
        "dampening": torch.optim.SGD(ps(), lr=1e-2, momentum=0.9, dampening=0.1),
        "maximize-adam": torch.optim.Adam(ps(), lr=1e-3, maximize=True),
        "maximize-sgd": torch.optim.SGD(ps(), lr=1e-2, maximize=True),
        "two-groups-adam": torch.optim.Adam([{"params": [a]}, {"params": [b], "lr": 1e-2}], lr=1e-3),
        "two-groups-sgd": torch.optim.SGD([{"params": [a]}, {"params": [b], "lr": 1e-2}], lr=1e-3),
        "tensor-lr": torch.optim.Adam(ps(), lr=torch.tensor(1e-3)),
    }
    for name, opt in refused.items():
        assert _optim_config(opt) is None, name

    n, P = 3, 37
    gen = torch.Generator().manual_seed(9)
    for make in (lambda q: torch.optim.Adam(q, lr=3e-3, betas=(0.8, 0.95), eps=1e-4, weight_decay=1e-2),
                 lambda q: torch.optim.SGD(q, lr=5e-2, momentum=0.9, weight_decay=1e-2)):
        p0 = torch.randn(n, P, generator=gen)
        qs = [torch.nn.Parameter(p0[i].clone()) for i in range(n)]
        opt = make(qs)
        cfg = _optim_config(opt)
        params, m, v = p0.clone(), torch.zeros(n, P), torch.zeros(n, P)
        step = torch.zeros(n, dtype=torch.int32)
        for _ in range(5):
            g = torch.randn(n, P, generator=gen)
            for i in range(n):
                qs[i].grad = g[i].clone()
            opt.step()
            flat_optimizer_step(params, m, v, step, torch.cat([g.reshape(-1), torch.zeros(n)]), cfg)
        torch.testing.assert_close(params, torch.stack([q.detach() for q in qs]), rtol=1e-5, atol=1e-6)
        assert step.tolist() == [5] * n

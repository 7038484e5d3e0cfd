"""The several-lanes step's leaner loop edge (csrc/mlp_train_lanes.hip): the next-but-one sample's
permutation word travels raw across the loop's back edge -- and across launches and epochs --
and its -1 (a batch position past a ragged last batch) is formed at the gather a step later;
1 / (batch size [x OUT]) is divided once per launch for the full and for the ragged batch and
selected per step.  Against autograd + torch.optim in fp64 (the loop of tests/ref_train.py,
which here also returns the optimizer's moments) at the fp32 tolerances of
tests/test_grp_rows_gpu.py for losses and parameters and of tests/test_entrypoints_gpu.py
for the moments (GPU only).

Shapes: 448 samples are 1.75 batches of 256, 3.5 of 128, 7 of 64 -- so batch 256 (split over
4 workgroups, 64 samples each: the ragged batch of 192 leaves member 3 empty) and batch 128
(one workgroup, 2 lanes per sample: the ragged batch of 64 leaves half the lanes empty) end
every epoch in a short batch, and 7 steps cross 3 and 1 epoch ends; batch 64 (one workgroup,
4 lanes per sample) runs 7 full batches, one epoch to its very end, and with 416 samples
6 full batches and one of 32.  512 samples at batch 256 never see a short batch."""
import functools

import pytest
import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream, SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC, MlpSpec, mlp_forward_ref
from distributed_training_pytorch_amd.ops.optim import OptimConfig

from .ref_train import loss_fn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CE_SPEC = MlpSpec(2, 10, 5, 4)
OPTS = {"adam": OptimConfig(lr=1e-2), "sgd": OptimConfig("sgd", 5e-2, momentum=0.9, weight_decay=1e-4)}
# batch -> (groups setting, lanes per sample, workgroups per model)
INSTANCES = {256: ("on", 4, 4), 128: ("off", 2, 1), 64: ("off", 4, 1)}


def _spec(loss):
    return CE_SPEC if loss == "ce" else TOY_SPEC


def _init(spec):
    g = torch.Generator().manual_seed(1)  # the seed of tests/test_grp_rows_gpu.py
    return [torch.randn(spec.P, generator=g) * 0.4 for _ in range(2)]


def _data(n, loss):
    return ToyData(n=n, seed=21, classes=4 if loss == "ce" else 0)


def _geom(n, batch):
    return SamplerGeometry(n=n, batch=batch, seed=3)


@functools.lru_cache(maxsize=None)
def _reference(n, batch, steps, loss="mse", optim="adam"):
    """tests/ref_train.py:torch_train for one rank, keeping the optimizer's state: (params,
    losses [steps, 2], first moment / momentum buffer, second moment or None), computed once
    per configuration and shared (never modified)"""
    spec, ds = _spec(loss), _data(n, loss)
    X, Y = ds.X.detach().cpu().double(), ds.Y.detach().cpu()
    stream = EpochIndexStream(_geom(n, batch))
    params = [torch.nn.Parameter(p.double().clone()) for p in _init(spec)]
    opts = [OPTS[optim].torch_optimizer([p]) for p in params]
    losses = []
    for t in range(steps):
        idx = torch.tensor(stream.indices(t), dtype=torch.long)
        row = []
        for p, opt in zip(params, opts):
            q = p.detach().clone().requires_grad_(True)
            lo = loss_fn(mlp_forward_ref(q, spec, X[idx]), Y[idx].double() if loss == "mse" else Y[idx], loss)
            (p.grad,) = torch.autograd.grad(lo, q)
            opt.step()
            row.append(lo.item())
        losses.append(row)
    first = "exp_avg" if optim == "adam" else "momentum_buffer"
    m = torch.stack([o.state[p][first].float() for p, o in zip(params, opts)])
    v = torch.stack([o.state[p]["exp_avg_sq"].float() for p, o in zip(params, opts)]) if optim == "adam" else None
    return (torch.stack([p.detach().float() for p in params]), torch.tensor(losses, dtype=torch.float32), m, v)


def _run(n, batch, launches, loss="mse", optim="adam"):
    """(params, losses, opt_m, opt_v) after train(k) for every k of ``launches``"""
    spec = _spec(loss)
    groups, lanes, members = INSTANCES[batch]
    X, Y = _data(n, loss).device_tensors(DEV)
    tr = FusedTrainer(spec, 2, X, Y, _geom(n, batch), OPTS[optim],
                      EngineConfig(loss=loss, groups=groups, steps_per_launch=max(launches)),
                      init_params=[p.to(DEV) for p in _init(spec)])
    assert (tr.lanes, tr.kernel_waves, tr.groups) == (lanes, 4, members), tr.groups_refused
    for k in launches:
        tr.train(k)
    tr.synchronize()
    tr.check_comm()
    steps = sum(launches)
    assert tr.step_ctr.tolist() == [steps, steps]
    out = tr.params.cpu(), tr.losses(0, steps), tr.m.cpu(), tr.v.cpu()
    tr.close()
    return out


def _report(tag, got, ref):
    err = (got.double() - ref.double()).abs()
    print(f"{tag}: max abs err {err.max().item():.3e}, max rel err "
          f"{(err / ref.double().abs().clamp_min(1e-30)).max().item():.3e}")


def _check_fp32(got, ref):
    (p, l, m, v), (rp, rl, rm, rv) = got, ref
    for tag, g_, r_ in (("loss", l, rl), ("params", p, rp), ("opt_m", m, rm), ("opt_v", v, rv)):
        if r_ is not None:
            _report(tag, g_, r_)
    torch.testing.assert_close(l, rl, rtol=2e-4, atol=1e-5)
    torch.testing.assert_close(p, rp, rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(m, rm, rtol=1e-3, atol=1e-5)
    if rv is not None:
        torch.testing.assert_close(v, rv, rtol=1e-3, atol=1e-7)


SHAPES = [(448, 256), (448, 128), (448, 64), (416, 64)]


@pytest.mark.parametrize("n,batch", SHAPES)
def test_ragged_last_batch_across_epochs(n, batch):
    """7 steps in one launch: every step's loss (a ragged step's mean divides by the short
    batch's size), the parameters and both moments match the reference."""
    spe = -(-n // batch)
    assert _geom(n, batch).steps_per_epoch == spe
    assert [_geom(n, batch).batch_size_at(t) for t in (0, spe - 1)] == [batch, n - (spe - 1) * batch]
    _check_fp32(_run(n, batch, (7,)), _reference(n, batch, 7))


@pytest.mark.parametrize("n,batch", SHAPES)
def test_launch_split_same_bits(n, batch):
    """train(7), train(1) x 7 and train(3) + train(4) are the same bits: a launch's prologue
    forms the same index, validity and reciprocal that the loop carries over its back edge
    (launches begin in front of, on and behind a ragged batch and an epoch's end)."""
    whole = _run(n, batch, (7,))
    for launches in ((1,) * 7, (3, 4)):
        for tag, a, b in zip(("params", "loss", "opt_m", "opt_v"), _run(n, batch, launches), whole):
            assert torch.equal(a, b), (launches, tag)


@pytest.mark.parametrize("loss,optim", [("mse", "adam"), ("mse", "sgd"), ("ce", "adam"), ("ce", "sgd")])
def test_full_batches_only(loss, optim):
    """512 samples at batch 256, 5 steps on the split-batch instance: only the full batch's
    reciprocal is ever selected -- 1 / (256 OUT) under MSE, 1 / 256 under cross-entropy."""
    _check_fp32(_run(512, 256, (5,), loss, optim), _reference(512, 256, 5, loss, optim))

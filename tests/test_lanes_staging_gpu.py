"""The several-lanes step's per-step staged state (csrc/mlp_lanes.h, mlp_train_lanes.hip): the
per-wave staging areas of the dW tiles, the K-split accumulator pairs kept apart until the
park, and the final tiles parked while the last tile's MFMAs run.  What can go wrong is one
layer's staged rows aliasing another's, a tile parked before its last K-step, and a step
reading what the previous step staged for a sample slot that has no sample any more.

Every case runs 4 consecutive steps in ONE launch, on a dataset whose size leaves the epoch's
last batch ragged, so that the batch changes between steps (waves and sample slots valid in
step t are empty in step t + 1, and full again after it) and both batch-size reciprocals are
used.  Against autograd + torch.optim in fp64 (tests/ref_train.py) at the tolerances of
tests/test_lanes_gpu.py, and bitwise against 4 launches of 1 step (GPU only).

    instance      batch -> batches of the 4 steps (dataset size)
    split-batch   193 -> 193, 193, 57, 193 (443)    256 -> 256, 100, 256, 100 (356)
    4 lanes       1 -> 1, 1, 1, 1 (3)    17 -> 17, 17, 5, 17 (39)    64 -> 64, 23, 64, 23 (87)
    2 lanes       65 -> 65, 65, 9, 65 (139)    128 -> 128, 50, 128, 50 (178)
"""
import functools

import pytest
import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream, SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC, MlpSpec
from distributed_training_pytorch_amd.ops.optim import OptimConfig

from .ref_train import torch_train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CE_SPEC = MlpSpec(2, 10, 5, 4)
STEPS = 4
ADAM = OptimConfig(lr=1e-2)

# batch: (dataset size, groups setting, lanes, workgroups per model)
CASES = {193: (443, "on", 4, 4), 256: (356, "on", 4, 4),
         1: (3, "off", 4, 1), 17: (39, "off", 4, 1), 64: (87, "off", 4, 1),
         65: (139, "off", 2, 1), 128: (178, "off", 2, 1)}
PARAMS = [(b, loss) for b in CASES for loss in ("mse", "ce")]


def _spec(loss):
    return CE_SPEC if loss == "ce" else TOY_SPEC


def _init(spec):
    g = torch.Generator().manual_seed(1)
    return [torch.randn(spec.P, generator=g) * 0.4 for _ in range(2)]


def _data(batch, loss):
    return ToyData(n=CASES[batch][0], seed=21, classes=4 if loss == "ce" else 0)


def _geom(batch):
    return SamplerGeometry(n=CASES[batch][0], batch=batch, seed=3)


def _batches(batch):
    st = EpochIndexStream(_geom(batch))
    return [len(st.indices(t)) for t in range(STEPS)]


@functools.lru_cache(maxsize=None)
def _reference(batch, loss):
    """autograd + torch.optim in fp64, once per configuration, shared and never modified"""
    spec = _spec(loss)
    ds = _data(batch, loss)
    return torch_train(spec, _init(spec), ds.X, ds.Y, [EpochIndexStream(_geom(batch))], STEPS, ADAM, loss)


@functools.lru_cache(maxsize=None)
def _run(batch, loss, spl):
    """(params, m, v, losses) after 4 steps in launches of spl steps; shared, never modified"""
    n, groups, lanes, members = CASES[batch]
    spec = _spec(loss)
    X, Y = _data(batch, loss).device_tensors(DEV)
    tr = FusedTrainer(spec, 2, X, Y, _geom(batch), ADAM,
                      EngineConfig(loss=loss, groups=groups, steps_per_launch=spl),
                      init_params=[p.to(DEV) for p in _init(spec)])
    assert (tr.lanes, tr.kernel_waves, tr.groups) == (lanes, 4, members)
    tr.train(STEPS)
    tr.synchronize()
    tr.check_comm()
    assert tr.step_ctr.tolist() == [STEPS, STEPS]
    out = tr.params.cpu(), tr.m.cpu(), tr.v.cpu(), tr.losses(0, STEPS)
    tr.close()
    return out


def _report(tag, got, ref):
    err = (got.double() - ref.double()).abs()
    print(f"{tag}: max abs err {err.max().item():.3e}, max rel err "
          f"{(err / ref.double().abs().clamp_min(1e-30)).max().item():.3e}")


def test_batches_change_between_steps():
    """the cases are what the module's table says: every batch but 1 has a ragged step between
    full ones inside the 4 steps"""
    want = {193: [193, 193, 57, 193], 256: [256, 100, 256, 100], 1: [1, 1, 1, 1], 17: [17, 17, 5, 17],
            64: [64, 23, 64, 23], 65: [65, 65, 9, 65], 128: [128, 50, 128, 50]}
    assert {b: _batches(b) for b in CASES} == want


@pytest.mark.parametrize("batch,loss", PARAMS)
def test_four_steps_in_one_launch_match_torch(batch, loss):
    p, _, _, l = _run(batch, loss, STEPS)
    rp, rl = _reference(batch, loss)
    _report("loss", l, rl)
    _report("params", p, rp)
    torch.testing.assert_close(l, rl, rtol=2e-4, atol=1e-5)
    torch.testing.assert_close(p, rp, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("batch,loss", PARAMS)
def test_one_launch_of_four_steps_bitwise_equals_four_launches(batch, loss):
    """staged state that leaked across the step loop's back edge would show here: a launch of
    one step starts from freshly zeroed staging areas, the persistent launch's later steps
    from what the steps before them left"""
    one, four = _run(batch, loss, STEPS), _run(batch, loss, 1)
    for name, a, b in zip(("params", "opt_m", "opt_v", "loss"), one, four):
        assert torch.equal(a, b), name

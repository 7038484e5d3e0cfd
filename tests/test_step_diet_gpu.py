"""The split-batch step's leaner tail (csrc/grp_core.h, mlp_train_lanes.hip): exchange addresses
fixed per launch with the buffer parity as a scalar offset, member sums read from every
member's row alike, the weight scatter through per-launch LDS offsets, the loss log as a
running offset.  Against autograd + torch.optim (tests/ref_train.py) with the recipe and
the fp32 tolerances of tests/test_grp_rows_gpu.py (GPU only).

Every case: n = 512, 7 steps, groups="on".  No case provokes an exchange timeout; every run
asserts that check_comm() passes and that the step counters are right."""
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
STEPS = 7
ADAM = OptimConfig(lr=1e-2)


def _spec(loss):
    return CE_SPEC if loss == "ce" else TOY_SPEC


def _init(spec):
    # the seed of tests/test_grp_rows_gpu.py (plain fp32 autograd stays well inside the tolerances)
    g = torch.Generator().manual_seed(1)
    return [torch.randn(spec.P, generator=g) * 0.4 for _ in range(2)]


def _data(loss):
    return ToyData(n=512, seed=21, classes=4 if loss == "ce" else 0)


def _geom(batch):
    return SamplerGeometry(n=512, batch=batch, seed=3)


@functools.lru_cache(maxsize=None)
def _reference(batch, loss):
    """autograd + torch.optim, computed once per configuration and shared (never modified)"""
    spec = _spec(loss)
    ds = _data(loss)
    return torch_train(spec, _init(spec), ds.X, ds.Y, [EpochIndexStream(_geom(batch))], STEPS, ADAM, loss)


def _run(batch, groups, loss="mse", spl=3, **ecfg):
    """(params, losses of the 7 steps, the raw loss ring) after 7 steps"""
    spec = _spec(loss)
    X, Y = _data(loss).device_tensors(DEV)
    tr = FusedTrainer(spec, 2, X, Y, _geom(batch), ADAM,
                      EngineConfig(loss=loss, groups="on", steps_per_launch=spl, **ecfg),
                      init_params=[p.to(DEV) for p in _init(spec)])
    assert (tr.lanes, tr.groups) == (4, groups)
    tr.train(STEPS)
    tr.synchronize()
    tr.check_comm()
    assert tr.step_ctr.tolist() == [STEPS, STEPS]
    out = tr.params.cpu(), tr.losses(0, STEPS), tr.loss_log.cpu()
    tr.close()
    return out


def _report(tag, got, ref):
    err = (got.double() - ref.double()).abs()
    print(f"{tag}: max abs err {err.max().item():.3e}, max rel err "
          f"{(err / ref.double().abs().clamp_min(1e-30)).max().item():.3e}")


def _check_fp32(p, l, ref):
    rp, rl = ref
    _report("loss", l, rl)
    _report("params", p, rp)
    torch.testing.assert_close(l, rl, rtol=2e-4, atol=1e-5)
    torch.testing.assert_close(p, rp, rtol=1e-4, atol=2e-5)


def test_parity_addresses_across_launches():
    """steps_per_launch 1, 2 and 3: a launch starts on either parity of the exchange buffer,
    and a one-step launch runs only the write-through exchange (plain stores start with a
    launch's second).  The three runs are the same bits and match the reference."""
    res = {spl: _run(256, 4, spl=spl) for spl in (1, 2, 3)}
    _check_fp32(*res[3][:2], _reference(256, "mse"))
    for spl in (1, 2):
        assert torch.equal(res[spl][0], res[3][0]), spl
        assert torch.equal(res[spl][1], res[3][1]), spl


@pytest.mark.parametrize("batch,groups", [(130, 3), (200, 4)])
def test_runtime_member_counts(batch, groups):
    """the instances that read the member count from the arguments, with every member's row
    read unconditionally.  130: 3 members, the third with 2 samples; 200: the epoch's last
    batch is 112, so member 2 is partly empty and member 3 wholly."""
    p, l, _ = _run(batch, groups)
    _check_fp32(p, l, _reference(batch, "mse"))


@pytest.mark.parametrize("loss,P", [("mse", 371), ("ce", 404)])
def test_every_parameter_after_scatter(loss, P):
    """P = 371 is odd: thread 185 owns one parameter and writes its other slot to the sink;
    the CE head's P = 404 has every owner thread own two.  Every parameter of both models
    matches the reference after 7 steps (each step's forward reads the scattered weights)."""
    p, l, _ = _run(256, 4, loss=loss)
    assert _spec(loss).P == P and tuple(p.shape) == (2, P)
    _check_fp32(p, l, _reference(256, loss))


def test_loss_ring_wraps():
    """a ring of 4 rows, 7 steps in launches of 3: row t % 4 holds the loss of the last step
    written there -- steps 4, 5, 6 and 3 -- for both models, and the parameters match."""
    p, _, ring = _run(256, 4, log_cap=4)
    rp, rl = _reference(256, "mse")
    assert tuple(ring.shape) == (4, 2)
    want = rl[[4, 5, 6, 3]]
    _report("ring", ring, want)
    torch.testing.assert_close(ring, want, rtol=2e-4, atol=1e-5)
    _report("params", p, rp)
    torch.testing.assert_close(p, rp, rtol=1e-4, atol=2e-5)

"""The split-batch step publishing its gradients straight from payload-order rows
(csrc/grp_core.h, payload-order rows): every member count, partly and wholly empty members, the
CE head's third publisher chunk, the bf16 loss slot and the launch modes, against autograd
+ torch.optim (tests/ref_train.py) at the tolerances of tests/test_lanes_gpu.py (GPU only).

Every case: n = 512, 7 steps at steps_per_launch = 3, so launches, exchange parities and
epochs cross."""
import functools

import pytest
import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream, SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC, MlpSpec, mlp_forward_ref_bf16
from distributed_training_pytorch_amd.ops.optim import OptimConfig

from .ref_train import torch_train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CE_SPEC = MlpSpec(2, 10, 5, 4)
STEPS = 7
ADAM = OptimConfig(lr=1e-2)
SGD = OptimConfig("sgd", 5e-2, momentum=0.9, weight_decay=1e-4)


def _init(spec):
    # Adam divides by sqrt(v): a parameter whose gradient is near zero in the first steps turns
    # rounding noise into a step of order lr, in any fp32 implementation.  The seed is the
    # smallest for which plain torch autograd in fp32 stays within 2 % of the tolerances below
    # of the fp64 reference in every configuration of this file (seed 31, say, puts torch's
    # own fp32 CE run 7 tolerances away from its fp64 run).
    g = torch.Generator().manual_seed(1)
    return [torch.randn(spec.P, generator=g) * 0.4 for _ in range(2)]


def _data(loss):
    return ToyData(n=512, seed=21, classes=4 if loss == "ce" else 0)


def _geom(batch):
    return SamplerGeometry(n=512, batch=batch, seed=3)


@functools.lru_cache(maxsize=None)
def _reference(batch, loss, optim, bf16):
    """autograd + torch.optim, computed once per configuration and shared"""
    spec = CE_SPEC if loss == "ce" else TOY_SPEC
    ds = _data(loss)
    kw = {"forward": mlp_forward_ref_bf16} if bf16 else {}
    return torch_train(spec, _init(spec), ds.X, ds.Y, [EpochIndexStream(_geom(batch))], STEPS,
                       SGD if optim == "sgd" else ADAM, loss, **kw)


def _run(batch, groups, loss="mse", optim="adam", **ecfg):
    spec = CE_SPEC if loss == "ce" else TOY_SPEC
    X, Y = _data(loss).device_tensors(DEV)
    ecfg.setdefault("steps_per_launch", 3)
    tr = FusedTrainer(spec, 2, X, Y, _geom(batch), SGD if optim == "sgd" else ADAM,
                      EngineConfig(loss=loss, groups="on", **ecfg), init_params=[p.to(DEV) for p in _init(spec)])
    assert (tr.lanes, tr.groups) == (4, groups)
    tr.train(STEPS)
    tr.synchronize()
    tr.check_comm()
    out = tr.params.cpu(), tr.losses(0, STEPS)
    assert tr.step_ctr.tolist() == [STEPS, STEPS]
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


@pytest.mark.parametrize("batch,groups", [(100, 2), (130, 3), (200, 4), (256, 4)])
def test_rows_member_counts_match_torch(batch, groups):
    """100: 2 members, the second with 36 samples; 130: 3 members, the third with 2;
    200: the epoch's last batch is 112, so member 2 is partly empty and member 3 empty;
    256: the 4-member instance with the member count as a constant."""
    p, l = _run(batch, groups)
    _check_fp32(p, l, _reference(batch, "mse", "adam", False))


def test_rows_sgd_matches_torch():
    p, l = _run(256, 4, optim="sgd")
    _check_fp32(p, l, _reference(256, "mse", "sgd", False))


def test_rows_ce_head_matches_torch():
    """MlpSpec(2, 10, 5, 4): 136 granules per member -- the publisher's third chunk (lanes
    q < 8) and three poll items on some lanes."""
    p, l = _run(256, 4, loss="ce")
    _check_fp32(p, l, _reference(256, "ce", "adam", False))


def test_rows_bf16_loss_slot_matches_rounding_model():
    """bf16 compute: the wave's fp32 loss is written into the row's loss float after the
    park (the tile's loss cell saw bf16-truncated values and is parked in the sink).  The
    reference is autograd through the bf16 rounding model; accumulation order may move a
    bf16 value by one ulp (2^-8 = 3.9e-3 relative), hence the tolerances of the bf16 tests
    (tests/test_bf16_gpu.py) instead of the fp32 ones.  The loss itself is an fp32 sum of
    fp32 per-sample values of bf16-rounded outputs: had the truncated tile cell been
    published instead, it would be off by up to 2^-8 relative on every step."""
    p, l = _run(256, 4, precision="bf16")
    rp, rl = _reference(256, "mse", "adam", True)
    _report("loss", l, rl)
    _report("params", p, rp)
    torch.testing.assert_close(l, rl, rtol=2e-2, atol=1e-3)
    torch.testing.assert_close(p, rp, rtol=2e-2, atol=2e-3)
    fp_l = _reference(256, "mse", "adam", False)[1]
    assert not torch.allclose(l, fp_l, rtol=1e-6, atol=0)  # bf16 compute for real


def test_rows_bitwise_across_launch_modes():
    """persistent, per-step eager launches and hipGraph replays of the row form give bitwise
    the same state and losses (member-order sums, whatever order the members finish in)."""
    res = {"persistent": _run(256, 4), "eager": _run(256, 4, launch="eager"), "graph": _run(256, 4, launch="graph")}
    _check_fp32(*res["persistent"], _reference(256, "mse", "adam", False))
    for k in ("eager", "graph"):
        assert torch.equal(res["persistent"][0], res[k][0]), k
        assert torch.equal(res["persistent"][1], res[k][1]), k

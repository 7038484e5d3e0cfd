"""The flat optimizer that writes the FP8 weight operands (csrc/optim_fp8.hip, ops.fp8.Fp8WeightShadow) on the
GPU: one kernel step against the definitions bit for bit, training with the shadow against training without
it, graph replay, staleness and the refusals."""
import ctypes

import pytest
import torch

from distributed_training_pytorch_amd import _native as nat
from distributed_training_pytorch_amd.engine.graph_step import CapturedStep
from distributed_training_pytorch_amd.models.bank import ModelBank
from distributed_training_pytorch_amd.ops.fp8 import Fp8DelayedState, Fp8WeightShadow
from distributed_training_pytorch_amd.ops.optim import OptimConfig, flat_optimizer_step
from distributed_training_pytorch_amd.ops.schedule import LrSchedule

from .fp8_cases import ref_bytes
from .test_fp8_shadow_cpu import STEPS, check_same, check_stale, train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# name -> (P, [(column offset, out, in)]): the columns between the weights are bias-like spans
LAYOUTS = {
    "lone16": (16 * 16 + 7, [(0, 16, 16)]),                      # one partial tile
    "48x80@5": (5 + 48 * 80 + 3, [(5, 48, 80)]),                 # ragged both ways, element loads in both rows
    "80x80+128x64": (80 * 80 + 11 + 128 * 64 + 2, [(0, 80, 80), (80 * 80 + 11, 128, 64)]),  # P odd, > 4096: row 1 by
}                                                                # element, two records per row, the multi-block norm
VARIANTS = {
    "adam": dict(cfg=dict(name="adam")),
    "adamw": dict(cfg=dict(name="adamw", weight_decay=0.1)),
    "norm": dict(cfg=dict(name="adam", max_grad_norm=0.5)),
    "value": dict(cfg=dict(name="adam", clip_grad_value=0.3)),
    "sched": dict(cfg=dict(name="adam", schedule=LrSchedule.from_values([1e-2, 5e-3, 2e-3])), grad_scale=0.25, zero_grad=True),
    "sgd": dict(cfg=dict(name="sgd", momentum=0.9, lr=1e-2)),
}


def _buffers(P, seed=0):
    g = torch.Generator().manual_seed(seed)
    params, grad = torch.randn(2, P, generator=g), torch.randn(2 * P + 2, generator=g)
    return [t.to(DEV) for t in (params, torch.zeros(2, P), torch.zeros(2, P), torch.zeros(2, dtype=torch.int32), grad)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_kernel_step_against_the_definitions(layout, variant):
    P, mats = LAYOUTS[layout]
    assert layout != "80x80+128x64" or (P % 2 == 1 and P > 4096)
    var = VARIANTS[variant]
    cfg = OptimConfig(lr=1e-2, **var["cfg"]) if "lr" not in var["cfg"] else OptimConfig(**var["cfg"])
    kw = dict(grad_scale=var.get("grad_scale", 1.0), zero_grad=var.get("zero_grad", False))
    got, want = _buffers(P), _buffers(P)
    views = [got[0][r, c:c + o * i].view(o, i) for r in range(2) for c, o, i in mats]
    state = Fp8DelayedState(len(views), device=DEV)
    # per weight: a scale that keeps every |p * scale| in range, then one that saturates some
    scales = [torch.tensor(s) for _ in views for s in (64.0, 200.0)][:len(views)]
    for k, s in enumerate(scales):
        state.set_scale(k, s)
    sh = Fp8WeightShadow(got[0], views, [state.slot(k) for k in range(len(views))])
    norms = [torch.zeros(2, device=DEV) for _ in range(2)]
    for step in range(2):
        g = torch.randn(2 * P + 2, generator=torch.Generator().manual_seed(10 + step)).to(DEV)
        got[4].copy_(g), want[4].copy_(g)
        flat_optimizer_step(*got, cfg, shadow=sh, norm_out=norms[0], **kw)
        flat_optimizer_step(*want, cfg, norm_out=norms[1], **kw)
        for name, a, b in zip(("params", "m", "v", "step", "grad"), got, want):
            assert torch.equal(a, b), (name, step)
        assert torch.equal(norms[0], norms[1]) and got[3].tolist() == [step + 1] * 2
        clamped = 0
        for k, w in enumerate(views):
            wc, s = w.detach().cpu(), scales[k]
            prod = wc * s  # fp32 product and clamp, then the suite's fp64 model of the format
            clamped += int((prod.abs() > 448).sum())
            q = sh.q[k].cpu().view(torch.uint8)
            assert torch.equal(q, ref_bytes(prod.clamp(-448.0, 448.0), "e4m3")), (k, step)
            assert torch.equal(sh.qT[k].cpu().view(torch.uint8), q.t()), (k, step)
            assert torch.equal(sh.used[k].cpu(), torch.stack([s, torch.ones_like(s) / s])), (k, step)
            tiles = -(-w.shape[0] // 64) * -(-w.shape[1] // 64)
            assert int(state.partials[k, 0]) == tiles
            assert torch.equal(state.amax_of(k).cpu(), wc.abs().max()), (k, step)
        assert clamped > 0  # the saturating scale met the clamp
    assert sh.operand(views[0]) is not None and sh.served == 1


@pytest.mark.parametrize("H,h", [(32, 16), (80, 2)])  # (80, 2): ragged tiles, and the amax ring wraps within the run
def test_training_with_the_shadow_is_bit_identical(H, h):
    got, want = train(DEV, H, h, True), train(DEV, H, h, False)
    check_same(got, want)
    assert got[4] == [0] + [4] * (STEPS - 1)


def test_graph_replay_equals_eager():
    """Steps 1-2 eager (the stepper's warm-up), step 3 captured, steps 3-6 replayed."""
    stepper = {}

    def run(body, i):
        stepper.setdefault("s", CapturedStep(body, DEV, warmup=2)).run()

    got = train(DEV, 80, 2, True, run=run)
    assert stepper["s"].replays == STEPS - 2 and stepper["s"].fallback_reason is None
    check_same(got, train(DEV, 80, 2, True))


def test_a_stale_shadow_quantises_by_launch():
    check_stale(DEV)


def test_refusals():
    lib = nat.require(DEV)
    P = 24 * 16 + 16 * 16
    params, m, v, step, grad = _buffers(P)
    state = Fp8DelayedState(2, device=DEV)
    state.set_scale(0, 1.0), state.set_scale(1, 1.0)
    ok = params[0, 24 * 16:].view(16, 16)
    with pytest.raises(ValueError, match="multiples of 16"):
        Fp8WeightShadow(params, [params[0, :24 * 16].view(24, 16)], [state.slot(0)])
    with pytest.raises(ValueError, match="Fp8Slot"):
        Fp8WeightShadow(params, [ok], [None])
    with pytest.raises(ValueError, match="exclusive"):
        OptimConfig(max_grad_norm=1.0, clip_grad_value=1.0)
    with pytest.raises(ValueError, match="decoupled"):
        OptimConfig(name="sgd", decoupled_weight_decay=True)
    sh = Fp8WeightShadow(params, [ok], [state.slot(1)])
    norm_out = torch.zeros(2, device=DEV)

    def rc(edit_args=None, edit_rec=None):
        """The C entry's return code with one argument or record field changed."""
        cfg = OptimConfig()
        a = nat.OptArgs(nat.ptr(params), nat.ptr(m), nat.ptr(v), nat.ptr(step), nat.ptr(grad), None, 0, 2, P, cfg.kind, 1.0,
                        0, cfg.hyper(device=DEV), None, 0, 0.0, 0.0, None, nat.ptr(norm_out))
        recs = (nat.Fp8ShadowRec * 1)()
        ctypes.memmove(recs, sh._host_recs, ctypes.sizeof(recs))
        if edit_args:
            edit_args(a)
        if edit_rec:
            edit_rec(recs[0])
        return lib.dtp_flat_optimizer_fp8(ctypes.byref(a), recs, 1, ctypes.byref(sh._work), nat.stream_ptr())

    before = params.clone()
    assert rc(edit_rec=lambda r: (setattr(r, "out", 24), setattr(r, "offset", 0))) != 0
    assert rc(edit_rec=lambda r: setattr(r, "scale", None)) != 0
    assert rc(edit_args=lambda a: (setattr(a, "max_norm", 1.0), setattr(a, "clip_value", 1.0))) != 0
    assert rc(edit_args=lambda a: (setattr(a, "kind", nat.MODE_SGD), setattr(a.hp, "decoupled_wd", 1))) != 0
    assert rc(edit_rec=lambda r: setattr(r, "cap", 0)) != 0
    torch.cuda.synchronize()
    assert torch.equal(params, before)  # a refused call launches nothing
    for kw in (dict(compute_dtype=torch.bfloat16), dict(compute_dtype=torch.float8_e4m3fn, fp8_recipe="current")):
        with pytest.raises(ValueError, match="delayed"):
            ModelBank(2, hidden=32, depth=1, **kw).to(DEV).fp8_shadow()

"""--fp8_shadow without a GPU: training with the optimizer-written FP8 weight operands (``ops.fp8.
Fp8WeightShadow``, the torch definition of ``csrc/optim_fp8.hip``) against training without them, the
parser, the runner's precision rule and demo.py on the CPU."""
import os
import subprocess
import sys

import pytest
import torch

from distributed_training_pytorch_amd.models.bank import ModelBank
from distributed_training_pytorch_amd.ops.gemm import mlp
from distributed_training_pytorch_amd.ops.optim import FlatOptimizer, OptimConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS, BATCH = 6, 64


def train(dev, H, h, shadow, steps=STEPS, run=None, touch_before=()):
    """``steps`` Adam steps of a two-model delayed-FP8 bank on fixed batches -> (losses per step, flat, m, v,
    operands served per step).  ``run(body, i)``: how step i's body runs (default: call it);
    ``touch_before``: steps preceded by a torch in-place write to ``bank.flat`` that changes no value."""
    torch.manual_seed(0)
    bank = ModelBank(2, hidden=H, depth=2, compute_dtype=torch.float8_e4m3fn, fp8_recipe="delayed",
                     fp8_amax_history=h).to(dev)
    sh = bank.fp8_shadow() if shadow else None
    opt = FlatOptimizer(bank.flat, bank.flat_grad, OptimConfig(lr=1e-3), shadow=sh)
    g = torch.Generator().manual_seed(1)
    X, Y = torch.randn(steps, BATCH, 2, generator=g).to(dev), torch.randn(steps, BATCH, 1, generator=g).to(dev)
    x, y = torch.empty_like(X[0]), torch.empty_like(Y[0])
    losses = torch.zeros(steps, 2, device=dev)
    row = torch.zeros(2, device=dev)

    def forward(m):  # ToyModel's GPU forward at these widths, on either device (its CPU forward is plain torch)
        lin = [layer for layer in m.layers if isinstance(layer, torch.nn.Linear)]
        ws = [layer.weight for layer in lin]
        return mlp(x, ws, [layer.bias for layer in lin], m.spec.slope, m.compute_dtype, fp8_state=m._fp8_state(ws))

    def body(_=None):
        bank.zero_grad()
        ox, oy = forward(bank[0]), forward(bank[1])
        lx, ly = ((ox.float() - y) ** 2).mean(), ((oy.float() - y) ** 2).mean()
        (lx + ly).backward()
        opt.step()
        row.copy_(torch.stack([lx.detach(), ly.detach()]))

    served = []
    for i in range(steps):
        if i in touch_before:
            with torch.no_grad():
                bank.flat.mul_(1.0)
        x.copy_(X[i]), y.copy_(Y[i])
        before = sh.served if sh else 0
        run(body, i) if run else body()
        losses[i] = row
        served.append((sh.served if sh else 0) - before)
    return losses.cpu(), bank.flat.detach().cpu(), opt.m.cpu(), opt.v.cpu(), served


def check_same(got, want):
    for name, a, b in zip(("losses", "flat", "m", "v"), got, want):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("H,h", [(32, 16), (80, 2)])  # (80, 2): the amax ring wraps within the run
def test_training_with_the_shadow_is_bit_identical_cpu(H, h):
    got, want = train("cpu", H, h, True), train("cpu", H, h, False)
    check_same(got, want)
    assert got[4] == [0] + [4] * (STEPS - 1)  # two hidden weights per model; step 1 seeds through the quantiser


def check_stale(dev):
    """An in-place write to the flat buffer before step 4: that forward quantises by a launch (nothing served),
    the optimizer's next write makes the shadow fresh again, and the run is still the unshadowed one."""
    got, want = train(dev, 80, 2, True, touch_before=(3,)), train(dev, 80, 2, False, touch_before=(3,))
    check_same(got, want)
    assert got[4] == [0, 4, 4, 0, 4, 4]


def test_a_stale_shadow_quantises_by_launch_cpu():
    check_stale("cpu")


def test_parser_runner_and_the_precision_rule():
    import argument_parser
    from distributed_training_pytorch_amd.engine import runner

    cfg = argument_parser.get_args(["--precision", "fp8-delayed", "--fp8_shadow", "--hidden", "32"])
    assert cfg.fp8_shadow and runner._fp8_shadow(cfg)
    assert not runner._fp8_shadow(argument_parser.get_args(["--precision", "fp8-delayed", "--hidden", "32"]))
    with pytest.raises(ValueError, match="fp8-delayed"):
        runner._fp8_shadow(argument_parser.get_args(["--precision", "fp8", "--fp8_shadow", "--hidden", "32"]))


def test_demo_fp8_shadow_on_the_cpu(tmp_path):
    env = dict(os.environ, WANDB_MODE="dryrun")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "demo.py", "--device", "cpu", "--backend", "gloo", "--precision", "fp8-delayed",
                        "--fp8_shadow", "--hidden", "32", "--iters", "3", "--dry_run", "--no_progress", "--log_dir",
                        str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=200, env=env)
    assert r.returncode == 0 and "Finished" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "'fp8_weight_shadow': True" in r.stdout, r.stdout[-2000:]

"""--precision fp8-delayed without a GPU: the torch definition of the delayed-scaling recipe against
current scaling (``ops/fp8.py``), the parser, the width rule, and demo.py on the CPU."""
import os
import subprocess
import sys

import pytest
import torch

from distributed_training_pytorch_amd.models.wide import WideMLP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WIDTHS, BATCH = (2, 32, 48, 32, 1), 40


def recipe_steps(dev, recipe, steps, lr=0.0, dtype=torch.float32, cd=torch.float8_e4m3fn):
    """[output, every gradient] of each of ``steps`` steps of WideMLP(WIDTHS) on one repeated batch, as
    fp64 CPU tensors; plain SGD with ``lr`` between them (0: frozen weights).  ``recipe`` None: the plain
    PyTorch forward of the same module tree."""
    torch.manual_seed(0)
    m = WideMLP(WIDTHS, compute_dtype=cd, fp8_recipe=recipe or "current").to(dev, dtype)
    g = torch.Generator().manual_seed(1)
    x, gy = torch.randn(BATCH, WIDTHS[0], generator=g).to(dev, dtype), torch.randn(BATCH, 1, generator=g).to(dev)
    out = []
    for _ in range(steps):
        m.zero_grad()
        y = m(x) if recipe else m.reference_forward(x)
        y.backward(gy.to(y.dtype))
        out.append([y.detach().double().cpu()] + [p.grad.double().cpu() for p in m.parameters()])
        with torch.no_grad():
            for p in m.parameters():
                p -= lr * p.grad
    return out


def check_delayed_equals_current(dev):
    """Frozen weights, one batch: every history's maximum is the current amax, so from step 2 on the
    delayed recipe is the current one bit for bit (step 0 is seeded: current scaling by construction)."""
    cur = recipe_steps(dev, "current", 1)[0]
    for got in recipe_steps(dev, "delayed", 4)[2:]:
        for c, d in zip(cur, got):
            assert torch.equal(c, d)


def test_delayed_equals_current_on_a_repeated_batch_cpu():
    check_delayed_equals_current("cpu")


def test_parser_and_the_width_rule():
    import argument_parser
    from distributed_training_pytorch_amd.engine import runner

    cfg = argument_parser.get_args(["--precision", "fp8-delayed", "--hidden", "32"])
    assert cfg.precision == "fp8-delayed" and cfg.fp8_amax_history == 16
    assert runner._compute_dtype(cfg) == torch.float8_e4m3fn and not runner._fused_supported(cfg)
    assert runner._fp8_recipe(cfg) == {"fp8_recipe": "delayed", "fp8_amax_history": 16}
    with pytest.raises(ValueError, match="multiple of 16"):
        runner._compute_dtype(argument_parser.get_args(["--precision", "fp8-delayed", "--hidden", "10"]))


def test_demo_fp8_delayed_on_the_cpu(tmp_path):
    env = dict(os.environ, WANDB_MODE="dryrun")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "demo.py", "--device", "cpu", "--backend", "gloo", "--precision", "fp8-delayed",
                        "--hidden", "32", "--iters", "4", "--batch_size", "64", "--seed", "1", "--dry_run", "--no_progress",
                        "--log_dir", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=200, env=env)
    assert r.returncode == 0 and "Finished" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "engine: module" in r.stdout and "'fp8_recipe': 'delayed (amax history 16)'" in r.stdout, r.stdout[-2000:]

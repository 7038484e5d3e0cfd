"""--precision fp8 without a GPU: the torch definition of the FP8 ops, the parser, the width
rule, and demo.py on the CPU."""
import os
import subprocess
import sys

import pytest
import torch

from distributed_training_pytorch_amd.ops.fp8 import gemm_fp8, quantize_fp8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.mark.parametrize("shape,fmt_a", [((33, 20, 48), "e4m3"), ((16, 64, 144), "e5m2")])
def test_cpu_gemm_fp8_is_its_definition(shape, fmt_a):
    M, N, K = shape
    g = torch.Generator().manual_seed(0)
    x, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g).bfloat16(), torch.randn(N, generator=g)
    a, b = quantize_fp8(x, fmt_a, transpose=True), quantize_fp8(w, "e4m3")
    tdt, fmax = (torch.float8_e4m3fn, 448.0) if fmt_a == "e4m3" else (torch.float8_e5m2, 57344.0)
    scale = torch.tensor(fmax) / x.abs().max()
    assert a.data.dtype == tdt and torch.equal(a.scale, scale) and torch.equal(a.scale_inv, torch.tensor(1.0) / scale)
    assert torch.equal(a.data.float(), (x * scale).to(tdt).float()) and torch.equal(a.data_t.float(), a.data.float().t())
    want = (a.data.float() * a.scale_inv) @ (b.data.float() * b.scale_inv).t() + bias
    want = torch.nn.functional.leaky_relu(want, 0.1)
    got = gemm_fp8(a, b, bias=bias, act=True, slope=0.1, out_dtype=torch.float32)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)  # the scales applied before / after the sum


def test_parser_and_the_width_rule():
    import argument_parser
    from distributed_training_pytorch_amd.engine import runner

    cfg = argument_parser.get_args(["--precision", "fp8", "--hidden", "32"])
    assert cfg.precision == "fp8" and runner._compute_dtype(cfg) == torch.float8_e4m3fn
    assert not runner._fused_supported(cfg)
    with pytest.raises(ValueError, match="multiple of 16"):
        runner._compute_dtype(argument_parser.get_args(["--precision", "fp8", "--hidden", "10"]))


def test_demo_fp8_on_the_cpu(tmp_path):
    env = dict(os.environ, WANDB_MODE="dryrun")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    base = [sys.executable, "demo.py", "--device", "cpu", "--backend", "gloo", "--precision", "fp8", "--iters", "4",
            "--batch_size", "64", "--seed", "1", "--dry_run", "--no_progress", "--log_dir", str(tmp_path)]
    r = subprocess.run([*base, "--hidden", "32"], cwd=ROOT, capture_output=True, text=True, timeout=200, env=env)
    assert r.returncode == 0 and "Finished" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "engine: module" in r.stdout
    r = subprocess.run([*base, "--hidden", "10"], cwd=ROOT, capture_output=True, text=True, timeout=200, env=env)
    assert r.returncode != 0 and "--hidden to be a multiple of 16" in r.stderr, r.stderr[-2000:]

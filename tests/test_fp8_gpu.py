"""FP8 on the wide-MLP path (csrc/fp8_quant.hip, csrc/gemm_fp8.hip, ops/fp8.py): the
quantiser against torch's cast, the GEMM against fp64 under a derived bound, the MLP function
against fp64 autograd relative to its own CPU emulation, and ``demo.py --precision fp8``."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_training_pytorch_amd.ops.fp8 import gemm_fp8, quantize_fp8
from distributed_training_pytorch_amd.ops.gemm import mlp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"e4m3": (torch.float8_e4m3fn, 448.0), "e5m2": (torch.float8_e5m2, 57344.0)}
U = 2.0 ** -23  # fp32 unit roundoff taken one bit wide, so a truncating accumulator is covered


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------ A: quantiser
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 16), (33, 48), (64, 64), (130, 272)])  # the transpose tile is 64 x 64
def test_quantiser_matches_torch_cast(fmt, dtype, shape):
    tdt, fmax = FMT[fmt]
    x = (3.0 * _randn(*shape, seed=shape[0])).to(dtype)
    q = quantize_fp8(x.to(DEV), fmt, transpose=True)
    scale, scale_inv = q.scale.cpu(), q.scale_inv.cpu()
    # the amax is exact and the division correctly rounded (tensor / tensor: one IEEE division)
    assert torch.equal(scale, torch.tensor(fmax) / x.float().abs().max())
    assert abs(float(scale.double() * scale_inv.double()) - 1.0) <= U
    want = (x.float() * scale).to(tdt).float()
    assert torch.equal(q.data.float().cpu(), want)
    assert q.data_t.shape == (shape[1], shape[0]) and torch.equal(q.data_t.float().cpu(), want.t())


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_quantiser_all_zero_input(fmt):
    q = quantize_fp8(torch.zeros(33, 48, device=DEV), fmt, transpose=True)
    assert float(q.scale) == 1.0 and float(q.scale_inv) == 1.0
    assert not q.data.float().any() and not q.data_t.float().any()


# ------------------------------------------------------------------------------ B: GEMM
def _check_gemm(a, b, M, N, trans, epi, **opt):
    """fp64 product of the dequantised operands; products of two FP8 values are exact in fp32, so
    only the accumulation rounds: |C - ref| <= K U (|A| |B|^T) sa_inv sb_inv, carried through the
    epilogue (every step of it is 1-Lipschitz for slope <= 1), plus one fp32 rounding of the
    largest epilogue intermediate (scale product and epilogue arithmetic) and, for a bf16 output,
    the cast at relative 2^-8."""
    A = (a.data_t if trans else a.data).double().cpu()
    B = (b.data_t if trans else b.data).double().cpu()
    s = a.scale_inv.double().cpu() * b.scale_inv.double().cpu()
    lin, mag = (A @ B.t()) * s, (A.abs() @ B.abs().t()) * s
    kw, ref, slope = {}, lin, 0.1
    out_dtype = torch.float32 if epi in ("none", "acc") else torch.bfloat16
    if epi == "bias_act":
        bias = _randn(N, seed=5)
        ref = torch.nn.functional.leaky_relu(lin + bias.double(), slope)
        mag = mag + bias.abs().double()
        kw = dict(bias=bias.to(DEV), act=True, slope=slope)
    elif epi == "aux":
        aux = _randn(M, N, seed=6).bfloat16()
        ref = lin * torch.where(aux.double() > 0, 1.0, slope)
        kw = dict(aux=aux.to(DEV), slope=slope)
    elif epi == "acc":
        old = _randn(M, N, seed=7)
        ref = lin + old.double()
        mag = mag + old.abs().double()
        kw = dict(out=old.to(DEV), accumulate=True)
    c = gemm_fp8(a, b, trans_a=trans, trans_b=trans, out_dtype=out_dtype, **kw, **opt).double().cpu()
    K = A.shape[1]
    tol = K * U * mag + U * mag + (2.0 ** -8 * ref.abs() if out_dtype == torch.bfloat16 else 0.0)
    worst = float(((c - ref).abs() - tol).max())
    print(f"M={M} N={N} K={K} {a.fmt}x{b.fmt} {epi}: max |C-ref| {float((c - ref).abs().max()):.3e}, "
          f"max excess over the bound {worst:.3e}")
    assert c.shape == (M, N) and torch.isfinite(c).all() and worst <= 0.0


# tile 256 x 256, K-tile 128 bytes: every edge in M and in N, K below / at / past one K-tile and three
@pytest.mark.parametrize("fmt_a", ["e4m3", "e5m2"])
@pytest.mark.parametrize("K", [16, 128, 144, 384])
@pytest.mark.parametrize("MN", [(16, 16), (256, 256), (272, 16), (16, 272), (256, 272), (272, 272)])
def test_gemm_fp8_against_fp64(fmt_a, K, MN):
    """K <= 256 runs on the short-K instance (FP8 bytes decoded for the exact-fp32 MFMA), K = 384 on
    the pipelined FP8-MFMA kernel: the FP8 matrix unit keeps about 15 bits below the largest
    product of one instruction, which a short sum cannot hide under this bound (measured on the
    pipelined kernel, max |C - ref| / (|A| |B|^T) against (K + 1) 2^-23: K = 16: 1.4e-4 vs 2.0e-6;
    K = 128: 2.1e-5 vs 1.5e-5; K = 384: 7.9e-6 vs 4.6e-5; K = 4096: 1.7e-6 vs 4.9e-4)."""
    M, N = MN
    a = quantize_fp8(_randn(M, K, seed=1).to(DEV), fmt_a)
    b = quantize_fp8(_randn(N, K, seed=2).to(DEV), "e4m3")
    _check_gemm(a, b, M, N, False, "none")


# the two instances' own edge rows: the last short K and the first pipelined one (two K-tiles and
# a tail), three K-tiles and a tail; the short instance's 64 x 64 tile and one fragment past it
@pytest.mark.parametrize("fmt_a", ["e4m3", "e5m2"])
@pytest.mark.parametrize("MNK", [(80, 64, 256), (272, 264, 272), (272, 264, 400)])
def test_gemm_fp8_instance_edges(fmt_a, MNK):
    M, N, K = MNK
    a = quantize_fp8(_randn(M, K, seed=10).to(DEV), fmt_a)
    b = quantize_fp8(_randn(N, K, seed=11).to(DEV), "e4m3")
    _check_gemm(a, b, M, N, False, "none")


@pytest.mark.parametrize("fmt_a", ["e4m3", "e5m2"])
@pytest.mark.parametrize("epi", ["none", "bias_act", "aux", "acc"])
@pytest.mark.parametrize("K", [144, 400])  # the short-K and the pipelined instance
def test_gemm_fp8_epilogues(fmt_a, epi, K):
    M, N = 272, 264
    a = quantize_fp8(_randn(M, K, seed=3).to(DEV), fmt_a)
    b = quantize_fp8(_randn(N, K, seed=4).to(DEV), "e4m3")
    _check_gemm(a, b, M, N, False, epi)


# the 16x16x32 fp8 / bf8 MFMAs (mfma=1) in the pipelined kernel, under the same bound
@pytest.mark.parametrize("fmt_a", ["e4m3", "e5m2"])
# (the K = 256 row runs on the short instance, which has no MFMA choice: kept so that the option is
# seen to be ignored there, the 16x16x32 kernels are the K = 272 and 400 rows)
@pytest.mark.parametrize("MNK", [(80, 64, 256), (272, 264, 272), (272, 264, 400)])
def test_gemm_fp8_instance_edges_mfma1(fmt_a, MNK):
    M, N, K = MNK
    a = quantize_fp8(_randn(M, K, seed=10).to(DEV), fmt_a)
    b = quantize_fp8(_randn(N, K, seed=11).to(DEV), "e4m3")
    _check_gemm(a, b, M, N, False, "none", mfma=1)


@pytest.mark.parametrize("fmt_a", ["e4m3", "e5m2"])
@pytest.mark.parametrize("epi", ["none", "bias_act", "aux", "acc"])
def test_gemm_fp8_epilogues_mfma1(fmt_a, epi):
    M, N, K = 272, 264, 400
    a = quantize_fp8(_randn(M, K, seed=3).to(DEV), fmt_a)
    b = quantize_fp8(_randn(N, K, seed=4).to(DEV), "e4m3")
    _check_gemm(a, b, M, N, False, epi, mfma=1)


def test_gemm_fp8_transposed_copies_with_padded_k():
    """The dW form: both operands are transposed copies whose rows (K = 392, three K-tiles and a
    tail) are zero-padded to 400; the weight operand was quantised from a view that is only
    4-byte aligned (a row of a flat parameter buffer)."""
    a = quantize_fp8(_randn(392, 272, seed=8).to(DEV), "e5m2", transpose=True)
    flat = torch.zeros(392 * 32 + 1, device=DEV)
    flat[1:] = _randn(392 * 32, seed=9).to(DEV)
    b = quantize_fp8(flat[1:].view(392, 32), "e4m3", transpose=True)
    _check_gemm(a, b, 272, 32, True, "acc")


# ------------------------------------------------------------------------------ C: the MLP function
def test_mlp_fp8_against_fp64_and_its_cpu_emulation():
    """Per tensor (output, every weight and bias gradient): with e_ref the relative error of the CPU
    emulation (same quantisation points, torch casts) against fp64 autograd of the unquantised
    model, the GPU's relative error must be <= 2 e_ref: the GPU's bf16 intermediates can flip
    individual FP8 rounding decisions, independent errors of the emulation's own size (sqrt 2)."""
    widths, batch, slope = (2, 128, 144, 1), 80, 0.01
    g = torch.Generator().manual_seed(0)
    params = []
    for i, o in zip(widths[:-1], widths[1:]):
        params += [torch.randn(o, i, generator=g) / i ** 0.5, 0.1 * torch.randn(o, generator=g)]
    x, gy = torch.randn(batch, widths[0], generator=g), torch.randn(batch, widths[-1], generator=g)

    def run(dev, dtype, cd):
        ps = [p.clone().to(dev, dtype).requires_grad_() for p in params]
        xx = x.to(dev, dtype)
        if cd is None:  # plain autograd
            h = xx
            for l in range(0, len(ps), 2):
                h = torch.nn.functional.linear(h, ps[l], ps[l + 1])
                if l + 2 < len(ps):
                    h = torch.nn.functional.leaky_relu(h, slope)
            out = h
        else:
            out = mlp(xx, ps[0::2], ps[1::2], slope, cd)
        out.backward(gy.to(dev, out.dtype))
        return [out.detach().double().cpu()] + [p.grad.double().cpu() for p in ps]

    r64 = run("cpu", torch.float64, None)
    emu = run("cpu", torch.float32, torch.float8_e4m3fn)
    gpu = run(DEV, torch.float32, torch.float8_e4m3fn)
    names = ["out"] + [f"{'dW' if i % 2 == 0 else 'db'}{i // 2}" for i in range(len(params))]
    rows = []
    for n, r, e, c in zip(names, r64, emu, gpu):
        rows.append((n, float((e - r).norm() / r.norm()), float((c - r).norm() / r.norm())))
        print(f"{rows[-1][0]:>4}: e_ref {rows[-1][1]:.4e}  gpu {rows[-1][2]:.4e}")
    for n, e_ref, e_gpu in rows:
        assert e_gpu <= 2.0 * e_ref, (n, e_ref, e_gpu)


# ------------------------------------------------------------------------------ E: entrypoint
def test_demo_precision_fp8_runs_the_module_engine(tmp_path):
    env = dict(os.environ, WANDB_MODE="dryrun")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "demo.py", "--precision", "fp8", "--hidden", "128", "--iters", "100", "--seed", "0",
                        "--dry_run", "--no_progress", "--log_every", "25", "--log_dir", str(tmp_path)], cwd=ROOT,
                       capture_output=True, text=True, timeout=150, env=env)
    assert r.returncode == 0 and "Finished" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "precision=fp8: using the module engine" in r.stdout and "engine: module" in r.stdout, r.stdout[-2000:]
    rows = [json.loads(l) for l in open(tmp_path / "metrics.jsonl") if "loss/" in l]
    for k in ("loss/lossX", "loss/lossY"):
        v = torch.tensor([row[k] for row in rows if k in row])
        assert len(v) == 100 and torch.isfinite(v).all() and v[-10:].mean() < v[:10].mean(), (k, v[:10], v[-10:])

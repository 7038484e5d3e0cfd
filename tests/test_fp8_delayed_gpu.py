"""FP8 delayed scaling on the GPU (csrc/gemm_epi_quant.h, csrc/gemm_fp8.hip, csrc/fp8_quant.hip, ops/fp8.py):
the quantising GEMM epilogue, the given-scale quantiser and the scale update, each byte for byte against
the torch definition; the recipe against current scaling and against its own CPU definition."""
import pytest
import torch

from distributed_training_pytorch_amd.ops.fp8 import Fp8DelayedState, gemm_fp8, quantize_fp8

from .test_fp8_delayed_cpu import check_delayed_equals_current, recipe_steps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FMT = {"e4m3": (torch.float8_e4m3fn, 448.0), "e5m2": (torch.float8_e5m2, 57344.0)}


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def _check_quantised(q, x, scale, fmt, state, sat):
    """q.data, the whole padded q.data_t and the slot's amax against the torch definition applied to ``x``."""
    tdt, fmax = FMT[fmt]
    M, N = x.shape
    Mp = -(-M // 16) * 16
    xs = x.float().cpu() * scale
    clamped = int((xs.abs() > fmax).sum())
    # a saturating scale must meet both branches of the clamp (the tensor's own scale meets it at most where
    # amax * (fmax / amax) rounds a hair past fmax)
    xa = x.float().abs().cpu()
    assert 0 < clamped < x.numel() / 2 if sat > 1 else clamped <= int((xa == xa.max()).sum()), clamped
    want = xs.clamp(-fmax, fmax).to(tdt)
    assert torch.equal(_bytes(q.data), _bytes(want))
    want_t = torch.zeros(N, Mp, dtype=tdt)
    want_t[:, :M] = want.t()
    assert torch.equal(_bytes(torch.as_strided(q.data_t, (N, Mp), (Mp, 1))), _bytes(want_t))
    assert torch.equal(state.amax_of(0).cpu(), x.float().abs().max().cpu())
    assert torch.equal(q.scale.cpu(), scale) and q.fmt == fmt


# K = 288: pipelined with a K tail; K = 128: the short-K instance; "view": C only 2-byte aligned (per-element epilogue)
EPI_CASES = [(form, M, N, 288, False) for form in ("fwd", "dx") for M, N in ((256, 256), (300, 272), (40, 48))]
EPI_CASES += [("fwd", 300, 272, 128, False), ("dx", 300, 272, 288, True)]


@pytest.mark.parametrize("sat", [1, 8])
@pytest.mark.parametrize("form,M,N,K,view", EPI_CASES, ids=lambda v: str(v))
def test_gemm_epilogue_emits_the_quantised_output(form, M, N, K, view, sat):
    fmt = "e4m3" if form == "fwd" else "e5m2"
    a = quantize_fp8(_randn(M, K, seed=1).to(DEV), fmt)
    b = quantize_fp8(_randn(N, K, seed=2).to(DEV), "e4m3")
    kw = (dict(bias=_randn(N, seed=3).to(DEV), act=True, slope=0.1) if form == "fwd"
          else dict(aux=_randn(M, N, seed=4).bfloat16().to(DEV), slope=0.1))

    def out():
        return torch.empty(M * N + 1, dtype=torch.bfloat16, device=DEV)[1:].view(M, N) if view else None

    plain = gemm_fp8(a, b, out=out(), out_dtype=torch.bfloat16, **kw)
    scale = torch.tensor(FMT[fmt][1]) / plain.float().abs().max().cpu() * sat
    state = Fp8DelayedState(1, device=DEV)
    state.set_scale(0, scale, fmt)
    c, q = gemm_fp8(a, b, out=out(), out_dtype=torch.bfloat16, quant_out=(fmt, state.slot(0)), **kw)
    assert torch.equal(c.view(torch.int16), plain.view(torch.int16))
    _check_quantised(q, c, scale, fmt, state, sat)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,view", [((1, 16), False), ((64, 64), False), ((70, 48), False), ((70, 48), True)])
def test_given_scale_quantiser(fmt, dtype, shape, view):
    M, K = shape
    x = (3.0 * _randn(M, K, seed=M)).to(dtype)
    xd = x.to(DEV)
    if view:  # element-aligned only
        flat = torch.zeros(M * K + 1, dtype=dtype, device=DEV)
        flat[1:] = xd.reshape(-1)
        xd = flat[1:].view(M, K)
    sat = 4 if M > 1 else 1  # (one row of 16: too few elements to clamp under half of them)
    scale = torch.tensor(FMT[fmt][1]) / x.float().abs().max() * sat
    state = Fp8DelayedState(1, device=DEV)
    state.set_scale(0, scale, fmt)
    _check_quantised(quantize_fp8(xd, fmt, transpose=True, scale=state.slot(0)), x, scale, fmt, state, sat)


def test_scale_update_against_the_torch_definition():
    """Three records in one launch, H = 3, five pushes: record 0 never has a producer (empty history: scale 1),
    record 1 sees an amax of 1e-40 (the quotient overflows: the 2^126 cap), record 2 (e5m2) wraps its ring."""
    pushes = [[3.0, 0.25], [7.0], [2.0, 1.5, 0.5], [1.0], [0.5]]
    states = [Fp8DelayedState(3, history=3, device=d) for d in ("cpu", DEV)]
    for st in states:
        st.bind(2, "e5m2")
    for vals in pushes:
        for st in states:
            for rec, v in ((1, [1e-40]), (2, vals)):
                st.partials[rec, 1:1 + len(v)] = torch.tensor(v).view(torch.int32).to(st.device)
                st.partials[rec, 0] = len(v)
            st.update()
        cpu, gpu = states
        for name in ("history", "scales", "pos", "partials"):
            assert torch.equal(getattr(cpu, name), getattr(gpu, name).cpu()), name
    assert gpu.scales[:, 0].tolist() == [1.0, 2.0 ** 126, 57344.0 / 2.0]  # the ring holds 2, 1, 0.5
    assert sorted(gpu.history[2].tolist()) == [0.5, 1.0, 2.0] and gpu.pos.tolist() == [0, 2, 2]


def test_delayed_equals_current_on_a_repeated_batch_gpu():
    check_delayed_equals_current(DEV)


def test_three_steps_against_the_cpu_definition():
    """The bound of test_fp8_gpu.py's MLP test (GPU against emulation): per tensor, with e_ref the error of the
    CPU definition of the same recipe against fp64 autograd of the unquantised model, the GPU's is <= 2 e_ref.
    Here at the third of three SGD steps."""
    r64 = recipe_steps("cpu", None, 3, lr=0.05, dtype=torch.float64)[-1]
    emu = recipe_steps("cpu", "delayed", 3, lr=0.05)[-1]
    gpu = recipe_steps(DEV, "delayed", 3, lr=0.05)[-1]
    for i, (r, e, c) in enumerate(zip(r64, emu, gpu)):
        e_ref, e_gpu = float((e - r).norm() / r.norm()), float((c - r).norm() / r.norm())
        print(f"tensor {i}: e_ref {e_ref:.4e}  gpu {e_gpu:.4e}")
        assert e_gpu <= 2.0 * e_ref, (i, e_ref, e_gpu)

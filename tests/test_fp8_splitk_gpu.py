"""The split-K instances of csrc/gemm_fp8.hip and csrc/gemm_mxfp8.hip and their reduction kernel, exactly:
operands on which fp32 arithmetic is exact in any order (fp8_cases.py), so every slicing of K must give the
table's expectation bit for bit.  One K-tile per slice, uneven slices, a ragged last slice, scale bytes
riding in slices with an offset, the reduction's element path, the plan taken by default, and the forced
combinations that must be refused."""
import pytest
import torch

from distributed_training_pytorch_amd import _native as nat
from distributed_training_pytorch_amd.ops.fp8 import gemm_fp8
from distributed_training_pytorch_amd.ops.mxfp8 import gemm_mxfp8

from . import fp8_cases as fc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FMTS = ["e4m3", "e5m2"]

# (M, N, K, epilogue, form, S)
FP8_SPLIT = [
    (16, 16, 384, "none", "fwd", 3),    # one K-tile per slice: sink and prologue of a 1-tile slice
    (272, 264, 400, "none", "fwd", 2),  # ragged M, N and a 16-byte K tail in the last slice only
    (272, 264, 400, "acc", "fwd", 3),   # uneven slices 1, 1, 2
    (272, 32, 392, "acc", "dw", 4),     # padded contraction 400; the last slice is a lone ragged tile
]
MX_SPLIT = [
    (256, 256, 416, "none", "fwd", 2),
    (272, 264, 2208, "acc", "fwd", 4),
    (288, 32, 392, "acc", "dw", 4),     # the MX_DW row, padded to 416
]


def _run(op, case, split_k, **extra):
    a, b, kw, want = case
    kw = dict(kw)
    if "out" in kw:
        kw["out"] = kw["out"].clone()
    got = op(a, b, split_k=split_k, **extra, **kw)
    assert torch.equal(got.cpu(), want), (split_k, float((got.cpu().double() - want.double()).abs().max()))


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("case", FP8_SPLIT, ids=fc.case_id)
def test_fp8_split_equals_the_exact_expectation(case, fmt_a):
    M, N, K, epi, form, S = case
    c = fc.fp8_case(M, N, K, fmt_a, epi, form, DEV)
    _run(gemm_fp8, c, S)
    _run(gemm_fp8, c, 1)  # the unsplit path is unchanged


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("case", MX_SPLIT, ids=fc.case_id)
def test_mxfp8_split_equals_the_exact_expectation(case, fmt_a):
    M, N, K, epi, form, S = case
    c = fc.mx_case(M, N, K, fmt_a, epi, form, DEV)
    _run(gemm_mxfp8, c, S, instance=1)
    _run(gemm_mxfp8, c, 1, instance=1)


@pytest.mark.parametrize("fmt_a", FMTS)
def test_mxfp8_scale_bytes_other_than_one_in_an_offset_slice(fmt_a):
    """sa = sb = 130 everywhere: a slice that read its scales at offset 0 of the row would still pass with
    drawn bytes only by luck; with 130 against the 127 past K every misplaced dword shows."""
    c = fc.mx_case(272, 264, 2208, fmt_a, "none", "fwd", DEV, sa=130, sb=130)
    _run(gemm_mxfp8, c, 4, instance=1)
    _run(gemm_mxfp8, c, 1, instance=1)


# ------------------------------------------------------------------------------ the reduction's element path
@pytest.mark.parametrize("fmt_a", FMTS)
def test_reduction_into_a_view_at_an_odd_element_offset(fmt_a):
    """A fused gradient target: a [272, 32] view from element 1 of a flat fp32 buffer (4-byte aligned only)."""
    a, A = fc.fp8_operand(272, 392, fmt_a, 11, fc.SA_INV, True, DEV)
    b, B = fc.fp8_operand(32, 392, "e4m3", 12, fc.SB_INV, True, DEV)
    flat = torch.full((1 + 272 * 32 + 3,), fc.PREFILL, device=DEV)
    view = flat[1:1 + 272 * 32].view(272, 32)
    assert view.data_ptr() % 16 == 4
    want = fc.expected((A @ B.t()) * (fc.SA_INV * fc.SB_INV) + fc.PREFILL, torch.float32)
    gemm_fp8(a, b, trans_a=True, trans_b=True, out=view, accumulate=True, split_k=4)
    assert torch.equal(view.cpu(), want)
    assert float(flat[0]) == fc.PREFILL and (flat[1 + 272 * 32:] == fc.PREFILL).all()


@pytest.mark.parametrize("fmt_a", FMTS)
def test_reduction_with_bias_and_n_not_a_multiple_of_4(fmt_a):
    M, N, K = 48, 30, 400
    a, A = fc.fp8_operand(M, K, fmt_a, 5, fc.SA_INV, False, DEV)
    b, B = fc.fp8_operand(N, K, "e4m3", 6, fc.SB_INV, False, DEV)
    bias = torch.arange(-15, 15, dtype=torch.float32)
    want = fc.expected((A @ B.t()) * (fc.SA_INV * fc.SB_INV) + bias.double(), torch.float32)
    got = gemm_fp8(a, b, bias=bias.to(DEV), out_dtype=torch.float32, split_k=3)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("which", ["fp8", "mxfp8"])
def test_the_plan_is_taken_by_default(which, fmt_a):
    """512 x 512, K = 4096: 4 tiles, 32 K-tiles -> the plan splits (4 slices of 8 at L = 8)."""
    M = N = 512
    K = 4096
    lib = nat.load()
    if which == "fp8":
        a, b, kw, want = fc.fp8_case(M, N, K, fmt_a, "none", "fwd", DEV)
        q, op, query = nat.GemmFp8Args(), gemm_fp8, lib.dtp_gemm_fp8_workspace
    else:
        a, b, kw, want = fc.mx_case(M, N, K, fmt_a, "none", "fwd", DEV)
        q, op, query = nat.GemmMxArgs(), gemm_mxfp8, lib.dtp_gemm_mxfp8_workspace
    q.M, q.N, q.K, q.out_dtype = M, N, K, nat.DT_F32
    assert query(q) == 4 * 4 * M * N
    planned, unsplit = op(a, b, **kw), op(a, b, split_k=1, **kw)
    assert torch.equal(planned, unsplit) and torch.equal(planned.cpu(), want)


# ------------------------------------------------------------------------------ what must be refused
@pytest.mark.parametrize("why,K,kw", [
    ("act", 400, dict(act=True, out_dtype=torch.float32)),
    ("bf16 out", 400, dict(out_dtype=torch.bfloat16)),
    ("mfma=1", 400, dict(out_dtype=torch.float32, mfma=1)),
    ("short K", 256, dict(out_dtype=torch.float32)),
    ("S > nk", 400, dict(out_dtype=torch.float32, split_k=5)),
])
def test_forced_split_is_refused(why, K, kw):
    a, _ = fc.fp8_operand(32, K, "e4m3", 1, fc.SA_INV, False, DEV)
    b, _ = fc.fp8_operand(32, K, "e4m3", 2, fc.SB_INV, False, DEV)
    with pytest.raises(ValueError):
        gemm_fp8(a, b, **{"split_k": 2, **kw})


def test_forced_split_on_the_mxfp8_short_k_instance_is_refused():
    am, _ = fc.mx_operand(32, 416, "e4m3", 1, False, DEV)
    bm, _ = fc.mx_operand(32, 416, "e4m3", 2, False, DEV)
    with pytest.raises(ValueError):  # K <= 2048 without instance = 1
        gemm_mxfp8(am, bm, out_dtype=torch.float32, split_k=2)

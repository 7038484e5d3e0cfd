"""The exact FP8 / MXFP8 tests' own ground, without a GPU: the fp64 model of the formats
(``fp8_cases.py``) against the byte tables, the torch definitions of both quantisers against that
model on the value tables (so "kernel == definition" and "definition == format" are both pinned),
the tiny-amax cases on the definition, and the exactness precondition of every GEMM case."""
import pytest
import torch

from distributed_training_pytorch_amd.ops.fp8 import gemm_fp8, quantize_fp8
from distributed_training_pytorch_amd.ops.mxfp8 import _quantize_def, gemm_mxfp8, quantize_mxfp8

from . import fp8_cases as fc

FMTS = ["e4m3", "e5m2"]
DTYPES = [torch.float32, torch.bfloat16]


# ------------------------------------------------------------------------------ the helpers themselves
@pytest.mark.parametrize("fmt", FMTS)
def test_format_model(fmt):
    v = fc.finite_values(fmt)
    assert len(v) == (127 if fmt == "e4m3" else 124)
    assert float(v[1]) == (2.0 ** -9 if fmt == "e4m3" else 2.0 ** -16) and float(v[-1]) == fc.FMT[fmt][1]
    # every byte decodes to itself and rounds to itself; -0 keeps its sign
    b = torch.cat([torch.arange(len(v)), 128 + torch.arange(len(v))]).to(torch.uint8)
    assert torch.equal(fc.ref_bytes(fc.decode_bytes(b, fmt), fmt), b)
    # ties go to the even byte, the nearest inputs on either side do not
    mid = (v[1:] + v[:-1]) / 2
    lo = torch.arange(len(v) - 1)
    assert torch.equal(fc.ref_bytes(mid, fmt).long(), lo + lo % 2)
    assert torch.equal(fc.ref_bytes(mid * (1 - 2.0 ** -30), fmt).long(), lo)
    assert torch.equal(fc.ref_bytes(-mid * (1 + 2.0 ** -30), fmt).long(), 128 + lo + 1)
    assert fc.ref_bytes(torch.tensor([1e9, -1e9]), fmt).tolist() == [len(v) - 1, 128 + len(v) - 1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_value_table_holds_what_it_claims(fmt, dtype):
    t, v = fc.value_table(fmt, dtype), fc.finite_values(fmt)
    have = set(t.tolist())
    mid = (v[1:] + v[:-1]) / 2
    assert all(x in have and -x in have for x in v[1:].tolist() + mid.tolist())
    ulp = 2.0 ** (-23 if dtype == torch.float32 else -7)
    for m in mid.tolist():  # the two inputs next to each tie, one ulp of the input dtype away
        near = sorted(x for x in have if 0 < abs(x - m) <= 1.01 * ulp * m)
        assert len(near) == 2 and near[0] < m < near[1], (m, near)
    assert 0.0 in have and torch.signbit(t[t == 0]).tolist() == [False, True]


# ------------------------------------------------------------------------------ A1: definition == format
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_per_tensor_definition_on_the_value_table(fmt, dtype):
    x = fc.per_tensor_table(fmt, dtype)
    q = quantize_fp8(x, fmt, transpose=True)
    want = fc.ref_bytes(x, fmt)
    assert float(q.scale) == 1.0 and float(q.scale_inv) == 1.0
    assert torch.equal(fc.fp8_bytes(q.data), want) and torch.equal(fc.fp8_bytes(q.data_t), want.t())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_mx_definition_on_the_value_table(fmt, dtype):
    x, s = fc.mx_table(fmt, dtype)
    want = fc.mx_table_reference(x, s, fmt)
    assert (want % 128).max() == len(fc.finite_values(fmt)) - 1  # fmax, and what lay past it
    q, scale = _quantize_def(x.float(), fmt)
    assert torch.equal(scale[:, :s.shape[1]], s) and torch.equal(fc.fp8_bytes(q), want)
    t = quantize_mxfp8(x.t().contiguous(), fmt, transpose=True)  # its transposed copy has the table's blocks again
    assert torch.equal(t.scale_t[:, :s.shape[1]], s) and (t.scale_t[:, s.shape[1]:] == 127).all()
    assert torch.equal(fc.fp8_bytes(t.data_t), want)


# ------------------------------------------------------------------------------ A2: the positions' derivation
def test_amax_positions_reach_the_workgroups_and_trips_they_name():
    shape = (2064, 2048)
    assert fc.amax_slot(shape, torch.float32, 0, 0) == (0, 0, 1024)
    wg, trip, grid = fc.amax_slot(shape, torch.float32, 2063, 2047)
    assert grid == 1024 and trip == 4  # the last element is read on a fifth trip
    for wg, trip in ((300, 0), (600, 1), (900, 2), (20, 4)):
        fc.amax_position(shape, torch.float32, wg, trip)
    assert fc.amax_slot((2064, 4096), torch.bfloat16, 2063, 4095)[1:] == (4, 1024)
    assert fc.amax_slot((1040, 1024), torch.float32, 1039, 1023) == (259, 3, 260)
    assert fc.amax_slot((1040, 2048), torch.bfloat16, 1039, 2047) == (259, 3, 260)


# ------------------------------------------------------------------------------ A5: tiny amax
@pytest.mark.parametrize("name", ["1e-37", "subnormal"])
@pytest.mark.parametrize("fmt", FMTS)
def test_tiny_amax_on_the_definition(fmt, name):
    """fmax / amax overflows fp32 below amax = fmax / FLT_MAX; uncapped, scale = inf, 1 / scale = 0
    and every element is 0 * inf = NaN.  The scale is capped at 2^126."""
    x = fc.tiny_inputs()[name]
    q = quantize_fp8(x, fmt, transpose=True)
    assert float(q.scale) == 2.0 ** 126 and float(q.scale_inv) == 2.0 ** -126
    fc.check_tiny(x, q, fmt)
    assert torch.equal(fc.fp8_bytes(q.data), fc.ref_bytes(x.double() * 2.0 ** 126, fmt))
    assert torch.equal(fc.fp8_bytes(q.data_t), fc.fp8_bytes(q.data).t())


def test_the_cap_leaves_every_other_scale_alone():
    for amax in (448.0 / 2.0 ** 126, 1e-30, 1.0, 3e38):
        x = torch.zeros(1, 16)
        x[0, 3] = -amax
        q = quantize_fp8(x, "e4m3")
        assert torch.equal(q.scale, torch.tensor(448.0) / torch.tensor(amax)) and float(q.scale) <= 2.0 ** 126


# ------------------------------------------------------------------------------ B: the GEMM cases are exact
@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("case", fc.all_fp8_cases(), ids=fc.case_id)
def test_fp8_gemm_cases_meet_the_exactness_precondition(case, fmt_a):
    M, N, K, epi, form, mfma = case
    a, b, kw, want = fc.fp8_case(M, N, K, fmt_a, epi, form)  # asserts the precondition
    assert want.shape == (M, N)
    if mfma == 0 and M * N * K <= 272 * 264 * 144:  # the CPU definition of the op on the same tuples
        assert torch.equal(gemm_fp8(a, b, **kw), want)


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("case", fc.all_mx_cases(), ids=fc.case_id)
def test_mx_gemm_cases_meet_the_exactness_precondition(case, fmt_a):
    M, N, K, epi, form, inst = case
    a, b, kw, want = fc.mx_case(M, N, K, fmt_a, epi, form)
    assert want.shape == (M, N)
    if inst == 0 and M * N * K <= 272 * 264 * 416:
        assert torch.equal(gemm_mxfp8(a, b, **kw), want)


@pytest.mark.parametrize("pair", fc.MX_SCALE_PAIRS, ids=fc.case_id)
@pytest.mark.parametrize("fmt_a", FMTS)
def test_mx_scale_range_cases_meet_the_exactness_precondition(pair, fmt_a):
    a, b, kw, want = fc.mx_case(64, 64, 128, fmt_a, "none", sa=pair[0], sb=pair[1])
    assert (a.scale == pair[0]).all() and (b.scale == pair[1]).all()
    assert torch.isfinite(want).all() and (want.abs()[want != 0] >= 2.0 ** -126).all()


@pytest.mark.parametrize("fmt_a", FMTS)
def test_mx_row_varying_scale_case_is_exact(fmt_a):
    a, b, kw, want = fc.mx_row_scale_case(fmt_a)  # asserts the precondition
    assert {0, 127, 130} <= set(a.scale[:16, 0].tolist()) and torch.equal(gemm_mxfp8(a, b, **kw), want)

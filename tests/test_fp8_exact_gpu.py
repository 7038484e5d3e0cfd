"""csrc/fp8_quant.hip and csrc/gemm_fp8.hip exactly, at their edges (cases and the fp64 model of the
formats: fp8_cases.py).  The quantiser byte for byte against the format's own rounding on a table of
every value, tie and near-tie; its reduction past 256 and at 1024 partials; its operand layouts and
its padding; a tensor whose amax underflows.  Every GEMM instance, the 16x16x32 one included, with
``torch.equal`` on operands where fp32 arithmetic is exact in any order.  The MLP function on the
pipelined kernels with adjacent FP8 layers and fused gradient targets.  The quantiser and the GEMM
replayed from one captured graph."""
import pytest
import torch

from distributed_training_pytorch_amd.ops.fp8 import gemm_fp8, quantize_fp8

from . import fp8_cases as fc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FMTS = ["e4m3", "e5m2"]
DTYPES = [torch.float32, torch.bfloat16]


def _same_as_definition(x_gpu, x_cpu, fmt):
    """Kernel == torch definition on the contiguous copy, bit for bit: scales, both copies, and zero
    bytes in the whole allocation behind data_t past M."""
    got, want = quantize_fp8(x_gpu, fmt, transpose=True), quantize_fp8(x_cpu, fmt, transpose=True)
    assert torch.equal(got.scale.cpu(), want.scale) and torch.equal(got.scale_inv.cpu(), want.scale_inv)
    assert torch.equal(fc.fp8_bytes(got.data), fc.fp8_bytes(want.data))
    M, K = x_cpu.shape
    Mp = -(-M // 16) * 16
    whole = fc.fp8_bytes(torch.as_strided(got.data_t, (K, Mp), (Mp, 1)))
    assert torch.equal(whole[:, :M], fc.fp8_bytes(want.data_t)) and not whole[:, M:].any()
    return got


# ------------------------------------------------------------------------------ A1: the value table
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_quantiser_on_the_value_table(fmt, dtype):
    x = fc.per_tensor_table(fmt, dtype)
    q = quantize_fp8(x.to(DEV), fmt, transpose=True)
    want = fc.ref_bytes(x, fmt)
    assert float(q.scale) == 1.0 and float(q.scale_inv) == 1.0
    got = fc.fp8_bytes(q.data)
    assert torch.equal(got, want), [(float(x[i, j]), int(got[i, j]), int(want[i, j])) for i, j in (got != want).nonzero()[:8]]
    assert torch.equal(fc.fp8_bytes(q.data_t), want.t())


# ------------------------------------------------------------------------------ A2: the reduction
_BIG = {}


def _big(shape, dtype):
    """randn clamped to |x| <= 1, made once per shape (the -7 is set and taken back by each test)."""
    if (shape, dtype) not in _BIG:
        g = torch.Generator().manual_seed(shape[0])
        _BIG[shape, dtype] = torch.randn(*shape, generator=g).clamp_(-1, 1).to(dtype)
    return _BIG[shape, dtype]


def _check_amax_at(shape, dtype, fmt, pos):
    x = _big(shape, dtype)
    old = x[pos].clone()
    x[pos] = -7.0
    try:
        got, want = quantize_fp8(x.to(DEV), fmt), quantize_fp8(x, fmt)
    finally:
        x[pos] = old
    fmax = fc.FMT[fmt][1]
    assert float(got.scale) == fmax / 7 and torch.equal(got.scale.cpu(), want.scale)  # 64 and 8192: exact
    assert torch.equal(got.data.view(torch.uint8), want.data.to(DEV).view(torch.uint8))


# amax_kernel at its cap: 1024 workgroups, 1,056,768 vectors, so 8192 of them are read on a fifth trip.
# quantize_kernel reads partial i in the pass i / 256 of its own loop: one position per pass
_F32_CAP = (2064, 2048)
_POS = {"first": (0, 0), "last": (2063, 2047), "wg300": (300, 0), "wg600_trip1": (600, 1), "wg900_trip2": (900, 2),
        "fifth_trip": (20, 4)}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("where", list(_POS))
def test_amax_reduction_at_the_workgroup_cap(where, fmt):
    pos = _POS[where] if where in ("first", "last") else fc.amax_position(_F32_CAP, torch.float32, *_POS[where])
    if where == "last":
        assert fc.amax_slot(_F32_CAP, torch.float32, *pos)[1] == 4
    _check_amax_at(_F32_CAP, torch.float32, fmt, pos)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape,dtype", [((1040, 1024), torch.float32), ((2064, 4096), torch.bfloat16)])
def test_amax_reduction_past_256_partials(shape, dtype, fmt):
    """260 partials (fp32): the only maximum sits in partial 259, the second pass of the loop.  bf16 at
    the cap: the only maximum is in workgroup 1023 on its last trip."""
    grid = fc.amax_slot(shape, dtype, 0, 0)[2]
    trips = -(-(shape[0] * shape[1] // (4 if dtype == torch.float32 else 8)) // (256 * grid))
    wg, trip = (259, 3) if grid == 260 else (1023, trips - 2)
    _check_amax_at(shape, dtype, fmt, fc.amax_position(shape, dtype, wg, trip))


# ------------------------------------------------------------------------------ A3 / A4: layouts and padding
@pytest.mark.parametrize("fmt", FMTS)
def test_bf16_input_that_is_only_2_byte_aligned(fmt):
    x = (3.0 * torch.randn(33, 48, generator=torch.Generator().manual_seed(1))).bfloat16()
    flat = torch.zeros(33 * 48 + 1, dtype=torch.bfloat16, device=DEV)
    flat[1:] = x.reshape(-1).to(DEV)
    v = flat[1:].view(33, 48)
    assert v.data_ptr() % 4 == 2
    _same_as_definition(v, x, fmt)


# [33, 52]: fp32 rows stay 16-byte aligned (vector loads, ldx > K), bf16 rows do not (element loads);
# [33, 56]: vector loads for both; [33, 50]: element loads for both
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [52, 56, 50])
def test_row_strided_input(width, dtype, fmt):
    big = (3.0 * torch.randn(33, width, generator=torch.Generator().manual_seed(width))).to(dtype)
    big[:, 48:] = 1e6  # never to be read: it would change the scale
    v = big.to(DEV)[:, :48]
    assert v.stride() == (width, 1)
    _same_as_definition(v, big[:, :48].contiguous(), fmt)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 16), (17, 64), (65, 80), (130, 272)])  # M % 16 != 0, tile rows 1 / 17 / 1 / 2
def test_transposed_copy_is_zero_past_m(shape, dtype, fmt):
    x = (3.0 * torch.randn(*shape, generator=torch.Generator().manual_seed(shape[0]))).to(dtype)
    torch.full((1 << 20,), 0x3c3c3c3c, dtype=torch.int32, device=DEV)  # leave no fresh zeros for the allocator
    _same_as_definition(x.to(DEV), x, fmt)


# ------------------------------------------------------------------------------ A5: tiny amax
@pytest.mark.parametrize("name", ["1e-37", "subnormal"])
@pytest.mark.parametrize("fmt", FMTS)
def test_tiny_amax(fmt, name):
    """An amax below fmax / FLT_MAX: uncapped, scale = inf, 1 / scale = 0, every element NaN."""
    x = fc.tiny_inputs()[name]
    got = _same_as_definition(x.to(DEV), x, fmt)
    fc.check_tiny(x, got, fmt)


# ------------------------------------------------------------------------------ B: exact GEMMs
def _run(case, fmt_a, **opt):
    M, N, K, epi, form, mfma = case
    a, b, kw, want = fc.fp8_case(M, N, K, fmt_a, epi, form, device=DEV)
    got = gemm_fp8(a, b, mfma=mfma, **kw, **opt).cpu()
    bad = (got != want).nonzero()
    assert got.dtype == want.dtype and torch.equal(got, want), (len(bad), [(i, j, float(got[i, j]), float(want[i, j]))
                                                                       for i, j in bad[:6].tolist()])


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("case", fc.all_fp8_cases(), ids=fc.case_id)
def test_gemm_fp8_is_exact(case, fmt_a):
    """K <= 256 on the short-K instance, past it the pipelined one with either matrix instruction
    (mfma: the last field).  Within one instruction the products span 2 bits, far inside what the FP8
    matrix unit keeps, so the pipelined kernels must be exact too."""
    _run(case, fmt_a)


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("mfma,K", [(0, 144), (0, 400), (1, 400)])
@pytest.mark.parametrize("layout", ["offset1", "sliced"])
def test_gemm_fp8_output_layouts(layout, mfma, K, fmt_a):
    """C as the view at element 1 of a flat fp32 buffer (a fused gradient target: 4-byte aligned,
    ldc = N), and C and aux as column slices of wider tensors.  The bytes around them stay."""
    M, N = 272, 264
    if layout == "offset1":
        a, b, kw, want = fc.fp8_case(M, N, K, fmt_a, "acc", device=DEV)
        flat = torch.full((M * N + 2,), 1234.5, device=DEV)
        out = flat[1:1 + M * N].view(M, N)
        out.copy_(kw["out"])
        kw["out"] = out
        gemm_fp8(a, b, mfma=mfma, **kw)
        assert torch.equal(out.cpu(), want) and float(flat[0]) == 1234.5 and float(flat[-1]) == 1234.5
    else:
        a, b, kw, want = fc.fp8_case(M, N, K, fmt_a, "aux", device=DEV)
        wide_c = torch.full((M, N + 9), 77.0, dtype=torch.bfloat16, device=DEV)
        wide_aux = torch.full((M, N + 5), -1.0, dtype=torch.bfloat16, device=DEV)
        wide_aux[:, 3:3 + N] = kw["aux"]
        kw.update(aux=wide_aux[:, 3:3 + N], out=wide_c[:, 4:4 + N])
        gemm_fp8(a, b, mfma=mfma, **kw)
        assert torch.equal(wide_c[:, 4:4 + N].cpu(), want)
        assert (wide_c[:, :4] == 77.0).all() and (wide_c[:, 4 + N:] == 77.0).all()


# ------------------------------------------------------------------------------ D: the MLP function
@pytest.fixture(scope="module")
def mlp_refs():
    """fp64 autograd and the CPU emulation of the model, computed once."""
    params, x, gy = fc.mlp_model((16, 272, 288, 16), 264)
    r64 = fc.mlp_autograd(params, x, gy, 0.01, "cpu", torch.float64, None)
    emu = fc.mlp_autograd(params, x, gy, 0.01, "cpu", torch.float32, torch.float8_e4m3fn)
    return params, x, gy, r64, emu


@pytest.mark.parametrize("fused", [False, True])
def test_mlp_fp8_on_the_pipelined_kernels(mlp_refs, fused):
    """Widths (16, 272, 288, 16), batch 264: every layer is FP8, layers 1 and 2 adjacent (dz is
    quantised again), forward K = 272 and 288, dx K = 288 and dW K = 264 -> 272 on the pipelined kernel,
    the rest on the short one.  Per tensor e_gpu <= 2 e_ref (test_fp8_gpu.py); with fused gradient
    targets (views of a flat buffer at element 1, prefilled) the targets hold prefill + gradient and
    every parameter's ready-hook fires once.  Measured (e_ref, plain, fused): see
    profiles/fp8_gemm/README.md."""
    params, x, gy, r64, emu = mlp_refs
    if fused:
        got, calls = fc.mlp_fused(params, x, gy, 0.01, DEV, torch.float8_e4m3fn)
        assert calls == [1] * len(params), calls
    else:
        got = fc.mlp_autograd(params, x, gy, 0.01, DEV, torch.float32, torch.float8_e4m3fn)
    rows = fc.error_rows(r64, emu, got)
    for n, e_ref, e_gpu in rows:
        print(f"fp8 fused={int(fused)} {n:>4}: e_ref {e_ref:.4e}  gpu {e_gpu:.4e}")
    for n, e_ref, e_gpu in rows:
        assert e_gpu <= 2.0 * e_ref, (n, e_ref, e_gpu)


# ------------------------------------------------------------------------------ E: graph capture
@pytest.mark.parametrize("shape", [(80, 144), (272, 400)])
def test_quantiser_and_gemm_replay_from_a_captured_graph(shape):
    """Nothing in the pair of quantiser launches or the GEMM reads the GPU back: captured once, they
    follow new data (and its new amax) on every replay, bitwise as an eager run."""
    M, K = shape
    g = torch.Generator().manual_seed(M)
    w = quantize_fp8(torch.randn(64, K, generator=g).to(DEV), "e4m3")
    xs = [(s * torch.randn(M, K, generator=g)).to(DEV) for s in (1.0, 37.0, 1e-3, 5.0)]
    x = xs[0].clone()

    def step():
        q = quantize_fp8(x, "e4m3", transpose=True)
        return q, gemm_fp8(q, w, out_dtype=torch.float32)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        q, c = step()
    for new in xs[1:]:
        x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eq, ec = quantize_fp8(new, "e4m3", transpose=True), None
        ec = gemm_fp8(eq, w, out_dtype=torch.float32)
        assert torch.equal(q.scale, eq.scale) and torch.equal(q.scale_inv, eq.scale_inv)
        assert torch.equal(q.data.view(torch.uint8), eq.data.view(torch.uint8))
        assert torch.equal(q.data_t.view(torch.uint8), eq.data_t.view(torch.uint8)) and torch.equal(c, ec)

"""csrc/mxfp8_quant.hip and csrc/gemm_mxfp8.hip exactly, at their edges (cases and the fp64 model of
the formats: fp8_cases.py).  The quantiser byte for byte against the format's own rounding on a table
of every value, tie and near-tie under two scale bytes; its operand layouts and its padding.  Both GEMM
instances with ``torch.equal`` on operands where fp32 arithmetic is exact in any order, default
dispatch and forced, and at the extreme E8M0 bytes.  The MLP function around K = 2048 with adjacent MX
layers and fused gradient targets.  The quantiser and the GEMM replayed from one captured graph."""
import pytest
import torch

from distributed_training_pytorch_amd.ops.mxfp8 import gemm_mxfp8, quantize_mxfp8

from . import fp8_cases as fc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FMTS = ["e4m3", "e5m2"]
DTYPES = [torch.float32, torch.bfloat16]
NAMES = ("scale", "data", "scale_t", "data_t")


def _same_as_definition(x_gpu, x_cpu, fmt):
    """Kernel == torch definition on the contiguous copy, bit for bit, all four arrays whole: zero
    bytes in data_t past M, byte 127 in both scale arrays past the live blocks."""
    got, want = quantize_mxfp8(x_gpu, fmt, transpose=True), quantize_mxfp8(x_cpu, fmt, transpose=True)
    for name in NAMES:
        w, g = fc.fp8_bytes(getattr(want, name)), fc.fp8_bytes(getattr(got, name))
        assert w.shape == g.shape and torch.equal(w, g), (name, (w != g).nonzero()[:8].tolist())
    M, K = x_cpu.shape
    Mp = -(-M // 32) * 32
    assert not fc.fp8_bytes(got.data_t)[:, M:].any()
    assert (got.scale[:, K // 32:] == 127).all() and (got.scale_t[:, Mp // 32:] == 127).all()
    return got


# ------------------------------------------------------------------------------ A1: the value table
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_quantiser_on_the_value_table(fmt, dtype):
    x, s = fc.mx_table(fmt, dtype)
    want = fc.mx_table_reference(x, s, fmt)
    q = quantize_mxfp8(x.to(DEV), fmt)
    got = fc.fp8_bytes(q.data)
    assert torch.equal(q.scale.cpu()[:, :s.shape[1]], s)
    assert torch.equal(got, want), [(float(x[i, j]), int(got[i, j]), int(want[i, j])) for i, j in (got != want).nonzero()[:8]]
    t = quantize_mxfp8(x.t().contiguous().to(DEV), fmt, transpose=True)  # the table's blocks down the columns
    assert torch.equal(t.scale_t.cpu()[:, :s.shape[1]], s) and (t.scale_t[:, s.shape[1]:] == 127).all()
    assert torch.equal(fc.fp8_bytes(t.data_t), want)


# ------------------------------------------------------------------------------ A3 / A4: layouts and padding
def _mx_randn(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    j = torch.randint(-6, 7, (M, K // 32), generator=g)
    return torch.randn(M, K, generator=g) * torch.exp2(j.float()).repeat_interleave(32, dim=1)


@pytest.mark.parametrize("fmt", FMTS)
def test_bf16_input_that_is_only_2_byte_aligned(fmt):
    x = _mx_randn(33, 64, 1).bfloat16()
    flat = torch.zeros(33 * 64 + 1, dtype=torch.bfloat16, device=DEV)
    flat[1:] = x.reshape(-1).to(DEV)
    v = flat[1:].view(33, 64)
    assert v.data_ptr() % 4 == 2
    _same_as_definition(v, x, fmt)


# K must be a whole number of MX blocks, so the views are 64 wide: of [33, 68] fp32 rows stay 16-byte
# aligned (vector loads, ldx > K) and bf16 rows do not; of [33, 72] both do; of [33, 66] neither does
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [68, 72, 66])
def test_row_strided_input(width, dtype, fmt):
    big = torch.full((33, width), 1e6)  # the columns past 64 are never to be read
    big[:, :64] = _mx_randn(33, 64, width)
    big = big.to(dtype)
    v = big.to(DEV)[:, :64]
    assert v.stride() == (width, 1)
    _same_as_definition(v, big[:, :64].contiguous(), fmt)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 32), (33, 160), (65, 128), (130, 288)])  # M % 32 != 0
def test_padding_of_every_array(shape, dtype, fmt):
    x = _mx_randn(*shape, shape[0]).to(dtype)
    torch.full((1 << 20,), 0x3c3c3c3c, dtype=torch.int32, device=DEV)  # leave no fresh zeros for the allocator
    _same_as_definition(x.to(DEV), x, fmt)


# ------------------------------------------------------------------------------ B: exact GEMMs
def _assert_equal(got, want):
    got = got.cpu()
    bad = (got != want).nonzero()
    assert got.dtype == want.dtype and torch.equal(got, want), (len(bad), [(i, j, float(got[i, j]), float(want[i, j]))
                                                                       for i, j in bad[:6].tolist()])


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("case", fc.all_mx_cases(), ids=fc.case_id)
def test_gemm_mxfp8_is_exact(case, fmt_a):
    """Scale bytes 126 .. 128 drawn per (row, block): K <= 2048 on the short instance, past it the
    pipelined one, and each forced onto the other's K (instance: the last field).  Within one matrix
    instruction the products span 6 bits, 2 from the data and 4 from the scales, inside what the
    block-scaled MFMA keeps, so the pipelined kernel must be exact too."""
    M, N, K, epi, form, inst = case
    a, b, kw, want = fc.mx_case(M, N, K, fmt_a, epi, form, device=DEV)
    _assert_equal(gemm_mxfp8(a, b, instance=inst, **kw), want)


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("inst", [1, 2])
@pytest.mark.parametrize("pair", fc.MX_SCALE_PAIRS, ids=fc.case_id)
def test_gemm_mxfp8_at_the_extreme_scale_bytes(pair, inst, fmt_a):
    """All of A's bytes sa, all of B's sb: the result is the integer product times 2^(sa + sb - 254), a
    normal number, whatever the two factors are alone (2^-127 is a subnormal, 2^127 times an element
    of 2 is past fp32).  The quantiser writes byte 0 for a block below 2^-119 and nothing past 246."""
    a, b, kw, want = fc.mx_case(64, 64, 128, fmt_a, "none", device=DEV, sa=pair[0], sb=pair[1])
    _assert_equal(gemm_mxfp8(a, b, instance=inst, **kw), want)


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("inst", [1, 2])
def test_gemm_mxfp8_with_extreme_bytes_that_differ_from_row_to_row(inst, fmt_a):
    """What the quantiser does write: a row whose block has underflowed (byte 0) between rows at 127
    and above, in every 16-row fragment of A, against B rows at 128, 135 and 240.  Each operand's
    scale must hold on its own, whatever its neighbours carry."""
    a, b, kw, want = fc.mx_row_scale_case(fmt_a, device=DEV)
    _assert_equal(gemm_mxfp8(a, b, instance=inst, **kw), want)


@pytest.mark.parametrize("fmt_a", FMTS)
@pytest.mark.parametrize("K", [416, 2208])  # the short and the pipelined instance
@pytest.mark.parametrize("layout", ["offset1", "sliced"])
def test_gemm_mxfp8_output_layouts(layout, K, fmt_a):
    """C as the view at element 1 of a flat fp32 buffer (a fused gradient target: 4-byte aligned,
    ldc = N), and C and aux as column slices of wider tensors.  The bytes around them stay."""
    M, N = 272, 264
    if layout == "offset1":
        a, b, kw, want = fc.mx_case(M, N, K, fmt_a, "acc", device=DEV)
        flat = torch.full((M * N + 2,), 1234.5, device=DEV)
        out = flat[1:1 + M * N].view(M, N)
        out.copy_(kw["out"])
        kw["out"] = out
        gemm_mxfp8(a, b, **kw)
        _assert_equal(out, want)
        assert float(flat[0]) == 1234.5 and float(flat[-1]) == 1234.5
    else:
        a, b, kw, want = fc.mx_case(M, N, K, fmt_a, "aux", device=DEV)
        wide_c = torch.full((M, N + 9), 77.0, dtype=torch.bfloat16, device=DEV)
        wide_aux = torch.full((M, N + 5), -1.0, dtype=torch.bfloat16, device=DEV)
        wide_aux[:, 3:3 + N] = kw["aux"]
        kw.update(aux=wide_aux[:, 3:3 + N], out=wide_c[:, 4:4 + N])
        gemm_mxfp8(a, b, **kw)
        _assert_equal(wide_c[:, 4:4 + N], want)
        assert (wide_c[:, :4] == 77.0).all() and (wide_c[:, 4 + N:] == 77.0).all()


# ------------------------------------------------------------------------------ D: the MLP function
@pytest.fixture(scope="module")
def mlp_refs():
    """fp64 autograd and the CPU emulation of the model, computed once."""
    params, x, gy = fc.mlp_model((32, 2080, 2112, 32), 2056)
    r64 = fc.mlp_autograd(params, x, gy, 0.01, "cpu", torch.float64, None)
    emu = fc.mlp_autograd(params, x, gy, 0.01, "cpu", torch.float32, torch.float8_e8m0fnu)
    return params, x, gy, r64, emu


@pytest.mark.parametrize("fused", [False, True])
def test_mlp_mxfp8_around_k_2048(mlp_refs, fused):
    """Widths (32, 2080, 2112, 32), batch 2056: every layer is MX, layers 1 and 2 adjacent (dz is
    quantised again), forward K = 2080 and 2112, dx K = 2112 and dW K = 2056 -> 2080 on the pipelined
    kernel, the rest on the short one.  Per tensor e_gpu <= 2 e_ref (test_mxfp8_gpu.py); with fused
    gradient targets (views of a flat buffer at element 1, prefilled) the targets hold prefill +
    gradient and every parameter's ready-hook fires once.  Measured: profiles/mxfp8/README.md."""
    params, x, gy, r64, emu = mlp_refs
    if fused:
        got, calls = fc.mlp_fused(params, x, gy, 0.01, DEV, torch.float8_e8m0fnu)
        assert calls == [1] * len(params), calls
    else:
        got = fc.mlp_autograd(params, x, gy, 0.01, DEV, torch.float32, torch.float8_e8m0fnu)
    rows = fc.error_rows(r64, emu, got)
    for n, e_ref, e_gpu in rows:
        print(f"mxfp8 fused={int(fused)} {n:>4}: e_ref {e_ref:.4e}  gpu {e_gpu:.4e}")
    for n, e_ref, e_gpu in rows:
        assert e_gpu <= 2.0 * e_ref, (n, e_ref, e_gpu)


# ------------------------------------------------------------------------------ E: graph capture
@pytest.mark.parametrize("shape", [(96, 160), (272, 2208)])
def test_quantiser_and_gemm_replay_from_a_captured_graph(shape):
    """The quantiser launch and the GEMM read nothing back: captured once, they follow new data on
    every replay, bitwise as an eager run."""
    M, K = shape
    g = torch.Generator().manual_seed(M)
    w = quantize_mxfp8(torch.randn(64, K, generator=g).to(DEV), "e4m3")
    xs = [(s * torch.randn(M, K, generator=g)).to(DEV) for s in (1.0, 37.0, 1e-3, 5.0)]
    x = xs[0].clone()

    def step():
        q = quantize_mxfp8(x, "e4m3", transpose=True)
        return q, gemm_mxfp8(q, w, out_dtype=torch.float32)

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
        eq = quantize_mxfp8(new, "e4m3", transpose=True)
        ec = gemm_mxfp8(eq, w, out_dtype=torch.float32)
        for name in NAMES:
            assert torch.equal(getattr(q, name).view(torch.uint8), getattr(eq, name).view(torch.uint8)), name
        assert torch.equal(c, ec)

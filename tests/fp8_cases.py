"""Shared cases of the exact FP8 / MXFP8 tests (test_fp8_exact_cpu.py, test_fp8_exact_gpu.py,
test_mxfp8_exact_gpu.py): an fp64 model of the two OCP formats that does not use torch's cast, the
value tables that visit every rounding decision, and GEMM operands on which fp32 arithmetic is
exact in any order, so a kernel is compared with ``torch.equal``."""
import math

import torch

from distributed_training_pytorch_amd.ops.fp8 import Fp8Tensor
from distributed_training_pytorch_amd.ops.mxfp8 import MxTensor

FMT = {  # torch dtype, fmax, emax (of 2^emax <= fmax), exponent bits, mantissa bits, bias
    "e4m3": (torch.float8_e4m3fn, 448.0, 8, 4, 3, 7),
    "e5m2": (torch.float8_e5m2, 57344.0, 15, 5, 2, 15),
}
OVER = {"e4m3": [464.0, 480.0, 500.0, 511.0], "e5m2": [60000.0, 61440.0, 65280.0, 65535.0]}  # in (fmax, 2 * 2^emax)


# ------------------------------------------------------------------------------ the formats, in fp64
def finite_values(fmt: str) -> torch.Tensor:
    """The non-negative finite values of the format in byte order (entry i is byte i), by the OCP
    formula: 2^(e - bias) (1 + m / 2^mb) for an exponent field e > 0, 2^(1 - bias) m / 2^mb for e = 0.
    e4m3 has no infinity and one NaN mantissa (S.1111.111); e5m2 gives up its whole top exponent."""
    _, fmax, _, eb, mb, bias = FMT[fmt]
    vals = []
    for byte in range(128):
        e, m = byte >> mb, byte & ((1 << mb) - 1)
        if fmt == "e4m3" and byte == 0x7f:
            break
        if fmt == "e5m2" and e == (1 << eb) - 1:
            break
        vals.append(2.0 ** (e - bias) * (1 + m / 2 ** mb) if e else 2.0 ** (1 - bias) * m / 2 ** mb)
    v = torch.tensor(vals, dtype=torch.float64)
    assert v[-1] == fmax and (v[1:] > v[:-1]).all()
    return v


def ref_bytes(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """Round to nearest, ties to the even byte, saturating at fmax; the sign bit is the input's
    (so -0 and a negative value that rounds to zero are byte 0x80).  ``x`` finite, any shape."""
    v = finite_values(fmt)
    x = x.double()
    a = x.abs().clamp(max=float(v[-1]))
    hi = torch.searchsorted(v, a).clamp(max=len(v) - 1)  # first value >= a
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - v[lo], v[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    byte = torch.where(pick_hi, hi, lo)
    return (byte + 128 * torch.signbit(x).long()).to(torch.uint8)


def decode_bytes(b: torch.Tensor, fmt: str) -> torch.Tensor:
    """fp64 values of FP8 bytes (finite ones only)."""
    v = finite_values(fmt)
    b = b.long()
    return torch.where(b >= 128, -1.0, 1.0) * v[b % 128]


def fp8_bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------ A1: the value table
def _ulp_neighbours(x: torch.Tensor, dtype: torch.dtype):
    """The next value of ``dtype`` below and above each positive ``x`` (x exact in dtype)."""
    it = torch.int32 if dtype == torch.float32 else torch.int16
    bits = x.to(dtype).view(it)
    return (bits - 1).view(dtype).double(), (bits + 1).view(dtype).double()


def value_table(fmt: str, dtype: torch.dtype) -> torch.Tensor:
    """Every finite value of the format, every midpoint between neighbours (the ties), each midpoint
    -+ one ulp of ``dtype`` (the nearest inputs that are no tie), half the smallest subnormal (the
    first midpoint) with its two neighbours, all of them in both signs, +-0 and fmax: a 1-D fp64
    tensor of values that ``dtype`` holds exactly.  A midpoint needs one mantissa bit more than the
    format, at most 5, so bf16 (8) keeps all of them; its ulp neighbours are bf16's own."""
    v = finite_values(fmt)
    mid = (v[1:] + v[:-1]) / 2
    below, above = _ulp_neighbours(mid, dtype)
    pos = torch.cat([v[1:], mid, below, above])
    t = torch.cat([pos, -pos, torch.tensor([0.0, -0.0], dtype=torch.float64)])
    assert torch.equal(t.to(dtype).double(), t), "table entries must be exact in the input dtype"
    assert (below < mid).all() and (above > mid).all() and float(mid[0]) == float(v[1]) / 2
    return t


def per_tensor_table(fmt: str, dtype: torch.dtype, rows: int = 5) -> torch.Tensor:
    """[rows, K] of ``dtype``, K a multiple of 16: the table, zero-padded, rotated by 21 r columns in
    row r so that the 64 x 64 tile meets every entry at several (row, column) positions.  Its amax is
    fmax, so the scale is exactly 1."""
    t = value_table(fmt, dtype)
    K = -(-len(t) // 16) * 16
    row = torch.zeros(K, dtype=torch.float64)
    row[:len(t)] = t
    return torch.stack([row.roll(21 * r) for r in range(rows)]).to(dtype)


def mx_table(fmt: str, dtype: torch.dtype, rows: int = 32):
    """([rows, K] of ``dtype``, the expected scale byte per 32-block [K / 32]): 32-blocks of 31 table
    entries (and the values past fmax, which must come out as fmax) with fmax in slot 31, scale byte
    127, each followed by a copy times 2^-3, scale byte 124 and the same FP8 bytes.  Row r is rotated
    by 5 r blocks.  ``rows`` = 32 lets the transpose of the table be quantised too (its transposed
    copy has these blocks again)."""
    _, fmax, _, _, _, _ = FMT[fmt]
    over = torch.tensor(OVER[fmt], dtype=torch.float64)
    over = over[over.to(dtype).double() == over]
    t = torch.cat([value_table(fmt, dtype), over, -over])
    nb = -(-len(t) // 31)
    body = torch.zeros(nb * 31, dtype=torch.float64)
    body[:len(t)] = t
    blocks = torch.cat([body.view(nb, 31), torch.full((nb, 1), fmax, dtype=torch.float64)], dim=1)
    both = torch.stack([blocks, blocks * 2.0 ** -3], dim=1).reshape(2 * nb, 32)
    sbyte = torch.tensor([127, 124] * nb, dtype=torch.uint8)
    x = torch.stack([both.roll(5 * r, 0).reshape(-1) for r in range(rows)])
    s = torch.stack([sbyte.roll(5 * r) for r in range(rows)])
    assert torch.equal(x.to(dtype).double(), x)
    return x.to(dtype), s


def mx_table_reference(x: torch.Tensor, s: torch.Tensor, fmt: str) -> torch.Tensor:
    """Bytes of the MX table: each block divided by its expected scale, then the format's rounding."""
    mul = torch.exp2(127.0 - s.double()).repeat_interleave(32, dim=1)
    return ref_bytes(x.double() * mul, fmt)


# ------------------------------------------------------------------------------ A2: the reduction
def amax_slot(shape, dtype: torch.dtype, row: int, col: int):
    """(workgroup, trip) of amax_kernel that reads element (row, col) of a contiguous x:
    vector v = blockIdx * 256 + tid + 256 * gridDim * trip, gridDim = min(1024, ceil(vectors / 1024))."""
    M, K = shape
    epv = 4 if dtype == torch.float32 else 8
    vecs = M * (K // epv)
    grid = min(1024, -(-vecs // 1024))
    v = row * (K // epv) + col // epv
    trip, rest = divmod(v, 256 * grid)
    return rest // 256, trip, grid


def amax_position(shape, dtype: torch.dtype, wg: int, trip: int, tid: int = 37, lane_elem: int = 2):
    """(row, col) of an element that workgroup ``wg`` reads on trip ``trip``."""
    M, K = shape
    epv = 4 if dtype == torch.float32 else 8
    grid = min(1024, -(-(M * (K // epv)) // 1024))
    v = wg * 256 + tid + 256 * grid * trip
    assert wg < grid and v < M * (K // epv)
    row, c = divmod(v, K // epv)
    pos = (row, c * epv + lane_elem)
    assert amax_slot(shape, dtype, *pos)[:2] == (wg, trip)
    return pos


# ------------------------------------------------------------------------------ A5: tiny amax
def tiny_inputs():
    """name -> fp32 [33, 48], mostly exact zeros: a largest magnitude of 1e-37 (fmax / amax overflows
    fp32 in both formats) and one that is an fp32 subnormal."""
    out = {}
    for name, big in (("1e-37", 1e-37), ("subnormal", 2.0 ** -130)):
        x = torch.zeros(33, 48)
        x[0, 0], x[3, 17], x[20, 5], x[32, 47], x[9, 9] = big, -big, 0.3 * big, -0.011 * big, 0.75 * big
        assert float(x.abs().max()) == float(torch.tensor(big)) and (x != 0).sum() == 5
        out[name] = x
    assert float(out["subnormal"].abs().max()) < 2.0 ** -126
    return out


def check_tiny(x: torch.Tensor, q: Fp8Tensor, fmt: str) -> None:
    """Finite output and scales, zeros stay zero, and the dequantised value within half an FP8 step
    of x wherever x * scale is in the format's normal range."""
    _, fmax, _, _, mb, bias = FMT[fmt]
    scale, scale_inv = q.scale.cpu().double(), q.scale_inv.cpu().double()
    data = q.data.cpu().double()
    assert torch.isfinite(scale) and torch.isfinite(scale_inv) and scale_inv > 0 and torch.isfinite(data).all()
    assert not data[x == 0].any()
    y = x.double() * scale
    normal = y.abs() >= 2.0 ** (1 - bias)
    assert normal.any() and (y.abs() <= fmax).all()
    step = torch.exp2(torch.floor(torch.log2(y.abs()[normal])) - mb)
    assert ((data[normal] - y[normal]).abs() <= step / 2).all()
    assert ((data[normal] * scale_inv - x.double()[normal]).abs() <= step / 2 * scale_inv).all()


# ------------------------------------------------------------------------------ B: exact GEMM operands
ALPHABET = (-2, -1, 0, 1, 2)  # exact in e4m3 and in e5m2
SA_INV, SB_INV = 2.0 ** -3, 2.0 ** 5
SLOPE = 0.5
EPIS = ("none", "bias_act", "aux", "acc")


def _ints(rows, cols, seed, alphabet=ALPHABET):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(alphabet, dtype=torch.int64)[torch.randint(0, len(alphabet), (rows, cols), generator=g)]


def _padded(vals: torch.Tensor, pad: int):
    """[rows, K] int -> ([rows, Kp] int with zeros past K, Kp)."""
    rows, K = vals.shape
    Kp = -(-K // pad) * pad
    full = torch.zeros(rows, Kp, dtype=vals.dtype)
    full[:, :K] = vals
    return full, Kp


def fp8_operand(rows, K, fmt, seed, scale_inv, transposed, device="cpu", alphabet=ALPHABET):
    """(Fp8Tensor, decoded fp64 [rows, K] without the scale).  ``transposed``: the operand is a
    ``data_t``, a [rows, K] view of rows zero-padded to a multiple of 16, as the quantiser lays it out."""
    vals = _ints(rows, K, seed, alphabet)
    dtype = FMT[fmt][0]
    si = torch.tensor(scale_inv, dtype=torch.float32, device=device)
    if transposed:
        full, _ = _padded(vals, 16)
        d = full.float().to(dtype).to(device)[:, :K]
        return Fp8Tensor(None, d, None, si, fmt), vals.double()
    assert K % 16 == 0
    return Fp8Tensor(vals.float().to(dtype).to(device), None, None, si, fmt), vals.double()


def mx_operand(rows, K, fmt, seed, transposed, device="cpu", alphabet=ALPHABET, sbytes=(126, 127, 128)):
    """(MxTensor, dequantised fp64 [rows, Kp]).  Scale bytes drawn per (row, 32-block) from ``sbytes``,
    127 in the columns past the live blocks.  ``transposed``: a ``data_t`` / ``scale_t`` pair, the
    contraction zero-padded to whole blocks (the last block ragged), scales along the padded length."""
    vals = _ints(rows, K, seed, alphabet)
    full, Kp = _padded(vals, 32)
    assert transposed or Kp == K
    g = torch.Generator().manual_seed(seed + 1000)
    live = Kp // 32
    s = torch.full((rows, 4 * (-(-Kp // 128))), 127, dtype=torch.uint8)
    s[:, :live] = torch.tensor(sbytes, dtype=torch.uint8)[torch.randint(0, len(sbytes), (rows, live), generator=g)]
    dtype = FMT[fmt][0]
    d = full.float().to(dtype).to(device)
    deq = full.double() * torch.exp2(s[:, :live].double() - 127.0).repeat_interleave(32, dim=1)
    t = MxTensor(None, None, d, s.to(device), fmt) if transposed else MxTensor(d, s.to(device), None, None, fmt)
    return t, deq


def epilogue(lin: torch.Tensor, epi: str, seed: int):
    """(fp64 expectation, gemm keyword arguments on the CPU, the |bias| / |old C| magnitude, the
    exponent the epilogue takes off the granule).  Bias and old C integer-valued, aux of random sign,
    slope 0.5: every step stays exact."""
    M, N = lin.shape
    g = torch.Generator().manual_seed(seed + 77)
    if epi == "none":
        return lin, dict(out_dtype=torch.float32), torch.zeros_like(lin), 0
    if epi == "bias_act":
        bias = torch.randint(-8, 9, (N,), generator=g).float()
        return (torch.nn.functional.leaky_relu(lin + bias.double(), SLOPE), dict(bias=bias, act=True, slope=SLOPE,
                out_dtype=torch.bfloat16), bias.abs().double().expand(M, N), 1)
    if epi == "aux":
        aux = torch.randn(M, N, generator=g).bfloat16()
        return (lin * torch.where(aux.double() > 0, 1.0, SLOPE), dict(aux=aux, slope=SLOPE, out_dtype=torch.bfloat16),
                torch.zeros_like(lin), 1)
    assert epi == "acc"
    old = torch.randint(-64, 65, (M, N), generator=g).float()
    return lin + old.double(), dict(out=old, accumulate=True, out_dtype=torch.float32), old.abs().double(), 0


def check_exactness_precondition(ref: torch.Tensor, mag: torch.Tensor, g: int) -> None:
    """Every value the kernel can form (any partial sum, in any order, the epilogue's steps) is a
    multiple of 2^g and below 2^(24 + g) in magnitude: exact in fp32."""
    assert torch.isfinite(ref).all() and g >= -126 and 24 + g <= 127  # (multiples of 2^g >= 2^-126: normal numbers)
    q = ref / 2.0 ** g
    assert torch.equal(q, q.round()), "the reference is no multiple of the granule"
    assert float(mag.max()) < 2.0 ** (24 + g), (float(mag.max()), g)


def expected(ref: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    r32 = ref.float()
    assert torch.equal(r32.double(), ref)
    return r32 if out_dtype == torch.float32 else r32.bfloat16()  # one rounding of an exact value


def to_device(kw: dict, device) -> dict:
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


# (kernel instance, (M, N) list, K list, epilogue cases (M, N, K))
FP8_SHORT = dict(MN=[(16, 16), (80, 64), (272, 264)], K=[16, 64, 80, 256])
FP8_PIPE = dict(MN=[(16, 16), (256, 256), (272, 264)], K=[272, 384, 400], epi=(272, 264, 400))
MX_SHORT = dict(MN=[(16, 16), (272, 264)], K=[32, 96, 416, 2048], epi=(272, 264, 416))
MX_PIPE = dict(MN=[(16, 16), (272, 264)], K=[2080, 2208], epi=(272, 264, 2208))
MX_FORCED_PIPE = dict(MN=[(256, 256)], K=[32, 128, 288, 416])
MX_FORCED_SHORT = dict(MN=[(272, 264)], K=[2080])
MX_SCALE_PAIRS = [(0, 254), (254, 0), (0, 200), (1, 246), (246, 8), (127, 127)]
FP8_DW = [(392, 272, 32)]                    # (ragged contraction, M, N): 392 -> 400
MX_DW = [(392, 288, 32), (2184, 288, 32)]    # 392 -> 416 (short), 2184 -> 2208 (pipelined)


def seed_of(*key) -> int:
    return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)


def fp8_case(M, N, K, fmt_a, epi, form="fwd", device="cpu"):
    """One per-tensor case: (a, b, gemm kwargs on ``device``, expected tensor).  ``form``: fwd (both
    row-major), dx (B transposed) or dw (both transposed, K the ragged contraction)."""
    sd = seed_of(M, N, K, fmt_a == "e5m2", EPIS.index(epi))
    a, A = fp8_operand(M, K, fmt_a, sd, SA_INV, form == "dw", device)
    b, B = fp8_operand(N, K, "e4m3", sd + 1, SB_INV, form in ("dx", "dw"), device)
    lin, mag = (A @ B.t()) * (SA_INV * SB_INV), (A.abs() @ B.abs().t()) * (SA_INV * SB_INV)
    ref, kw, extra, down = epilogue(lin, epi, sd)
    # the accumulator holds integers (granule 2^0, below 2^24); alpha = 4 and the epilogue act on it after
    check_exactness_precondition(A @ B.t(), A.abs() @ B.abs().t(), 0)
    check_exactness_precondition(ref, mag + extra, -down)
    kw.update(trans_a=form == "dw", trans_b=form in ("dx", "dw"))
    return a, b, to_device(kw, device), expected(ref, kw["out_dtype"])


def mx_case(M, N, K, fmt_a, epi, form="fwd", device="cpu", sbytes=(126, 127, 128), sa=None, sb=None):
    """As ``fp8_case`` for MXFP8.  ``sa`` / ``sb``: every scale byte of A / B instead of drawn ones."""
    sd = seed_of(M, N, K, fmt_a == "e5m2", EPIS.index(epi), 3)
    a, A = mx_operand(M, K, fmt_a, sd, form == "dw", device, sbytes=(sa,) if sa is not None else sbytes)
    b, B = mx_operand(N, K, "e4m3", sd + 1, form in ("dx", "dw"), device, sbytes=(sb,) if sb is not None else sbytes)
    if sa is not None:  # A and B alone can leave fp64's comfortable range only in their product's exponent
        e = sa + sb - 254
        A, B = A * 2.0 ** (127 - sa), B * 2.0 ** (127 - sb)
        lin, mag, g = (A @ B.t()) * 2.0 ** e, (A.abs() @ B.abs().t()) * 2.0 ** e, e
    else:
        lin, mag = A @ B.t(), A.abs() @ B.abs().t()
        g = 2 * (min(sbytes) - 127)
    ref, kw, extra, down = epilogue(lin, epi, sd)
    check_exactness_precondition(lin, mag, g)
    check_exactness_precondition(ref, mag + extra, g - down)
    kw.update(trans_a=form == "dw", trans_b=form in ("dx", "dw"))
    return a, b, to_device(kw, device), expected(ref, kw["out_dtype"])


# A bytes cycled down the rows, so every 16-row fragment holds 0 (an underflowed block) next to
# bytes >= 127; B bytes cycled down its rows.  Each byte runs along the whole row, so C[m, n] is an
# integer times 2^(sa[m] + sb[n] - 254): one granule per element, between 2^-126 and 2^116
MX_ROW_BYTES_A = (0, 127, 1, 130, 60, 127, 0, 128)
MX_ROW_BYTES_B = (128, 240, 135)


def mx_row_scale_case(fmt_a, device="cpu", M=64, N=64, K=128):
    """(a, b, gemm kwargs, expected): scale bytes that differ from row to row at the extremes."""
    sd = seed_of(M, N, K, fmt_a == "e5m2", 11)
    ops, ints, byts = [], [], []
    for rows, fmt, cyc, seed in ((M, fmt_a, MX_ROW_BYTES_A, sd), (N, "e4m3", MX_ROW_BYTES_B, sd + 1)):
        v = _ints(rows, K, seed)
        by = torch.tensor(cyc, dtype=torch.uint8).repeat(-(-rows // len(cyc)))[:rows]
        s = torch.full((rows, 4 * (-(-K // 128))), 127, dtype=torch.uint8)
        s[:, :K // 32] = by.unsqueeze(1)
        ops.append(MxTensor(v.float().to(FMT[fmt][0]).to(device), s.to(device), None, None, fmt))
        ints.append(v.double())
        byts.append(by.double())
    g = byts[0].unsqueeze(1) + byts[1].unsqueeze(0) - 254.0
    whole, mag = ints[0] @ ints[1].t(), ints[0].abs() @ ints[1].abs().t()
    # integers below 2^24 on a granule that is a normal number, and the largest partial sum finite in fp32
    assert float(mag.max()) < 2.0 ** 24 and float(g.min()) >= -126 and float((mag * torch.exp2(g)).max()) < 2.0 ** 128
    ref = whole * torch.exp2(g)
    return ops[0], ops[1], dict(out_dtype=torch.float32), expected(ref, torch.float32)


def all_fp8_cases():
    """(M, N, K, epi, form, mfma) of every per-tensor case of the exact tests."""
    out = []
    for MN in FP8_SHORT["MN"]:
        out += [(*MN, K, "none", "fwd", 0) for K in FP8_SHORT["K"]]
    for mfma in (0, 1):
        for MN in FP8_PIPE["MN"]:
            out += [(*MN, K, "none", "fwd", mfma) for K in FP8_PIPE["K"]]
        out += [(*FP8_PIPE["epi"], e, "fwd", mfma) for e in EPIS[1:]]
        out += [(272, 264, 400, "aux", "dx", mfma), (272, 32, 392, "acc", "dw", mfma)]
    out += [(272, 264, 144, "aux", "dx", 0)]
    return out


def all_mx_cases():
    """(M, N, K, epi, form, instance) of every MXFP8 case with drawn scale bytes."""
    out = []
    for spec in (MX_SHORT, MX_PIPE):
        for MN in spec["MN"]:
            out += [(*MN, K, "none", "fwd", 0) for K in spec["K"]]
        out += [(*spec["epi"], e, "fwd", 0) for e in EPIS[1:]]
    out += [(*MN, K, "none", "fwd", 1) for MN in MX_FORCED_PIPE["MN"] for K in MX_FORCED_PIPE["K"]]
    out += [(*MN, K, "none", "fwd", 2) for MN in MX_FORCED_SHORT["MN"] for K in MX_FORCED_SHORT["K"]]
    out += [(272, 264, 416, "aux", "dx", 0), (272, 264, 2208, "aux", "dx", 0)]
    out += [(M, N, B, "acc", "dw", 0) for B, M, N in MX_DW]
    return out


def case_id(c) -> str:
    return "-".join(str(v) for v in c)


# ------------------------------------------------------------------------------ D: the MLP function
def mlp_model(widths, batch, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = []
    for i, o in zip(widths[:-1], widths[1:]):
        params += [torch.randn(o, i, generator=g) / i ** 0.5, 0.1 * torch.randn(o, generator=g)]
    return params, torch.randn(batch, widths[0], generator=g), torch.randn(batch, widths[-1], generator=g)


def mlp_autograd(params, x, gy, slope, dev, dtype, cd):
    """[output, gradient of every parameter] as fp64 CPU tensors: plain autograd (``cd`` None) or
    ``ops.gemm.mlp`` with compute dtype ``cd``."""
    from distributed_training_pytorch_amd.ops.gemm import mlp

    ps = [p.clone().to(dev, dtype).requires_grad_() for p in params]
    h = x.to(dev, dtype)
    if cd is None:
        for l in range(0, len(ps), 2):
            h = torch.nn.functional.linear(h, ps[l], ps[l + 1])
            if l + 2 < len(ps):
                h = torch.nn.functional.leaky_relu(h, slope)
    else:
        h = mlp(h, ps[0::2], ps[1::2], slope, cd)
    h.backward(gy.to(dev, h.dtype))
    return [h.detach().double().cpu()] + [p.grad.double().cpu() for p in ps]


PREFILL = 0.25


def mlp_fused(params, x, gy, slope, dev, cd):
    """The same through ``mark_fused_grad`` targets: every parameter a view of one flat fp32 buffer,
    its ``.grad`` a view of a flat gradient buffer filled with PREFILL.  Returns ([output, every
    gradient view minus PREFILL], hook calls per parameter)."""
    from distributed_training_pytorch_amd.ops.gemm import add_grad_ready_hook, mark_fused_grad, mlp

    n = 1 + sum(p.numel() for p in params)  # one element of lead: every view is 4-byte aligned only
    flat = torch.zeros(n, device=dev)
    gflat = torch.full((n,), PREFILL, device=dev)
    ps, calls, off = [], [], 1
    for i, p in enumerate(params):
        v = flat[off:off + p.numel()].view(p.shape)
        v.copy_(p)
        v = v.detach().requires_grad_()
        v.grad = gflat[off:off + p.numel()].view(p.shape)
        mark_fused_grad(v)
        calls.append(0)
        add_grad_ready_hook(v, lambda q, i=i: calls.__setitem__(i, calls[i] + 1))
        ps.append(v)
        off += p.numel()
    h = mlp(x.to(dev), ps[0::2], ps[1::2], slope, cd)
    h.backward(gy.to(dev, h.dtype))
    for p in ps:
        assert p.grad.data_ptr() >= gflat.data_ptr() and p.grad.data_ptr() < gflat.data_ptr() + 4 * n
    return [h.detach().double().cpu()] + [(p.grad.double() - PREFILL).cpu() for p in ps], calls


def error_rows(r64, emu, got):
    names = ["out"] + [f"{'dW' if i % 2 == 0 else 'db'}{i // 2}" for i in range(len(r64) - 1)]
    return [(n, float((e - r).norm() / r.norm()), float((c - r).norm() / r.norm())) for n, r, e, c in zip(names, r64, emu, got)]

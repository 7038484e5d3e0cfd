"""MXFP8 operands for the wide-MLP GEMM path: the block-scaled quantiser
(``csrc/mxfp8_quant.hip``) and the block-scaled FP8 GEMM (``csrc/gemm_mxfp8.hip``).

OCP MX: every run of 32 elements along the contraction dimension carries one power-of-two
scale, an E8M0 byte ``s`` meaning ``2^(s - 127)``.  For a block with ``a = max|x|``:

* ``s = clamp(floor(log2 a) - emax + 127, 0, 254)`` with emax = 8 (e4m3) or 15 (e5m2); an
  all-zero block gets 127; byte 255 (NaN) is never written;
* ``q = cvt_rne(clamp(x * 2^(127 - s), -fmax, fmax))``, fmax = 448 or 57344.  The clamp is part
  of the format: with the floor rule a block holds values up to just under ``2 * 2^emax``, past
  fmax, which the bare cast would turn into NaN (e4m3) or infinity (e5m2).

The multiply by a power of two is exact, so the HIP kernel and this torch definition agree bit
for bit.  Inputs are finite by contract (a NaN or infinity in ``x`` gives an unspecified block).

A block's scale depends on that block alone: quantising is one launch with no reduction over the
tensor, no workspace and no host read.  The transposed copy (the operand of the dx and dW GEMMs,
which contract over the other index) is quantised for its own contraction: its blocks run along
M, so it has its own maxima, scales and rounding and is *not* the transpose of ``data``.

On CPU tensors both ops run the torch definition; on a GPU the HIP kernels are required.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .. import _native as nat
from .fp8 import check_split_k, split_workspace
from .gemm import _DT, _ld, _ref

_FMT = {"e4m3": (torch.float8_e4m3fn, 448.0, 8, nat.FP8_E4M3), "e5m2": (torch.float8_e5m2, 57344.0, 15, nat.FP8_E5M2)}
BLOCK = 32
_SHORT_K = 2048  # gemm_mxfp8.hip's kShortK: by default sums up to here run on the exact-fp32 short-K instance


class MxTensor(NamedTuple):
    data: torch.Tensor | None     # [M, K] fp8
    scale: torch.Tensor | None    # [M, 4 ceil(K / 128)] uint8: byte kb scales data[m, 32 kb .. +32); 127 past K / 32
    data_t: torch.Tensor | None   # [K, Mp] fp8, Mp = M rounded up to 32 (zeros past M), blocks along M
    scale_t: torch.Tensor | None  # [K, 4 ceil(Mp / 128)] uint8
    fmt: str


def _scale_cols(k: int) -> int:
    return 4 * (-(-k // 128))


def _quantize_def(x: torch.Tensor, fmt: str):
    """The definition on an fp32 [M, K] (K % 32 == 0): (fp8 [M, K], uint8 [M, 4 ceil(K / 128)])."""
    dtype, fmax, emax, _ = _FMT[fmt]
    M, K = x.shape
    xb = x.reshape(M, K // BLOCK, BLOCK)
    a = xb.abs().amax(dim=2)
    e = torch.frexp(a).exponent.to(torch.int32) - 1 - emax
    s = torch.where(a == 0, torch.full_like(e, 127), (e + 127).clamp(0, 254))
    mul = ((254 - s) << 23).view(torch.float32)  # 2^(127 - s), built from its bits: exact
    q = (xb * mul.unsqueeze(2)).clamp(-fmax, fmax).to(dtype).reshape(M, K)
    scale = torch.full((M, _scale_cols(K)), 127, dtype=torch.uint8, device=x.device)
    scale[:, :K // BLOCK] = s.to(torch.uint8)
    return q, scale


def quantize_mxfp8(x: torch.Tensor, fmt: str = "e4m3", transpose: bool = False) -> MxTensor:
    """Block-scaled cast of a finite fp32 / bf16 [M, K], K a multiple of 32 (module docstring);
    with ``transpose`` also the [K, Mp] copy quantised along M."""
    if fmt not in _FMT:
        raise ValueError(f"quantize_mxfp8: fmt {fmt!r} not in {sorted(_FMT)}")
    if x.dim() != 2 or x.dtype not in _DT or x.shape[1] % BLOCK or 0 in x.shape:
        raise ValueError(f"quantize_mxfp8: x must be a non-empty fp32 / bf16 [M, K] with K a multiple of 32, got "
                         f"{x.dtype} {tuple(x.shape)}")
    dtype, _, _, code = _FMT[fmt]
    M, K = x.shape
    Mp = -(-M // BLOCK) * BLOCK
    x = x.detach()
    if x.device.type != "cuda" or not nat.native_enabled():
        xf = x.float()
        q, s = _quantize_def(xf, fmt)
        qt = st = None
        if transpose:
            xt = torch.zeros(K, Mp, dtype=torch.float32, device=x.device)
            xt[:, :M] = xf.t()
            qt, st = _quantize_def(xt, fmt)
        return MxTensor(q, s, qt, st, fmt)
    lib = nat.require(x.device)
    if x.stride(1) != 1:
        x = x.contiguous()  # (rows that are not 16-byte aligned are fine: the kernel then loads by element)
    q = torch.empty(M, K, dtype=dtype, device=x.device)
    s = torch.empty(M, _scale_cols(K), dtype=torch.uint8, device=x.device)
    qt = torch.empty(K, Mp, dtype=dtype, device=x.device) if transpose else None
    st = torch.empty(K, _scale_cols(Mp), dtype=torch.uint8, device=x.device) if transpose else None
    nat.check(lib.dtp_mxfp8_quantize(nat.ptr(x), _ld(x, "x"), M, K, _DT[x.dtype], code, nat.ptr(q), K, nat.ptr(s),
                                     s.shape[1], nat.ptr(qt), Mp, nat.ptr(st), st.shape[1] if transpose else 0,
                                     nat.stream_ptr()), "dtp_mxfp8_quantize")
    return MxTensor(q, s, qt, st, fmt)


def dequantize_mxfp8(t: MxTensor, transposed: bool = False, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """``data * 2^(scale - 127)`` of one copy, float64 (exact) or float32."""
    d, s = _operand(t, transposed, "dequantize_mxfp8", "t")
    e = s[:, :d.shape[1] // BLOCK].to(torch.float64) - 127.0
    return (d.to(torch.float64) * torch.exp2(e).repeat_interleave(BLOCK, dim=1)).to(dtype)


def _operand(t: MxTensor, trans: bool, who: str, name: str):
    d, s = (t.data_t, t.scale_t) if trans else (t.data, t.scale)
    if d is None or s is None:
        raise ValueError(f"{who}: {name} was quantised without its {'transposed' if trans else 'row-major'} copy")
    return d, s


def gemm_mxfp8(a: MxTensor, b: MxTensor, *, trans_a: bool = False, trans_b: bool = False,
               bias: torch.Tensor | None = None, aux: torch.Tensor | None = None, act: bool = False,
               slope: float = 0.01, out: torch.Tensor | None = None, accumulate: bool = False,
               out_dtype: torch.dtype | None = None, instance: int = 0, split_k: int | None = None) -> torch.Tensor:
    """C[M,N] (+)= epilogue(sum_k A(m,k) 2^(sa(m,k/32)-127) B(n,k) 2^(sb(n,k/32)-127)), fp32 accumulation.

    A is ``a.data`` [M,K] (``a.data_t`` with ``trans_a``), B is ``b.data`` [N,K] (``b.data_t`` with
    ``trans_b``), each with its scale array: e4m3 x e4m3 or e5m2 x e4m3.  Epilogue order as ``gemm``:
    + bias[n], * LeakyReLU'(aux[m,n]) (aux bf16), LeakyReLU, (+ old C), cast to bf16 or fp32.
    ``instance``: 0 = by K, 1 = the pipelined block-scaled MFMA kernel, 2 = the short-K one (probes).
    ``split_k``: as ``gemm_fp8`` (``None`` planned, 1 unsplit, S > 1 forced; the pipelined instance only)."""
    (A, SA), (B, SB) = _operand(a, trans_a, "gemm_mxfp8", "a"), _operand(b, trans_b, "gemm_mxfp8", "b")
    (M, K), (N, Kb) = A.shape, B.shape
    if K != Kb:
        raise ValueError(f"gemm_mxfp8: inner dimensions differ ({K} vs {Kb})")
    if b.fmt != "e4m3" or a.fmt not in _FMT:
        raise ValueError("gemm_mxfp8: operand formats are e4m3 x e4m3 or e5m2 x e4m3")
    if K % BLOCK:
        raise ValueError(f"gemm_mxfp8: K = {K} is not a multiple of 32")
    out_dtype = out_dtype or (out.dtype if out is not None else torch.bfloat16)
    if out_dtype not in _DT:
        raise ValueError(f"gemm_mxfp8: out dtype must be float32 or bfloat16, got {out_dtype}")
    if out is None:
        out = (torch.zeros if accumulate else torch.empty)(M, N, dtype=out_dtype, device=A.device)
    if out.shape != (M, N) or out.dtype != out_dtype:
        raise ValueError(f"gemm_mxfp8: out must be [{M},{N}] {out_dtype}")
    if aux is not None and (aux.shape != (M, N) or aux.dtype != torch.bfloat16):
        raise ValueError("gemm_mxfp8: aux must be a bf16 [M,N]")
    check_split_k("gemm_mxfp8", split_k, K, out_dtype, act, aux, instance == 1 or (instance != 2 and K > _SHORT_K),
                  f"instance = 1 or K > {_SHORT_K}")
    if A.device.type != "cuda" or not nat.native_enabled():
        r = _ref(dequantize_mxfp8(a, trans_a, torch.float32), dequantize_mxfp8(b, trans_b, torch.float32), False, False,
                 bias, aux, act, slope, 1.0)
        if accumulate:
            r = r + out.float()
        out.copy_(r.to(out_dtype))
        return out
    lib = nat.require(A.device)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        bias = bias.float().contiguous()
    args = nat.GemmMxArgs()
    args.A, args.B, args.C = nat.ptr(A), nat.ptr(B), nat.ptr(out)
    args.bias, args.aux = nat.ptr(bias), nat.ptr(aux)
    args.sa, args.sb = nat.ptr(SA), nat.ptr(SB)
    args.lda, args.ldb, args.ldc = _ld(A, "a"), _ld(B, "b"), _ld(out, "out")
    args.ldaux = _ld(aux, "aux") if aux is not None else 0
    args.ldsa, args.ldsb = _ld(SA, "a.scale"), _ld(SB, "b.scale")
    args.M, args.N, args.K = M, N, K
    args.fmt_a, args.fmt_b = _FMT[a.fmt][3], _FMT[b.fmt][3]
    args.out_dtype = _DT[out_dtype]
    args.act, args.accumulate, args.slope = int(act), int(accumulate), float(slope)
    args.instance = int(instance)
    work = split_workspace(args, lib.dtp_gemm_mxfp8_workspace, split_k, A.device)  # noqa: F841 (alive until queued)
    nat.check(lib.dtp_gemm_mxfp8(args, nat.stream_ptr()), "dtp_gemm_mxfp8")
    return out


# ------------------------------------------------------------------ MLPFunction with MXFP8 compute
def mx_layer(w: torch.Tensor) -> bool:
    """A Linear runs on the MXFP8 GEMM only if both its widths are multiples of 32 (whole MX
    blocks along either contraction); any other layer of the same model stays on the bf16 kernels."""
    return w.shape[0] % BLOCK == 0 and w.shape[1] % BLOCK == 0


def mlp_mxfp8_forward(ctx, x, slope, params):
    """``MLPFunction.forward`` for ``compute_dtype=torch.float8_e8m0fnu``: per MX layer the weight
    (from its fp32 master) and the input activation are quantised to e4m3 once, each with both
    copies; the GEMM writes the bf16 activation (the backward's aux)."""
    from .gemm import _compute_weight, gemm

    weights, biases = params[0::2], params[1::2]
    L, cd = len(weights), torch.bfloat16
    h = x.detach().to(cd).contiguous()
    hs, saved, kinds = [h], [], []
    for l in range(L):
        last = l == L - 1
        out_dtype = torch.float32 if last else cd
        if mx_layer(weights[l]):
            wq = quantize_mxfp8(weights[l], "e4m3", transpose=True)
            hq = quantize_mxfp8(h, "e4m3", transpose=True)
            h = gemm_mxfp8(hq, wq, bias=biases[l].detach(), act=not last, slope=slope, out_dtype=out_dtype)
            saved += [hq.data_t, hq.scale_t, wq.data_t, wq.scale_t]
            kinds.append(True)
        else:
            w = _compute_weight(weights[l], cd)
            h = gemm(h, w, bias=biases[l].detach(), act=not last, slope=slope, out_dtype=out_dtype)
            saved.append(w)
            kinds.append(False)
        if not last:
            hs.append(h)
    ctx.save_for_backward(*hs, *saved)
    ctx.params = [q if q.is_leaf else None for q in params]
    ctx.L, ctx.slope, ctx.x_dtype, ctx.kinds = L, slope, x.dtype, kinds
    ctx.x_needs = ctx.needs_input_grad[0]
    return h


def mlp_mxfp8_backward(ctx, gy):
    """dz is quantised to e4m3 once with both copies: dx = dz.data x W.data_t contracts over the
    layer's outputs, dW = dz.data_t x h.data_t over the (padded) batch.  Bias gradients read the
    bf16 dz."""
    from .gemm import _fused_grad_target, _grad_ready, colsum, gemm

    L, slope, cd = ctx.L, ctx.slope, torch.bfloat16
    saved = list(ctx.saved_tensors)
    hs, rest = saved[:L], saved[L:]
    per_layer = []
    for k in ctx.kinds:
        n = 4 if k else 1
        per_layer.append(rest[:n])
        rest = rest[n:]
    dz = gy.to(cd).contiguous()
    gW: list[torch.Tensor | None] = [None] * L
    gb: list[torch.Tensor | None] = [None] * L
    dx = None
    need = ctx.needs_input_grad[3:]
    for l in range(L - 1, -1, -1):
        pw, pb = ctx.params[2 * l], ctx.params[2 * l + 1]
        tw = _fused_grad_target(pw) if (pw is not None and need[2 * l]) else None
        tb = _fused_grad_target(pb) if (pb is not None and need[2 * l + 1]) else None
        if ctx.kinds[l]:
            h_t, h_st, w_t, w_st = per_layer[l]
            dq = quantize_mxfp8(dz, "e4m3", transpose=True)
            hT = MxTensor(None, None, h_t, h_st, "e4m3")
            wT = MxTensor(None, None, w_t, w_st, "e4m3")
            if tw is not None:  # dW += dz^T h in the GEMM epilogue
                gemm_mxfp8(dq, hT, trans_a=True, trans_b=True, out=tw, accumulate=True)
            else:
                gW[l] = gemm_mxfp8(dq, hT, trans_a=True, trans_b=True, out_dtype=torch.float32)
        elif tw is not None:
            gemm(dz, hs[l], trans_a=True, trans_b=True, out=tw, accumulate=True)
        else:
            gW[l] = gemm(dz, hs[l], trans_a=True, trans_b=True, out_dtype=torch.float32)
        if tb is not None:
            colsum(dz, out=tb, accumulate=True)
        else:
            gb[l] = colsum(dz)
        for q, t in ((pw, tw), (pb, tb)):
            if t is not None:
                _grad_ready(q)
        if l > 0 or ctx.x_needs:
            kw = dict(aux=hs[l], slope=slope, out_dtype=cd) if l > 0 else dict(out_dtype=torch.float32)
            if ctx.kinds[l]:
                r = gemm_mxfp8(dq, wT, trans_b=True, **kw)
            else:
                r = gemm(dz, per_layer[l][0], trans_b=True, **kw)
            if l > 0:
                dz = r
            else:
                dx = r.to(ctx.x_dtype)
    grads = []
    for l in range(L):
        grads += [gW[l], gb[l]]
    return (dx, None, None, *grads)

"""FP8 operands for the wide-MLP GEMM path: the per-tensor quantiser
(``csrc/fp8_quant.hip``) and the FP8 GEMM (``csrc/gemm_fp8.hip``).

The hybrid recipe: e4m3 for activations and weights, e5m2 for the gradients flowing
back, fp32 accumulation, one scale per tensor from the tensor's current amax
(``scale = min(fmax / amax, 2^126)``, formed and kept on the device: nothing here reads
the GPU back, so a step can be captured into a hipGraph).  gfx950's formats are the OCP
ones, ``torch.float8_e4m3fn`` and ``torch.float8_e5m2``.

The cap: for a tensor whose amax is below ``fmax / FLT_MAX`` (about 1.3e-36 for e4m3,
1.7e-34 for e5m2: an underflowing gradient) the quotient is infinite, ``1 / scale`` is 0
and every element, exact zeros included, would come out as ``0 * inf`` = NaN.  With the
scale capped at 2^126 it is still one correctly rounded division (the kernel and the torch
definition stay bitwise equal), ``1 / scale`` stays a normal number, zeros stay zeros and
such a tensor is quantised into the low end of the format instead of poisoning the step.

The GEMM only takes K-contiguous operands, so the quantiser also writes the transposed
copy when asked (one launch reads ``x`` once and writes both).

On CPU tensors both ops run the torch definition of the same math; on a GPU the HIP
kernels are required.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .. import _native as nat
from .gemm import _DT, _ld, _ref

_MFMA = 0  # the kernel's matrix instruction: 0 = 16x16x128 f8f6f4, 1 = 16x16x32 fp8 / bf8
_SHORT_K = 256  # gemm_fp8.hip's kShortK: sums up to here run on the exact-fp32 short-K instance
_SCALE_CAP = 2.0 ** 126  # the largest scale (module docstring); fp8_quant.hip holds the same constant
_FMT = {"e4m3": (torch.float8_e4m3fn, 448.0, nat.FP8_E4M3), "e5m2": (torch.float8_e5m2, 57344.0, nat.FP8_E5M2)}


class Fp8Tensor(NamedTuple):
    data: torch.Tensor            # [M, K] fp8
    data_t: torch.Tensor | None   # [K, M] fp8: a view of rows padded with zeros to a multiple of 16
    scale: torch.Tensor           # fp32 scalar on the tensor's device: data = cvt(x * scale)
    scale_inv: torch.Tensor       # 1 / scale
    fmt: str


_PART_CAP = 16384  # amax partials per tensor of a delayed-scaling state (one per 64 x 64 tile, or 8 per GEMM tile)


class Fp8Slot(NamedTuple):
    """One tensor of an ``Fp8DelayedState``: what ``quantize_fp8(scale=...)`` and ``gemm_fp8(quant_out=...)`` take."""
    state: "Fp8DelayedState"
    index: int


class Fp8DelayedState:
    """Delayed scaling for ``n_tensors`` quantised tensors: per tensor a ring of the last ``history`` amaxes,
    the scale ``min(fmax / max(ring), 2^126)`` (1 while the ring holds only zeros) with its inverse, and the
    amax partials that the tensor's last producer wrote (word 0 their count).  ``update()`` is one launch
    over all of them (``csrc/fp8_quant.hip`` scale_update_kernel): each tensor whose producer ran since the
    last update has its amax pushed into its ring, and every scale is formed again.  Everything lives on the
    device; nothing is read back, so a step replays in a hipGraph once every tensor it touches is seeded.

    Seeding: the first time a tensor is quantised, its scale comes from its own amax (amax launch, update of
    that one record, given-scale quantiser): current scaling built from the same pieces.  That path cannot
    be captured into a graph (it depends on host state) and raises if tried."""

    def __init__(self, n_tensors: int, history: int = 16, device="cpu"):
        if n_tensors < 1 or not 1 <= int(history) <= 1024:
            raise ValueError(f"Fp8DelayedState: n_tensors >= 1 and 1 <= history <= 1024, got {n_tensors}, {history}")
        self.n, self.H, self.device = int(n_tensors), int(history), torch.device(device)
        dev = self.device
        self.history = torch.zeros(self.n, self.H, dtype=torch.float32, device=dev)
        self.scales = torch.ones(self.n, 2, dtype=torch.float32, device=dev)  # scale, 1 / scale
        self.partials = torch.zeros(self.n, 1 + _PART_CAP, dtype=torch.int32, device=dev)
        self.pos = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.seeded = [False] * self.n
        self.fmt: list[str | None] = [None] * self.n
        self._recs = None
        if dev.type == "cuda" and nat.native_enabled():
            self._write_records()

    def _write_records(self) -> None:
        import ctypes

        recs = (nat.Fp8ScaleRec * self.n)()
        for i, r in enumerate(recs):
            r.partials, r.history = nat.ptr(self.partials[i]), nat.ptr(self.history[i])
            r.scale, r.pos = nat.ptr(self.scales[i]), nat.ptr(self.pos[i:i + 1])
            r.cap, r.H, r.fmax = _PART_CAP, self.H, _FMT[self.fmt[i] or "e4m3"][1]
        host = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8)
        if self._recs is None:
            self._recs = torch.empty(ctypes.sizeof(recs), dtype=torch.uint8, device=self.device)
        self._recs.copy_(host)
        self._rec_bytes = ctypes.sizeof(nat.Fp8ScaleRec)

    def slot(self, index: int) -> Fp8Slot:
        if not 0 <= index < self.n:
            raise IndexError(f"Fp8DelayedState: slot {index} of {self.n}")
        return Fp8Slot(self, index)

    def bind(self, index: int, fmt: str) -> None:
        """The format of tensor ``index`` (its fmax goes into the record); fixed at first use."""
        if self.fmt[index] == fmt:
            return
        if self.fmt[index] is not None:
            raise ValueError(f"Fp8DelayedState: slot {index} holds {self.fmt[index]} tensors, not {fmt}")
        if torch.cuda.is_available() and self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Fp8DelayedState: a tensor's first use cannot be captured into a graph; run a step eagerly first")
        self.fmt[index] = fmt
        if self._recs is not None:
            self._write_records()

    def set_scale(self, index: int, scale, fmt: str = "e4m3") -> None:
        """Give tensor ``index`` a scale by hand (tests, probes); it counts as seeded."""
        self.bind(index, fmt)
        s = torch.as_tensor(scale, dtype=torch.float32, device=self.device)
        self.scales[index, 0] = s
        self.scales[index, 1] = torch.ones_like(s) / s
        self.seeded[index] = True

    def amax_of(self, index: int) -> torch.Tensor:
        """The maximum of the tensor's current partials (0 if its producer has not run since the last update)."""
        p = self.partials[index]
        live = torch.arange(_PART_CAP, device=p.device) < p[0]
        return torch.where(live, p[1:], torch.zeros_like(p[1:])).max().view(torch.float32)

    def update(self, index: int | None = None) -> None:
        """Push and rescale every tensor (``index``: that one only).  One launch; no host read."""
        if self._recs is not None:
            lib = nat.require(self.device)
            first, count = (0, self.n) if index is None else (index, 1)
            nat.check(lib.dtp_fp8_scale_update(nat.ptr(self._recs) + first * self._rec_bytes, count, nat.stream_ptr()),
                      "dtp_fp8_scale_update")
            return
        for i in (range(self.n) if index is None else (index,)):  # the torch definition of the same math
            if int(self.partials[i, 0]) > 0:
                p = int(self.pos[i])
                self.history[i, p] = self.amax_of(i)
                self.pos[i] = (p + 1) % self.H
                self.partials[i, 0] = 0
            amax = self.history[i].abs().max()
            fmax = torch.full_like(amax, _FMT[self.fmt[i] or "e4m3"][1])
            scale = torch.where(amax > 0, (fmax / amax).clamp(max=_SCALE_CAP), torch.ones_like(amax))
            self.scales[i, 0] = scale
            self.scales[i, 1] = torch.ones_like(scale) / scale


def fp8_amax(x: torch.Tensor, slot: Fp8Slot) -> None:
    """The amax partials of ``x`` into the slot's record (``dtp_fp8_amax``, the first launch of the
    current-scaling quantiser on its own): what seeds a delayed scale."""
    st, i = slot
    M, K = x.shape
    if x.device.type != "cuda" or not nat.native_enabled():
        st.partials[i, 1] = x.detach().float().abs().max().view(torch.int32)
        st.partials[i, 0] = 1
        return
    lib = nat.require(x.device)
    nat.check(lib.dtp_fp8_amax(nat.ptr(x), _ld(x, "x"), M, K, _DT[x.dtype], nat.ptr(st.partials[i]), _PART_CAP,
                               nat.stream_ptr()), "dtp_fp8_amax")


_SPAN_CHUNK = 4096  # elements per span item of a shadow's work table (16 per thread)


class Fp8WeightShadow:
    """The e4m3 operands of weight matrices inside a flat fp32 parameter buffer, written by the optimizer.

    Under delayed scaling a weight's scale is known before the weight is, so the flat optimizer's launch
    (``csrc/optim_fp8.hip``, ``flat_optimizer_step(shadow=...)``) also writes, per weight, ``q = cvt(clamp(
    p_new * scale, +-448))`` [out, in], its transpose ``qT`` [in, out], amax|p_new| into the slot's partials
    and the ``{scale, 1 / scale}`` it read into ``used``: the slot's scale is formed again by the next
    ``Fp8DelayedState.update()``, before the forward's GEMM reads the operand, so the operand carries the
    scale it was written with.  ``mlp_fp8_delayed_forward`` then takes ``operand(w)`` and launches no
    quantiser for ``w``.

    ``weights``: contiguous 2-D views of one row of ``flat`` each, both widths multiples of 16; ``slots``:
    their ``Fp8Slot``s.  Staleness is ``ops.gemm.ComputeShadow``'s rule: the operands are trusted only while
    the version counters of ``flat`` and of every weight are the ones recorded at ``mark_fresh()``; any torch
    in-place write makes ``operand`` return None until the optimizer has written again.  On a stale weight the
    forward quantises by a launch, with the scale in ``used`` once the optimizer has written one (the scale
    the operand it replaces was written with), else with the slot's."""

    def __init__(self, flat: torch.Tensor, weights, slots):
        weights, slots = list(weights), list(slots)
        if flat.dtype != torch.float32 or not flat.is_contiguous() or flat.dim() not in (1, 2):
            raise ValueError("Fp8WeightShadow: a contiguous fp32 flat buffer")
        if not weights or len(weights) != len(slots):
            raise ValueError("Fp8WeightShadow: one slot per weight, at least one weight")
        self.flat, self.weights, self.slots = flat, weights, slots
        rows = flat if flat.dim() == 2 else flat.view(1, -1)
        n, P = rows.shape
        self._offsets = []
        dev = flat.device
        for w, s in zip(weights, slots):
            if not isinstance(s, Fp8Slot) or s.state.device != dev:
                raise ValueError("Fp8WeightShadow: every weight needs an Fp8Slot of a state on the buffer's device")
            off = (w.data_ptr() - flat.data_ptr()) // 4
            if (w.dim() != 2 or w.dtype != torch.float32 or not w.is_contiguous() or w.device != dev or off < 0
                    or off + w.numel() > n * P or off // P != (off + w.numel() - 1) // P):
                raise ValueError("Fp8WeightShadow: every weight must be a contiguous 2-D view of one flat row")
            if not fp8_layer(w) or 0 in w.shape:
                raise ValueError(f"Fp8WeightShadow: both widths must be multiples of 16, got {tuple(w.shape)}")
            if -(-w.shape[0] // 64) * -(-w.shape[1] // 64) > _PART_CAP:
                raise ValueError(f"Fp8WeightShadow: {tuple(w.shape)} has more 64 x 64 tiles than the {_PART_CAP} partials")
            s.state.bind(s.index, "e4m3")
            self._offsets.append(off)
        self.q = [torch.zeros(w.shape, dtype=torch.float8_e4m3fn, device=dev) for w in weights]
        self.qT = [torch.zeros(w.shape[::-1], dtype=torch.float8_e4m3fn, device=dev) for w in weights]
        self.used = [torch.ones(2, dtype=torch.float32, device=dev) for _ in weights]
        for i, w in enumerate(weights):
            w._dtp_fp8_shadow = (self, i)
        self._token, self.written, self.served = None, False, 0
        self._recs = self._work = None
        if dev.type == "cuda" and nat.native_enabled():
            self._build_table(n, P)

    def _build_table(self, n: int, P: int) -> None:
        """The records (host copy for the entry's checks, device copy for the kernel) and the work items:
        per row, the tiles of its weights and the columns between them in chunks."""
        import ctypes

        recs = (nat.Fp8ShadowRec * len(self.weights))()
        for i, (w, (st, k)) in enumerate(zip(self.weights, self.slots)):
            r = recs[i]
            r.scale, r.partials, r.used = nat.ptr(st.scales[k]), nat.ptr(st.partials[k]), nat.ptr(self.used[i])
            r.q, r.qT, r.offset = nat.ptr(self.q[i]), nat.ptr(self.qT[i]), self._offsets[i]
            r.out, r.in_, r.cap = w.shape[0], w.shape[1], _PART_CAP
        items = []
        for model in range(n):
            col = 0
            mine = sorted((off - model * P, i) for i, off in enumerate(self._offsets) if off // P == model)
            for c, i in [*mine, (P, None)]:
                if c < col:
                    raise ValueError("Fp8WeightShadow: the weights overlap")
                items += [(-1, s, min(_SPAN_CHUNK, c - s), model) for s in range(col, c, _SPAN_CHUNK)]
                if i is not None:
                    out, k = self.weights[i].shape
                    items += [(i, t, 0, model) for t in range(-(-out // 64) * -(-k // 64))]
                    col = c + out * k
        table = (nat.Fp8WorkItem * len(items))()
        seen = set()
        for it, (rec, a, b, model) in zip(table, items):
            it.rec, it.a, it.b, it.model, it.first = rec, a, b, model, int(model not in seen)
            seen.add(model)
        dev = self.flat.device
        self._host_recs, self._n_items = recs, len(items)
        self._recs = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(dev)
        self._items = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        self._work = nat.Fp8ShadowWork(nat.ptr(self._recs), nat.ptr(self._items), len(items), 0)
        assert ctypes.sizeof(nat.Fp8WorkItem) == 32 and ctypes.sizeof(nat.Fp8ShadowRec) == 64

    def _current(self):
        return (self.flat._version, *(w._version for w in self.weights))

    def seeded(self) -> bool:
        """Does every weight's slot hold a scale?  (The first step seeds them in the forward.)"""
        return all(st.seeded[k] for st, k in self.slots)

    def step_native(self, lib, args) -> None:
        """``dtp_flat_optimizer_fp8`` with this shadow's records and work table."""
        import ctypes

        nat.check(lib.dtp_flat_optimizer_fp8(ctypes.byref(args), self._host_recs, len(self.weights), ctypes.byref(self._work),
                                             nat.stream_ptr()), "dtp_flat_optimizer_fp8")
        self.written = True

    def write_ref(self) -> None:
        """What the kernel writes besides the update, by the torch definition (CPU tensors)."""
        for i, (w, (st, k)) in enumerate(zip(self.weights, self.slots)):
            x = w.detach().float()
            q = (x * st.scales[k, 0]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
            self.q[i].copy_(q)
            self.qT[i].copy_(q.t())
            st.partials[k, 1] = x.abs().max().view(torch.int32)
            st.partials[k, 0] = 1
            self.used[i].copy_(st.scales[k])
        self.written = True

    def operand(self, w: torch.Tensor) -> Fp8Tensor | None:
        """The optimizer-written operand of ``w`` if it is fresh, else None."""
        sh = getattr(w, "_dtp_fp8_shadow", None)
        if sh is None or sh[0] is not self or self._token != self._current():
            return None
        i = sh[1]
        self.served += 1
        return Fp8Tensor(self.q[i], self.qT[i], self.used[i][0], self.used[i][1], "e4m3")

    def used_scales(self, w: torch.Tensor) -> torch.Tensor | None:
        """``{scale, 1 / scale}`` of the last operand the optimizer wrote for ``w`` (None before the first)."""
        return self.used[w._dtp_fp8_shadow[1]] if self.written else None

    def mark_fresh(self) -> None:
        self._token = self._current()

    def detach_(self) -> None:
        for w in self.weights:
            if getattr(w, "_dtp_fp8_shadow", (None,))[0] is self:
                del w._dtp_fp8_shadow


def _quantize_given(x: torch.Tensor, fmt: str, transpose: bool, slot: Fp8Slot, scales: torch.Tensor | None = None) -> Fp8Tensor:
    """``cvt(clamp(x * scale, -fmax, fmax))`` with the slot's scale (``scales``: this ``{scale, 1 / scale}``
    pair instead); the slot's partials receive amax|x|."""
    st, i = slot
    dtype, fmax, code = _FMT[fmt]
    st.bind(i, fmt)
    x = x.detach()
    if x.stride(1) != 1:
        x = x.contiguous()
    if not st.seeded[i]:  # current scaling from the same pieces: amax, the one record's update, then below
        if x.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("quantize_fp8: an unseeded Fp8DelayedState cannot be captured into a graph; run a step "
                               "eagerly first")
        fp8_amax(x, slot)
        st.update(i)
        st.seeded[i] = True
    M, K = x.shape
    Mp = -(-M // 16) * 16
    scale, scale_inv = (st.scales[i, 0], st.scales[i, 1]) if scales is None else (scales[0], scales[1])
    if x.device.type != "cuda" or not nat.native_enabled():
        q = (x.float() * scale).clamp(-fmax, fmax).to(dtype)
        qt = None
        if transpose:
            qt = torch.zeros(K, Mp, dtype=dtype)
            qt[:, :M] = q.t()
            qt = qt[:, :M]
        st.partials[i, 1] = x.float().abs().max().view(torch.int32)
        st.partials[i, 0] = 1
        return Fp8Tensor(q, qt, scale, scale_inv, fmt)
    lib = nat.require(x.device)
    q = torch.empty(M, K, dtype=dtype, device=x.device)
    qt = torch.empty(K, Mp, dtype=dtype, device=x.device) if transpose else None
    nat.check(lib.dtp_fp8_quantize_scaled(nat.ptr(x), _ld(x, "x"), M, K, _DT[x.dtype], code, nat.ptr(q), K, nat.ptr(qt), Mp,
                                          nat.ptr(scale), nat.ptr(st.partials[i]), _PART_CAP, nat.stream_ptr()),
              "dtp_fp8_quantize_scaled")
    return Fp8Tensor(q, None if qt is None else qt[:, :M], scale, scale_inv, fmt)


def quantize_fp8(x: torch.Tensor, fmt: str = "e4m3", transpose: bool = False, scale: Fp8Slot | None = None) -> Fp8Tensor:
    """``cvt(x * scale)`` with ``scale = min(fmax(fmt) / amax|x|, 2^126)`` (1 for an all-zero ``x``), round to
    nearest even; ``x`` is [M, K] fp32 or bf16 with K a multiple of 16.

    ``scale``: a slot of an ``Fp8DelayedState``.  The scale is then the slot's (from earlier steps' amaxes),
    ``x * scale`` is clamped to +-fmax before the convert (a stale scale saturates), and the one launch that
    reads ``x`` also leaves amax|x| in the slot for the next ``update()``."""
    if fmt not in _FMT:
        raise ValueError(f"quantize_fp8: fmt {fmt!r} not in {sorted(_FMT)}")
    if x.dim() != 2 or x.dtype not in _DT or x.shape[1] % 16 or 0 in x.shape:
        raise ValueError(f"quantize_fp8: x must be a non-empty fp32 / bf16 [M, K] with K a multiple of 16, got "
                         f"{x.dtype} {tuple(x.shape)}")
    if scale is not None:
        return _quantize_given(x, fmt, transpose, scale)
    dtype, fmax, code = _FMT[fmt]
    M, K = x.shape
    Mp = -(-M // 16) * 16
    if x.device.type != "cuda" or not nat.native_enabled():
        amax = x.detach().abs().max().float()
        # tensor / tensor: one correctly rounded fp32 division, as the kernel's (a python scalar
        # over a tensor is reciprocal-then-multiply, two roundings)
        scale = torch.where(amax > 0, (torch.full_like(amax, fmax) / amax).clamp(max=_SCALE_CAP), torch.ones_like(amax))
        q = (x.detach().float() * scale).to(dtype)
        qt = None
        if transpose:
            qt = torch.zeros(K, Mp, dtype=dtype)
            qt[:, :M] = q.t()
            qt = qt[:, :M]
        return Fp8Tensor(q, qt, scale, torch.ones_like(scale) / scale, fmt)
    lib = nat.require(x.device)
    x = x.detach()
    if x.stride(1) != 1:
        x = x.contiguous()  # (rows that are not 16-byte aligned are fine: the kernel then loads by element)
    q = torch.empty(M, K, dtype=dtype, device=x.device)
    qt = torch.empty(K, Mp, dtype=dtype, device=x.device) if transpose else None
    ws = torch.empty(nat.FP8_WS_FLOATS, dtype=torch.float32, device=x.device)
    nat.check(lib.dtp_fp8_quantize(nat.ptr(x), _ld(x, "x"), M, K, _DT[x.dtype], code, nat.ptr(q), K, nat.ptr(qt), Mp,
                                   nat.ptr(ws), nat.stream_ptr()), "dtp_fp8_quantize")
    return Fp8Tensor(q, None if qt is None else qt[:, :M], ws[0], ws[1], fmt)


def _operand(t: Fp8Tensor, trans: bool, name: str) -> torch.Tensor:
    d = t.data_t if trans else t.data
    if d is None:
        raise ValueError(f"gemm_fp8: {name} was quantised without its transposed copy")
    return d


def check_split_k(who: str, split_k: int | None, K: int, out_dtype: torch.dtype, act: bool, aux, pipelined: bool,
                  why_not: str) -> None:
    """A forced ``split_k``: S >= 1, and S > 1 only where the split-K instances run (an fp32 output without
    ``act`` / ``aux`` on the pipelined f8f6f4 kernel, at most one slice per 128-byte K-tile)."""
    if split_k is None:
        return
    if not isinstance(split_k, int) or split_k < 1:
        raise ValueError(f"{who}: split_k must be None (planned) or an int >= 1, got {split_k!r}")
    if split_k == 1:
        return
    if out_dtype != torch.float32 or act or aux is not None:
        raise ValueError(f"{who}: split_k > 1 needs an fp32 output without act and aux")
    if not pipelined:
        raise ValueError(f"{who}: split_k > 1 runs on the pipelined 16x16x128 kernel only ({why_not})")
    if split_k > -(-K // 128):
        raise ValueError(f"{who}: split_k = {split_k} exceeds the {-(-K // 128)} 128-byte K-tiles of K = {K}")


def split_workspace(args, query, split_k: int | None, device) -> torch.Tensor | None:
    """Set ``args.splitk`` / ``work`` / ``work_bytes``: the library's plan (``query``: its workspace size, 0 = no
    plan) for ``None``, a forced slice count otherwise.  The workspace comes from torch's caching allocator
    (stream-ordered, capturable); the caller keeps the returned tensor until the launch is queued."""
    if split_k is None and (args.out_dtype != nat.DT_F32 or args.act or args.aux):
        args.splitk = 1  # no plan for these (forward / dx): spare them the query
        return None
    args.splitk = 0 if split_k is None else split_k
    nbytes = query(args) if split_k is None else (4 * split_k * args.M * args.N if split_k > 1 else 0)
    if not nbytes:
        return None
    work = torch.empty(nbytes, dtype=torch.uint8, device=device)
    args.work, args.work_bytes = nat.ptr(work), nbytes
    return work


def gemm_fp8(a: Fp8Tensor, b: Fp8Tensor, *, trans_a: bool = False, trans_b: bool = False,
             bias: torch.Tensor | None = None, aux: torch.Tensor | None = None, act: bool = False, slope: float = 0.01,
             out: torch.Tensor | None = None, accumulate: bool = False,
             out_dtype: torch.dtype | None = None, mfma: int = _MFMA, split_k: int | None = None,
             quant_out: tuple[str, Fp8Slot] | None = None):
    """C[M,N] (+)= epilogue(a.scale_inv * b.scale_inv * A(m,k) B(n,k)), fp32 accumulation.

    ``quant_out = (fmt, slot)``: also return C quantised with the slot's delayed scale, row-major and
    transposed, as ``(C, Fp8Tensor)``: ``q = cvt(clamp(C * scale, -fmax, fmax))`` of the bf16 C, bit for bit
    what ``quantize_fp8(C, fmt, True, scale=slot)`` gives; amax|C| goes to the slot.  On the pipelined
    kernel its epilogue writes all of it (no quantiser launch, C is not read back); short K, unaligned
    views and an unseeded slot run the GEMM and the quantiser one after the other.  Needs a bf16 C,
    no ``accumulate`` and N a multiple of 16.

    A is ``a.data`` [M,K] (``a.data_t`` with ``trans_a``), B is ``b.data`` [N,K] (``b.data_t`` with
    ``trans_b``): e4m3 x e4m3 or e5m2 x e4m3.  Epilogue order as ``gemm``: + bias[n],
    * LeakyReLU'(aux[m,n]) (aux bf16), LeakyReLU, (+ old C), cast to bf16 or fp32.
    ``split_k``: K-slices per output tile.  ``None``: the library plans (a few-tile fp32 problem with a
    long K, the weight gradient of a 1024-2048-wide layer, is split over the idle CUs); 1: unsplit;
    S > 1: forced (tests and probes).  The sum is the same; on CPU tensors it is only checked."""
    A, B = _operand(a, trans_a, "a"), _operand(b, trans_b, "b")
    (M, K), (N, Kb) = A.shape, B.shape
    if K != Kb:
        raise ValueError(f"gemm_fp8: inner dimensions differ ({K} vs {Kb})")
    if b.fmt != "e4m3":
        raise ValueError("gemm_fp8: operand formats are e4m3 x e4m3 or e5m2 x e4m3")
    out_dtype = out_dtype or (out.dtype if out is not None else torch.bfloat16)
    if out_dtype not in _DT:
        raise ValueError(f"gemm_fp8: out dtype must be float32 or bfloat16, got {out_dtype}")
    if out is None:
        out = (torch.zeros if accumulate else torch.empty)(M, N, dtype=out_dtype, device=A.device)
    if out.shape != (M, N) or out.dtype != out_dtype:
        raise ValueError(f"gemm_fp8: out must be [{M},{N}] {out_dtype}")
    if aux is not None and (aux.shape != (M, N) or aux.dtype != torch.bfloat16):
        raise ValueError("gemm_fp8: aux must be a bf16 [M,N]")
    Kp = -(-K // 16) * 16  # a transposed copy's rows are padded with zeros to 16 bytes: the kernel sums over the padded K
    check_split_k("gemm_fp8", split_k, Kp, out_dtype, act, aux, Kp > _SHORT_K and int(mfma) != 1,
                  f"not mfma = 1, not K <= {_SHORT_K}")
    if quant_out is not None:
        qfmt, slot = quant_out
        if qfmt not in _FMT or out_dtype != torch.bfloat16 or accumulate or N % 16 or split_k not in (None, 1):
            raise ValueError("gemm_fp8: quant_out needs fmt e4m3 / e5m2, a bf16 out without accumulate or split_k, "
                             f"and N a multiple of 16 (got {qfmt!r}, {out_dtype}, N = {N})")
        slot.state.bind(slot.index, qfmt)
        if A.device.type != "cuda" or not nat.native_enabled() or not slot.state.seeded[slot.index]:
            c = gemm_fp8(a, b, trans_a=trans_a, trans_b=trans_b, bias=bias, aux=aux, act=act, slope=slope, out=out,
                         out_dtype=out_dtype, mfma=mfma)
            return c, quantize_fp8(c, qfmt, True, scale=slot)
    if A.device.type != "cuda" or not nat.native_enabled():
        r = _ref(A.float(), B.float(), False, False, bias, aux, act, slope, a.scale_inv * b.scale_inv)
        if accumulate:
            r = r + out.float()
        out.copy_(r.to(out_dtype))
        return out
    lib = nat.require(A.device)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        bias = bias.float().contiguous()
    if Kp != K and not (trans_a and trans_b):
        raise ValueError(f"gemm_fp8: K = {K} is not a multiple of 16 (only two transposed copies carry the padding)")
    args = nat.GemmFp8Args()
    args.A, args.B, args.C = nat.ptr(A), nat.ptr(B), nat.ptr(out)
    args.bias, args.aux = nat.ptr(bias), nat.ptr(aux)
    args.sa_inv, args.sb_inv = nat.ptr(a.scale_inv), nat.ptr(b.scale_inv)
    args.lda, args.ldb, args.ldc = max(_ld(A, "a"), Kp), max(_ld(B, "b"), Kp), _ld(out, "out")
    args.ldaux = _ld(aux, "aux") if aux is not None else 0
    args.M, args.N, args.K = M, N, Kp
    args.fmt_a, args.fmt_b = _FMT[a.fmt][2], _FMT[b.fmt][2]
    args.out_dtype = _DT[out_dtype]
    args.act, args.accumulate, args.slope = int(act), int(accumulate), float(slope)
    args.mfma = int(mfma)
    work = split_workspace(args, lib.dtp_gemm_fp8_workspace, split_k, A.device)  # noqa: F841 (alive until queued)
    if quant_out is None:
        nat.check(lib.dtp_gemm_fp8(args, nat.stream_ptr()), "dtp_gemm_fp8")
        return out
    st, i = slot
    Mp = -(-M // 16) * 16
    q = torch.empty(M, N, dtype=_FMT[qfmt][0], device=A.device)
    qt = torch.empty(N, Mp, dtype=_FMT[qfmt][0], device=A.device)
    qo = nat.Fp8QuantOut()
    qo.q, qo.qT, qo.ldq, qo.ldqt = nat.ptr(q), nat.ptr(qt), N, Mp
    qo.scale, qo.part, qo.cap, qo.fmt = nat.ptr(st.scales[i, 0]), nat.ptr(st.partials[i]), _PART_CAP, _FMT[qfmt][2]
    nat.check(lib.dtp_gemm_fp8_quant(args, qo, nat.stream_ptr()), "dtp_gemm_fp8_quant")
    return out, Fp8Tensor(q, qt[:, :M], st.scales[i, 0], st.scales[i, 1], qfmt)


# ------------------------------------------------------------------ MLPFunction with fp8 compute
def fp8_layer(w: torch.Tensor) -> bool:
    """A Linear runs on the FP8 GEMM only if both its widths are multiples of 16 (16-byte
    operand rows); any other layer of the same model stays on the bf16 kernels."""
    return w.shape[0] % 16 == 0 and w.shape[1] % 16 == 0


def mlp_fp8_forward(ctx, x, slope, params):
    """``MLPFunction.forward`` for ``compute_dtype=torch.float8_e4m3fn``: per FP8 layer the weight
    (from its fp32 master) and the input activation are quantised to e4m3 once, each with its
    transposed copy for the backward; the GEMM writes the bf16 activation (the backward's aux)."""
    from .gemm import _compute_weight, gemm

    weights, biases = params[0::2], params[1::2]
    L, cd = len(weights), torch.bfloat16
    h = x.detach().to(cd).contiguous()
    hs, saved, kinds = [h], [], []
    for l in range(L):
        last = l == L - 1
        out_dtype = torch.float32 if last else cd
        if fp8_layer(weights[l]):
            wq = quantize_fp8(weights[l], "e4m3", transpose=True)
            hq = quantize_fp8(h, "e4m3", transpose=True)
            h = gemm_fp8(hq, wq, bias=biases[l].detach(), act=not last, slope=slope, out_dtype=out_dtype)
            saved += [hq.data_t, hq.scale_inv, wq.data_t, wq.scale_inv]
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


def mlp_fp8_backward(ctx, gy):
    """dz is quantised to e5m2 (row-major for dx = dz W, transposed for dW = dz^T h); both GEMMs
    run e5m2 x e4m3 on the copies the forward saved.  Bias gradients read the bf16 dz."""
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
            h_t, h_sinv, w_t, w_sinv = per_layer[l]
            dq = quantize_fp8(dz, "e5m2", transpose=True)
            hT = Fp8Tensor(None, h_t, None, h_sinv, "e4m3")
            wT = Fp8Tensor(None, w_t, None, w_sinv, "e4m3")
            if tw is not None:  # dW += dz^T h in the GEMM epilogue
                gemm_fp8(dq, hT, trans_a=True, trans_b=True, out=tw, accumulate=True)
            else:
                gW[l] = gemm_fp8(dq, hT, trans_a=True, trans_b=True, out_dtype=torch.float32)
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
                r = gemm_fp8(dq, wT, trans_b=True, **kw)
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


# ------------------------------------------------------------------ the same with delayed scaling
def mlp_fp8_delayed_forward(ctx, x, slope, params, state: Fp8DelayedState):
    """``mlp_fp8_forward`` under delayed scaling.  ``state`` holds three tensors per layer (3 l: the weight,
    3 l + 1: the layer's input, 3 l + 2: the gradient of its output).  One ``update()`` launch opens the
    step; weights go through the given-scale quantiser (one read each); layer l's GEMM emits layer l + 1's
    quantised input with both copies from its epilogue, so an activation is never read back.  Only the
    first FP8 layer's input is quantised by a launch of its own.  A weight with a fresh ``Fp8WeightShadow``
    is not quantised here at all: the optimizer wrote its operand."""
    from .gemm import _compute_weight, gemm

    weights, biases = params[0::2], params[1::2]
    L, cd = len(weights), torch.bfloat16
    if any(state.seeded):
        state.update()
    h = x.detach().to(cd).contiguous()
    hs, saved, kinds = [h], [], []
    hq = None  # the quantised h, when the previous GEMM emitted it
    for l in range(L):
        last = l == L - 1
        out_dtype = torch.float32 if last else cd
        if fp8_layer(weights[l]):
            # the optimizer-written operand while it is fresh (Fp8WeightShadow): no quantiser launch
            sh = getattr(weights[l], "_dtp_fp8_shadow", (None,))[0]
            wq = sh.operand(weights[l]) if sh is not None else None
            if wq is None and sh is not None and sh.used_scales(weights[l]) is not None and state.seeded[3 * l]:
                wq = _quantize_given(weights[l], "e4m3", True, state.slot(3 * l), sh.used_scales(weights[l]))
            elif wq is None:
                wq = quantize_fp8(weights[l], "e4m3", transpose=True, scale=state.slot(3 * l))
            if hq is None:
                hq = quantize_fp8(h, "e4m3", transpose=True, scale=state.slot(3 * l + 1))
            kw = dict(bias=biases[l].detach(), act=not last, slope=slope, out_dtype=out_dtype)
            saved += [hq.data_t, hq.scale_inv, wq.data_t, wq.scale_inv]
            if not last and fp8_layer(weights[l + 1]):
                h, hq = gemm_fp8(hq, wq, quant_out=("e4m3", state.slot(3 * l + 4)), **kw)
            else:
                h, hq = gemm_fp8(hq, wq, **kw), None
            kinds.append(True)
        else:
            w = _compute_weight(weights[l], cd)
            h, hq = gemm(h, w, bias=biases[l].detach(), act=not last, slope=slope, out_dtype=out_dtype), None
            saved.append(w)
            kinds.append(False)
        if not last:
            hs.append(h)
    ctx.save_for_backward(*hs, *saved)
    ctx.params = [q if q.is_leaf else None for q in params]
    ctx.L, ctx.slope, ctx.x_dtype, ctx.kinds = L, slope, x.dtype, kinds
    ctx.x_needs = ctx.needs_input_grad[0]
    ctx.fp8_state = state
    return h


def mlp_fp8_delayed_backward(ctx, gy):
    """``mlp_fp8_backward`` under delayed scaling: the dx GEMM of layer l emits layer l - 1's e5m2 dz with
    both copies; only the gradient entering the last FP8 layer is quantised by a launch of its own."""
    from .gemm import _fused_grad_target, _grad_ready, colsum, gemm

    L, slope, cd, state = ctx.L, ctx.slope, torch.bfloat16, ctx.fp8_state
    saved = list(ctx.saved_tensors)
    hs, rest = saved[:L], saved[L:]
    per_layer = []
    for k in ctx.kinds:
        n = 4 if k else 1
        per_layer.append(rest[:n])
        rest = rest[n:]
    dz = gy.to(cd).contiguous()
    dq = None  # the quantised dz, when the previous dx GEMM emitted it
    gW: list[torch.Tensor | None] = [None] * L
    gb: list[torch.Tensor | None] = [None] * L
    dx = None
    need = ctx.needs_input_grad[3:]
    for l in range(L - 1, -1, -1):
        pw, pb = ctx.params[2 * l], ctx.params[2 * l + 1]
        tw = _fused_grad_target(pw) if (pw is not None and need[2 * l]) else None
        tb = _fused_grad_target(pb) if (pb is not None and need[2 * l + 1]) else None
        if ctx.kinds[l]:
            h_t, h_sinv, w_t, w_sinv = per_layer[l]
            if dq is None:
                dq = quantize_fp8(dz, "e5m2", transpose=True, scale=state.slot(3 * l + 2))
            hT = Fp8Tensor(None, h_t, None, h_sinv, "e4m3")
            wT = Fp8Tensor(None, w_t, None, w_sinv, "e4m3")
            if tw is not None:
                gemm_fp8(dq, hT, trans_a=True, trans_b=True, out=tw, accumulate=True)
            else:
                gW[l] = gemm_fp8(dq, hT, trans_a=True, trans_b=True, out_dtype=torch.float32)
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
            nq = None
            if ctx.kinds[l] and l > 0 and ctx.kinds[l - 1]:
                r, nq = gemm_fp8(dq, wT, trans_b=True, quant_out=("e5m2", state.slot(3 * l - 1)), **kw)
            elif ctx.kinds[l]:
                r = gemm_fp8(dq, wT, trans_b=True, **kw)
            else:
                r = gemm(dz, per_layer[l][0], trans_b=True, **kw)
            dq = nq
            if l > 0:
                dz = r
            else:
                dx = r.to(ctx.x_dtype)
    grads = []
    for l in range(L):
        grads += [gW[l], gb[l]]
    return (dx, None, None, *grads)


class MLPFp8DelayedFunction(torch.autograd.Function):
    """``ops.gemm.MLPFunction`` with ``compute_dtype=torch.float8_e4m3fn`` and an ``Fp8DelayedState``."""

    @staticmethod
    def forward(ctx, x, slope, state, *params):
        return mlp_fp8_delayed_forward(ctx, x, slope, params, state)

    @staticmethod
    def backward(ctx, gy):
        return mlp_fp8_delayed_backward(ctx, gy)


def delayed_state_for(weights, history: int = 16) -> Fp8DelayedState:
    """The state of an MLP with these weights: three tensors per layer, on the weights' device."""
    return Fp8DelayedState(3 * len(weights), history, weights[0].device)

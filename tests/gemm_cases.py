"""Exact-input case table for the GEMM and colsum kernels (``test_gemm_edges_gpu.py``).

Every operand, ``bias``, ``aux`` and old-C value is a small integer (A, B, aux, bias in
[-3, 3], old C in [-64, 64]: all exact in bf16), ``alpha`` is 1 or 0.5 and the slope 0.25.
With K <= 2048 every product, every partial sum and every epilogue step is then exact in
fp32 in ANY summation order, so a correct kernel with fp32 accumulation returns the fp64
reference bit for bit -- whatever its MFMA shape, split-K order or use of atomics -- and a
bf16 output equals the reference rounded once to nearest even.  The tests compare with
``torch.equal``; ``test_case_table_is_exact_on_cpu`` checks the condition itself.

Operands and ``aux`` sit as views inside NaN-filled boxes (anything a kernel reads outside
the operand poisons the result), outputs inside a box of a finite sentinel that must come
back bit-identical around the view.

A *group* shares its operands (one shape, dtype, layout and kernel request); its *cases*
vary the epilogue, the output dtype and the placement of ``out`` / ``aux``.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import torch

from distributed_training_pytorch_amd.ops.gemm import _auto_splitk, colsum, gemm

SLOPE = 0.25
SENTINEL = 1000.0
F32, BF16 = torch.float32, torch.bfloat16
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
_DN = {F32: "f32", BF16: "bf16"}


def lname(ta: bool, tb: bool) -> str:
    return ("T" if ta else "N") + ("T" if tb else "N")


# ---------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------
PAD_ROWS = 2


def _box_geometry(width: int, placement: str) -> tuple[int, int]:
    """(column offset, leading dimension) in elements."""
    if placement == "aligned":  # 16-byte aligned offset, ld a multiple of 8 (bf16) and of 4 (f32)
        off = 8
        return off, -(-(off + width + 3) // 8) * 8
    if placement == "odd":  # 3 elements in, odd ld: no row is 16-byte aligned relative to the last
        off = 3
        return off, (off + width + 2) | 1
    raise ValueError(placement)


def boxed(t: torch.Tensor, placement: str, fill: float, device=None):
    """``t`` ([R, W] or [W]) as a view inside a larger buffer filled with ``fill``: pad rows
    above and below, a leading dimension larger than the width, a column offset.
    Returns (buffer, view); the buffer lives on ``device`` (default: ``t``'s)."""
    device = t.device if device is None else device
    if t.dim() == 1:
        off, ld = _box_geometry(t.shape[0], placement)
        buf = torch.full((ld,), fill, dtype=t.dtype)
        buf[off:off + t.shape[0]] = t
        buf = buf.to(device)
        return buf, buf[off:off + t.shape[0]]
    R, W = t.shape
    off, ld = _box_geometry(W, placement)
    buf = torch.full((R + 2 * PAD_ROWS, ld), fill, dtype=t.dtype)
    buf[PAD_ROWS:PAD_ROWS + R, off:off + W] = t
    buf = buf.to(device)
    return buf, buf[PAD_ROWS:PAD_ROWS + R, off:off + W]


def outside_unchanged(before: torch.Tensor, after: torch.Tensor, view_of_after: torch.Tensor) -> bool:
    """Everything of the box outside the view is bit-identical to the clone taken before."""
    a, b = after.clone(), before.clone()
    off = (view_of_after.data_ptr() - after.data_ptr()) // after.element_size()
    if after.dim() == 1:
        n = view_of_after.shape[0]
        a[off:off + n] = 0
        b[off:off + n] = 0
    else:
        ld = after.stride(0)
        r0, c0 = divmod(off, ld)
        R, W = view_of_after.shape
        a[r0:r0 + R, c0:c0 + W] = 0
        b[r0:r0 + R, c0:c0 + W] = 0
    return torch.equal(a, b)  # the sentinel is finite: value equality is bit equality here


# ---------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Epi:
    name: str
    alpha: float = 1.0
    bias: bool = False
    aux: bool = False
    act: bool = False
    accumulate: bool = False
    out_dtype: torch.dtype | None = None  # None: taken from the case


EPI = {e.name: e for e in [
    Epi("none"),
    Epi("bias", bias=True),
    Epi("alpha_bias_act", alpha=0.5, bias=True, act=True),
    Epi("aux", aux=True),
    Epi("acc_f32", accumulate=True, out_dtype=F32),
    Epi("acc_bf16", accumulate=True, out_dtype=BF16),
    Epi("all", alpha=0.5, bias=True, aux=True, act=True, accumulate=True),
    # split-K epilogues (f32 output, no activation) and the skinny-output kernel's
    Epi("alpha", alpha=0.5),
    Epi("acc", accumulate=True),
    Epi("acc_alpha", alpha=0.5, accumulate=True),
    Epi("acc_alpha_bias", alpha=0.5, bias=True, accumulate=True),
    # the 256x256 register kernel's two
    Epi("bias_act_bf16", bias=True, act=True),
    Epi("aux_acc_f32", aux=True, accumulate=True),
]}
EPI_SET = ["none", "bias", "alpha_bias_act", "aux", "acc_f32", "acc_bf16", "all"]


@dataclass(frozen=True)
class Case:
    epi: str
    out_dtype: torch.dtype
    out_place: str
    aux_place: str
    ops_place: str = "aligned"  # both operands
    b_place: str | None = None  # operand b alone, when it differs

    @property
    def id(self) -> str:
        s = f"{self.epi}-{_DN[self.out_dtype]}-ops:{self.ops_place}"
        if self.b_place:
            s += f"/b:{self.b_place}"
        s += f"-out:{self.out_place}"
        if EPI[self.epi].aux:
            s += f"-aux:{self.aux_place}"
        return s


@dataclass(frozen=True)
class Group:
    family: str
    kernel: str  # the kernel family dtp_gemm's rules send every case of the group to
    M: int
    N: int
    K: int
    dtype: torch.dtype
    ta: bool
    tb: bool
    fast: object = None
    splitk: int | None = None
    force_big: bool = False
    nonfinite: bool = False
    cases: tuple = field(default=(), compare=False)
    cpu_shape: tuple | None = None  # cut-down (M, N, K) for the CPU side of the table

    @property
    def id(self) -> str:
        s = f"{self.family}-{self.kernel}-{self.M}x{self.N}x{self.K}-{_DN[self.dtype]}-{lname(self.ta, self.tb)}"
        if self.fast is not None:
            s += f"-fast{self.fast}"
        if self.splitk is not None:
            s += f"-splitk{self.splitk}"
        if self.force_big:
            s += "-big"
        if self.nonfinite:
            s += "-nonfinite"
        return s


def _epi_cases(ops_places=("aligned", "odd"), epis=EPI_SET, out_dtypes=(F32, BF16), mixed_aux=True):
    """The standard epilogue set x output dtypes x placements of out / aux (aux follows out,
    plus out aligned with aux odd: the vector store next to an aux that cannot be a vector load)."""
    cases = []
    for op in ops_places:
        for name in epis:
            e = EPI[name]
            for od in ((e.out_dtype,) if e.out_dtype else out_dtypes):
                places = [("aligned", "aligned"), ("odd", "odd")]
                if e.aux and mixed_aux:
                    places.append(("aligned", "odd"))
                for po, pa in places:
                    cases.append(Case(name, od, po, pa, op))
    return tuple(cases)


def _rot(seq, i, n):
    """n items of seq starting at i, cyclically: spreads a product without running all of it."""
    return [seq[(i + j) % len(seq)] for j in range(n)]


def _family_a():
    gs = []
    shapes = [(1, 1, 17), (5, 129, 31), (127, 128, 33), (129, 127, 63), (128, 257, 65), (130, 40, 129)]
    for M, N, K in shapes:
        for dt in (F32, BF16):
            for ta, tb in LAYOUTS:
                gs.append(Group("a", "tile128", M, N, K, dt, ta, tb, fast=False, cases=_epi_cases()))
    # tile decode at K = 17: nine M-tiles (second 8-row group has one member, grid not a
    # multiple of 8) and a 72-tile grid (the XCD remap); the epilogue set once per group,
    # output dtype and placements alternating
    i = 0
    for M, N, K in [(1030, 130, 17), (1030, 1000, 17)]:
        for dt in (F32, BF16):
            for ta, tb in LAYOUTS:
                cases = []
                for j, name in enumerate(EPI_SET):
                    e = EPI[name]
                    od = e.out_dtype or (F32, BF16)[(i + j) % 2]
                    pl = ("aligned", "odd")[(i + j // 2) % 2]
                    cases.append(Case(name, od, pl, pl, ("aligned", "odd")[(i + j) % 2]))
                gs.append(Group("a", "tile128", M, N, K, dt, ta, tb, fast=False, cases=tuple(cases)))
                i += 1
    # atomic split-K: slice counts that divide, leave empty last slices, or exceed the K-tiles
    i = 0
    for dt in (F32, BF16):
        bk = 32 if dt == F32 else 64
        for K in (129, 300, 577):
            for sk in (2, 3, 7, 64):
                ta, tb = LAYOUTS[i % 4]
                kern = "tile128_atomic" if min(sk, -(-K // bk)) > 1 else "tile128"
                cases = tuple(Case(e, F32, po, po, op) for e in ("none", "acc_alpha_bias")
                              for po, op in (("aligned", "aligned"), ("odd", "odd")))
                gs.append(Group("a", kern, 129, 130, K, dt, ta, tb, splitk=sk, cases=cases))
                i += 1
    return gs


def _family_b():
    gs = []
    pairs = [(1, 1), (127, 7), (129, 8), (300, 255), (127, 257), (300, 264), (1, 264)]
    i = 0
    for K in (1, 2, 3, 8, 16, 17):
        for dt in (F32, BF16):
            for ta, tb in LAYOUTS:
                # four of the seven (M, N) pairs per group, rotating: every pair meets every K
                # and dtype; the loads are per element whatever the placement: alternate it
                for j, (M, N) in enumerate(_rot(pairs, i, 4)):
                    cases = _epi_cases(ops_places=(("aligned", "odd")[(i + j) % 2],))
                    gs.append(Group("b", "skinny_k" if K <= 16 else "tile128", M, N, K, dt, ta, tb, cases=cases))
                i += 1
    return gs


def _family_c():
    gs = []
    modes = ("none", "acc", "alpha", "acc_alpha")
    i = 0
    for wide_a in (True, False):
        for J in (1, 2, 3, 4):
            for W in (8, 248, 264):
                for K in (64, 65, 255, 257, 300):
                    M, N = (W, J) if wide_a else (J, W)
                    # the wide operand stays aligned (the kernel's precondition); the skinny one alternates
                    sk = ("aligned", "odd")[i % 2]
                    cases = tuple(Case(e, F32, po, po, "aligned" if wide_a else sk, sk if wide_a else "aligned")
                                  for e in modes for po in ("aligned", "odd"))
                    gs.append(Group("c", "skinny_out", M, N, K, BF16, True, True, cases=cases))
                    i += 1
    # neighbours that fall through to the general kernel
    nb = [(264, 2, 63, "aligned"), (2, 264, 63, "aligned"),   # K = 63
          (13, 2, 300, "aligned"), (3, 13, 300, "aligned"),    # W = 13
          (264, 5, 300, "aligned"), (5, 264, 300, "aligned"),  # min(M, N) = 5
          (264, 2, 300, "odd"), (3, 264, 300, "odd"),          # a misaligned wide operand
          (3, 4, 64, "aligned"), (4, 2, 300, "aligned")]       # M and N both <= 4
    for M, N, K, op in nb:
        cases = tuple(Case(e, F32, po, po, op) for e in modes for po in ("aligned", "odd"))
        gs.append(Group("c", "tile128", M, N, K, BF16, True, True, cases=cases))
    return gs


def _dma_kernel(fast, K):
    if fast == 4:
        return "dma2"
    if fast == 37 and (K // 64) % 2 == 0:
        return "ph8_persistent"
    return "ph8"


def _family_d():
    gs = []
    shapes = [(8, 8, 64), (40, 24, 64), (264, 40, 128), (40, 264, 192), (520, 264, 256)]
    for fast in (4, True, 34, 36, 37):
        for M, N, K in shapes:
            for ta, tb in LAYOUTS:
                gs.append(Group("d", _dma_kernel(fast, K), M, N, K, BF16, ta, tb, fast=fast,
                                cases=_epi_cases(ops_places=("aligned",))))
        # ragged against the 8-column epilogue chunk (N % 8 != 0 rules out a transposed b)
        gs.append(Group("d", _dma_kernel(fast, 64), 13, 301, 64, BF16, False, False, fast=fast,
                        cases=_epi_cases(ops_places=("aligned",))))
    # a broken precondition under fast=True comes back through the 128x128 kernel
    few = _epi_cases(ops_places=("aligned",), epis=("none", "alpha_bias_act", "all"), mixed_aux=False)
    gs.append(Group("d", "tile128", 40, 24, 96, BF16, False, False, fast=True, cases=few))
    gs.append(Group("d", "tile128", 12, 24, 64, BF16, True, False, fast=True, cases=few))
    gs.append(Group("d", "tile128", 40, 24, 64, BF16, False, True, fast=True,
                    cases=_epi_cases(ops_places=("odd",), epis=("none", "alpha_bias_act", "all"), mixed_aux=False)))
    return gs


def _family_e():
    gs = []
    cases = tuple(Case(e, F32, po, po) for e in ("none", "acc_alpha_bias") for po in ("aligned", "odd"))
    plan = [(96, 96, 1024, [(True, True)]), (8, 301, 1024, [(False, False), (True, False)]),
            (264, 40, 2048, LAYOUTS),
            (300, 1, 1024, [(False, False)])]  # the last Linear (one output) of a 1024-wide MLP
    for M, N, K, lays in plan:
        for ta, tb in lays:
            gs.append(Group("e", "ph8_splitk", M, N, K, BF16, ta, tb, cases=cases))
    # 17 K-tiles: no plan, atomic split-K on the 128x128 kernel
    gs.append(Group("e", "tile128_atomic", 96, 96, 1088, BF16, True, True, cases=cases))
    return gs


def _family_f():
    gs = []
    i = 0
    for M, N in [(8, 130824), (130824, 8)]:
        for ta, tb in LAYOUTS:
            pl = ("aligned", "odd")[i % 2]
            cases = (Case("bias_act_bf16", BF16, pl, pl), Case("aux_acc_f32", F32, pl, pl))
            cpu = (8, 1032, 256) if M == 8 else (1032, 8, 256)
            gs.append(Group("f", "big256", M, N, 256, BF16, ta, tb, force_big=True, cases=cases, cpu_shape=cpu))
            i += 1
    return gs


def _family_h():
    """One non-finite case per family a-e: a NaN in the last row of A (the row a clamped
    load duplicates) and an Inf in the first."""
    c2 = lambda *e: tuple(Case(x, od, "aligned", "aligned") for x in e for od in (F32, BF16))  # noqa: E731
    f32 = lambda *e: tuple(Case(x, F32, "aligned", "aligned") for x in e)  # noqa: E731
    return [
        Group("h", "tile128", 129, 127, 63, BF16, False, True, fast=False, nonfinite=True, cases=c2("none", "all")),
        Group("h", "tile128_atomic", 129, 130, 300, F32, True, True, splitk=3, nonfinite=True,
              cases=f32("none", "acc_alpha_bias")),
        Group("h", "skinny_k", 129, 257, 3, BF16, False, False, nonfinite=True, cases=c2("none", "all")),
        Group("h", "skinny_out", 264, 3, 257, BF16, True, True, nonfinite=True, cases=f32("none", "acc_alpha")),
        Group("h", "ph8", 264, 40, 128, BF16, False, True, fast=True, nonfinite=True, cases=c2("none", "all")),
        Group("h", "dma2", 40, 264, 192, BF16, True, False, fast=4, nonfinite=True, cases=c2("none", "all")),
        Group("h", "ph8_splitk", 8, 301, 1024, BF16, False, False, nonfinite=True,
              cases=f32("none", "acc_alpha_bias")),
    ]


GROUPS = _family_a() + _family_b() + _family_c() + _family_d() + _family_e() + _family_f() + _family_h()


def groups_of(family: str) -> list[Group]:
    return [g for g in GROUPS if g.family == family]


# ---------------------------------------------------------------------------------------
# the host's dispatch rules (csrc/gemm.hip: dtp_gemm), mirrored to name a case's kernel
# ---------------------------------------------------------------------------------------
def _ld(t):
    return max(t.stride(0), 1) if t.shape[0] > 1 else max(t.shape[1], 1)


def _vec(t, epc):
    return _ld(t) % epc == 0 and t.data_ptr() % 16 == 0


def ph8_plan(M, N, K):
    tiles = -(-M // 256) * -(-N // 256)
    if K % 64 or tiles >= 128:
        return 0
    nk, s = K // 64, 1
    while tiles * s * 2 <= 256 and nk % (s * 4) == 0 and nk // (s * 2) >= 8:
        s *= 2
    return s if s > 1 else 0


def route(g: Group, M, N, K, a, b, e: Epi, out_dtype) -> str:
    bf = g.dtype == BF16
    ta, tb = g.ta, g.tb
    if (bf and ta and tb and out_dtype == F32 and not (e.act or e.aux or e.bias) and (M <= 4 or N <= 4) and K >= 64):
        x, W = (a, M) if N <= 4 else (b, N)
        if W % 8 == 0 and _vec(x, 8):
            return "skinny_out"
    fast = 0 if g.fast is None else (1 if g.fast is True else -1 if g.fast is False else int(g.fast))
    va, vb = _vec(a, 8 if bf else 4), _vec(b, 8 if bf else 4)
    shape_ok = bf and K % 64 == 0 and va and vb and (not ta or M % 8 == 0) and (not tb or N % 8 == 0) and not g.force_big
    splitk = g.splitk
    if splitk is None:
        splitk = 1
        if out_dtype == F32 and not e.act and not e.aux:
            if shape_ok and fast >= 0 and ph8_plan(M, N, K) > 1:
                return "ph8_splitk"
            splitk = _auto_splitk(M, N, K, g.dtype)
    splitk = max(1, min(splitk, -(-K // (64 if bf else 32))))
    if K <= 16 and splitk == 1:
        return "skinny_k"
    big_tiles = -(-M // 256) * -(-N // 256)
    if shape_ok and splitk == 1 and fast >= 0 and (fast > 0 or big_tiles >= 128):
        if fast < 2 or fast - 2 in (32, 34):
            return "ph8"
        if fast - 2 == 35:
            return "ph8_persistent" if (K // 64) % 2 == 0 else "ph8"
        return "dma2"
    lean = va and vb and (M if ta else K) % 8 == 0 and (N if tb else K) % 8 == 0
    if bf and splitk == 1 and big_tiles >= 512 and K >= 256 and lean and (g.force_big or not (ta or tb)):
        return "big256"
    return "tile128_atomic" if splitk > 1 else "tile128"


# ---------------------------------------------------------------------------------------
# inputs, reference, run
# ---------------------------------------------------------------------------------------
def _gen(g: Group) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(g.id.encode()))


def _ints(gen, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen, dtype=torch.int16)


def _ab64(A: torch.Tensor, B: torch.Tensor, nonfinite: bool) -> torch.Tensor:
    """fp64 A B^T of the logical [M, K], [N, K] operands.  With non-finite values the sum is
    formed explicitly (no BLAS shortcut may decide where a NaN lands)."""
    A, B = A.double(), B.double()
    if not nonfinite:
        return A @ B.t()
    rows = [(A[m0:m0 + 16, None, :] * B[None, :, :]).sum(-1) for m0 in range(0, A.shape[0], 16)]
    return torch.cat(rows)


@dataclass
class Operands:
    M: int
    N: int
    K: int
    A: torch.Tensor  # logical [M, K], [N, K], CPU, the group's dtype
    B: torch.Tensor
    ab: torch.Tensor  # fp64
    bias: torch.Tensor
    aux: torch.Tensor
    old: torch.Tensor  # fp32 integers in [-64, 64]


def operands(g: Group, cpu_side: bool = False) -> Operands:
    M, N, K = g.cpu_shape if (cpu_side and g.cpu_shape) else (g.M, g.N, g.K)
    gen = _gen(g)
    A = _ints(gen, (M, K), 3).to(g.dtype)
    B = _ints(gen, (N, K), 3).to(g.dtype)
    if g.nonfinite:
        assert M >= 2 and K >= 2
        A[M - 1, K // 3] = float("nan")
        A[0, K - 1] = float("inf")
    return Operands(M, N, K, A, B, _ab64(A, B, g.nonfinite), _ints(gen, (N,), 3).float(),
                    _ints(gen, (M, N), 3).to(g.dtype), _ints(gen, (M, N), 64).float())


def reference(o: Operands, e: Epi) -> torch.Tensor:
    """fp64, in the documented epilogue order: alpha AB + bias, * LeakyReLU'(aux), LeakyReLU, + old C."""
    r = e.alpha * o.ab
    if e.bias:
        r = r + o.bias.double()
    if e.aux:
        r = r * torch.where(o.aux.double() > 0, 1.0, SLOPE)
    if e.act:
        r = torch.where(r > 0, r, r * SLOPE)
    if e.accumulate:
        r = r + o.old.double()
    return r


def exact_in(ref: torch.Tensor, dtype: torch.dtype) -> bool:
    """ref (fp64) survives the round trip through ``dtype`` (NaN and Inf in place)."""
    back = ref.to(dtype).double()
    return bool(((back == ref) | (back.isnan() & ref.isnan())).all())


def same(got: torch.Tensor, want: torch.Tensor, nonfinite: bool) -> bool:
    if not nonfinite:
        return torch.equal(got, want)
    try:
        torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True)
    except AssertionError:
        return False
    return True


class Runner:
    """Runs a group's cases on one device; the operands are boxed once per placement."""

    def __init__(self, g: Group, device, cpu_side: bool = False):
        self.g, self.dev = g, torch.device(device)
        self.o = operands(g, cpu_side)
        self._ops = {}

    def ops(self, pa: str, pb: str):
        if (pa, pb) not in self._ops:
            g, o = self.g, self.o
            a = boxed(o.A.t().contiguous() if g.ta else o.A, pa, float("nan"), self.dev)[1]
            b = boxed(o.B.t().contiguous() if g.tb else o.B, pb, float("nan"), self.dev)[1]
            self._ops = {(pa, pb): (a, b)}  # one placement at a time stays resident
        return self._ops[(pa, pb)]

    def run(self, c: Case):
        """(got, expected, outside-of-view unchanged, kernel the dispatch rules name, fp64 reference)."""
        g, o, e = self.g, self.o, EPI[c.epi]
        a, b = self.ops(c.ops_place, c.b_place or c.ops_place)
        ref = reference(o, e)
        want = ref.float().to(c.out_dtype)
        init = o.old if e.accumulate else torch.full((o.M, o.N), float("nan"))
        box, out = boxed(init.to(c.out_dtype), c.out_place, SENTINEL, self.dev)
        before = box.clone()
        aux = boxed(o.aux, c.aux_place, float("nan"), self.dev)[1] if e.aux else None
        bias = o.bias.to(self.dev) if e.bias else None
        kern = route(g, o.M, o.N, o.K, a, b, e, c.out_dtype)
        ret = gemm(a, b, trans_a=g.ta, trans_b=g.tb, out=out, bias=bias, aux=aux, act=e.act, slope=SLOPE,
                   accumulate=e.accumulate, alpha=e.alpha, splitk=g.splitk, force_big=g.force_big, fast=g.fast)
        assert ret is out
        return out, want.to(self.dev), outside_unchanged(before, box, out), kern, ref


def plan_bytes(g: Group, a: torch.Tensor, b: torch.Tensor, M, N, K) -> int:
    """dtp_gemm_workspace for the group's operands: > 0 iff the 8-phase split-K plan applies."""
    from distributed_training_pytorch_amd import _native as nat

    args = nat.GemmArgs()
    args.A, args.B, args.M, args.N, args.K = a.data_ptr(), b.data_ptr(), M, N, K
    args.lda, args.ldb = _ld(a), _ld(b)
    args.dtype = nat.DT_BF16 if g.dtype == BF16 else nat.DT_F32
    args.out_dtype, args.trans_a, args.trans_b = nat.DT_F32, int(g.ta), int(g.tb)
    args.fast = 0 if g.fast is None else (1 if g.fast is True else -1 if g.fast is False else int(g.fast))
    return nat.load().dtp_gemm_workspace(args)


# ---------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------
COLSUM_M = (1, 3, 13, 29, 255, 256, 257, 600)
COLSUM_N = (1, 63, 64, 65, 77, 256, 264, 520)
COLSUM_GROUPS = [(dt, pl) for dt in (F32, BF16) for pl in ("aligned", "odd")]


def colsum_kernel(dtype, N, x) -> str:
    return "colsum_bf16x8" if dtype == BF16 and N % 8 == 0 and _vec(x, 8) else "colsum"


def colsum_cases(dtype, placement, device):
    """Yields (id, got, expected, outside unchanged, kernel, fp64 reference) for every M x N, fresh and accumulate."""
    gen = torch.Generator().manual_seed(zlib.crc32(f"colsum-{_DN[dtype]}-{placement}".encode()))
    for M in COLSUM_M:
        for N in COLSUM_N:
            xc = _ints(gen, (M, N), 3).to(dtype)
            old = _ints(gen, (N,), 64).float()
            x = boxed(xc, placement, float("nan"), device)[1]
            for acc in (False, True):
                ref = xc.double().sum(0) + (old.double() if acc else 0.0)
                box, out = boxed(old if acc else torch.full((N,), float("nan")), placement, SENTINEL, device)
                before = box.clone()
                ret = colsum(x, out=out, accumulate=acc)
                assert ret is out
                yield (f"{M}x{N}-{'acc' if acc else 'fresh'}", out, ref.float().to(device),
                       outside_unchanged(before, box, out), colsum_kernel(dtype, N, x), ref)


def count_cases() -> dict:
    n = {f: sum(len(g.cases) for g in groups_of(f)) for f in "abcdefh"}
    n["g"] = len(COLSUM_GROUPS) * len(COLSUM_M) * len(COLSUM_N) * 2
    return dict(sorted(n.items()))


assert all(g.K <= 2048 for g in GROUPS), "exactness needs K <= 2048"
assert len({g.id for g in GROUPS}) == len(GROUPS)

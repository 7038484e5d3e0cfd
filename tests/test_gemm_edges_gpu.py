"""Every GEMM and colsum kernel exactly at its tile, alignment and dispatch edges.

Inputs are small integers (``gemm_cases.py``), so any correct kernel with fp32 accumulation
returns the fp64 reference bit for bit: the comparisons are ``torch.equal`` (and
``assert_close(rtol=0, atol=0, equal_nan=True)`` for the non-finite cases), operands sit in
NaN-filled boxes and outputs in sentinel boxes that must come back untouched.  One test per
group (shape, dtype, layout, kernel request); a failure lists the cases of the group that
missed.  The last test is the CPU side of the same table: the condition that justifies
exact equality.
"""
import pytest
import torch

from . import gemm_cases as gc

DEV = torch.device("cuda", 0)


def _run_group(g: gc.Group, device, cpu_side=False):
    r = gc.Runner(g, device, cpu_side)
    bad = []
    for c in g.cases:
        got, want, untouched, kern, ref = r.run(c)
        why = []
        if not gc.same(got, want, g.nonfinite):
            n = (~((got == want) | (got.isnan() & want.isnan()))).sum().item()
            why.append(f"{n} of {want.numel()} elements differ from the fp64 reference")
        if not untouched:
            why.append("wrote outside the output view")
        if kern != g.kernel and not (cpu_side and g.cpu_shape):
            why.append(f"dispatch rules name {kern}")
        if cpu_side and not gc.exact_in(ref, torch.float32):
            why.append("reference is not exact in fp32")
        if cpu_side and not gc.same(ref.to(c.out_dtype), want, g.nonfinite):
            why.append("rounding the reference to the output dtype depends on the route through fp32")
        if why:
            bad.append(f"{c.id}: {'; '.join(why)}")
    assert not bad, f"{g.id}: {len(bad)} of {len(g.cases)} cases failed\n  " + "\n  ".join(bad[:12])
    return r


def _ids(gs):
    return [g.id for g in gs]


@pytest.mark.gpu
@pytest.mark.parametrize("g", gc.groups_of("a"), ids=_ids(gc.groups_of("a")))
def test_tile128_kernel(g):
    """The 128x128 kernel (fast=False or an explicit split-K): shapes that cross one M/N tile
    and the K-tile, the tile decode with and without the XCD remap, the whole epilogue set in
    both dtypes and every layout, lean and per-element operand loads, atomic split-K with
    dividing, ragged, empty and clamped slice counts."""
    _run_group(g, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("g", gc.groups_of("b"), ids=_ids(gc.groups_of("b")))
def test_skinny_k_kernel(g):
    """K <= 16 on the output-bandwidth kernel (K = 1, 2 compiled in, else read at run time),
    K = 17 on the MFMA kernel: the bf16 vector store with aux aligned and with aux in a
    misaligned view (which must take the per-element path), f32 operands to a bf16 output."""
    _run_group(g, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("g", gc.groups_of("c"), ids=_ids(gc.groups_of("c")))
def test_skinny_output_kernel(g):
    """The skinny-output weight gradient (bf16 TT, min(M, N) <= 4, K >= 64) at the edges of its
    8-row and 32-row loops and 256-row blocks, strided outputs in both orientations; the
    neighbours across each dispatch boundary fall through to the general kernel."""
    _run_group(g, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("g", gc.groups_of("d"), ids=_ids(gc.groups_of("d")))
def test_lds_dma_kernels(g):
    """The two-buffer and 8-phase LDS-DMA kernels with one K-tile, an odd K-tile count, tiles
    that are mostly clamped rows, six tiles on the persistent grid, N ragged against the
    8-column epilogue chunk; vector and per-element epilogues; broken preconditions fall back."""
    _run_group(g, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("g", gc.groups_of("e"), ids=_ids(gc.groups_of("e")))
def test_ph8_split_k_plan(g):
    """The 8-phase split-K plan on one- and two-tile problems, N % 4 != 0 and misaligned
    outputs (the scalar branch of the reduction), and its neighbour without a plan."""
    r = _run_group(g, DEV)
    a, b = r.ops("aligned", "aligned")
    assert (gc.plan_bytes(g, a, b, g.M, g.N, g.K) > 0) == (g.kernel == "ph8_splitk")


@pytest.mark.gpu
@pytest.mark.parametrize("g", gc.groups_of("f"), ids=_ids(gc.groups_of("f")))
def test_big256_register_kernel(g):
    """The 256x256 register kernel on 512 tiles of eight live rows or columns."""
    _run_group(g, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,placement", gc.COLSUM_GROUPS,
                         ids=[f"{gc._DN[d]}-{p}" for d, p in gc.COLSUM_GROUPS])
def test_colsum_edges(dtype, placement):
    """colsum at the edges of its row loops, its 256-row blocks (atomics above) and its column
    blocks, in aligned (bf16, N % 8 == 0: the 16-byte kernel) and misaligned views."""
    bad = [cid for cid, got, want, untouched, _, _ in gc.colsum_cases(dtype, placement, DEV)
           if not (torch.equal(got, want) and untouched)]
    assert not bad, f"{len(bad)} colsum cases failed: {bad[:12]}"


@pytest.mark.gpu
@pytest.mark.parametrize("g", gc.groups_of("h"), ids=_ids(gc.groups_of("h")))
def test_non_finite_values(g):
    """A NaN in the last row of A (the row clamped loads duplicate) and an Inf in the first:
    NaN and Inf exactly where the fp64 reference has them, exact values everywhere else."""
    r = _run_group(g, DEV)
    assert r.o.ab.isnan().any() and r.o.ab.isinf().any() and r.o.ab.isfinite().any()


# --- the CPU side of the same table --------------------------------------------------------
@pytest.mark.parametrize("family", list("abcdefh"))
def test_case_table_is_exact_on_cpu(family):
    """Every case of the table (family f at a cut-down shape): gemm() on CPU tensors -- the fp32
    torch path -- equals the fp64 reference bit for bit, the reference survives the round trip
    through fp32, every input survives the one through bf16, and the dispatch rules send the
    case to the kernel family the table names."""
    for g in gc.groups_of(family):
        r = _run_group(g, "cpu", cpu_side=True)
        o = r.o
        for t in (o.A, o.B, o.bias, o.aux, o.old):
            assert gc.exact_in(t.double(), torch.bfloat16), g.id
        assert o.ab.abs()[o.ab.isfinite()].max() < 2 ** 15, g.id


@pytest.mark.parametrize("dtype,placement", gc.COLSUM_GROUPS,
                         ids=[f"{gc._DN[d]}-{p}" for d, p in gc.COLSUM_GROUPS])
def test_colsum_table_is_exact_on_cpu(dtype, placement):
    kernels = set()
    for cid, got, want, untouched, kern, ref in gc.colsum_cases(dtype, placement, "cpu"):
        assert torch.equal(got, want) and untouched and gc.exact_in(ref, torch.float32), cid
        kernels.add(kern)
    # the aligned bf16 view reaches the 16-byte kernel, every other view the generic one
    assert kernels == ({"colsum", "colsum_bf16x8"} if (dtype, placement) == (gc.BF16, "aligned") else {"colsum"})


def test_case_table_covers_the_dispatch():
    names = {g.kernel for g in gc.GROUPS}
    assert names == {"tile128", "tile128_atomic", "skinny_k", "skinny_out", "dma2", "ph8", "ph8_persistent",
                     "ph8_splitk", "big256"}

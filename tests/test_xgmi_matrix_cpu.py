"""The CPU side of ``tests/xgmi_cases.py``: the stand-alone all-reduce's payloads are what the
exact comparison of ``tests/test_xgmi_matrix_gpu.py`` assumes them to be."""
import pytest
import torch

from . import xgmi_cases as xc


def test_sizes_cover_the_workgroup_edges_and_both_parities():
    assert xc.AR_CAP % 1024 == 4 and -(-xc.AR_CAP // 1024) == 5
    assert xc.AR_SIZES == [4100, 1, 3, 4, 5, 4100, 1023, 1024, 1025, 4097, 4100]
    # a workgroup counts the calls that reach it: parities seen by workgroup b (1024 floats each)
    for b in range(5):
        calls = [c for c, n in enumerate(xc.AR_SIZES) if n > 1024 * b]
        assert len(calls) >= 3 and xc.AR_SIZES[calls[-1]] == xc.AR_CAP
    # a short call is followed by a long one of the same parity of workgroup 0 (every call reaches it)
    assert any(xc.AR_SIZES[c] < 8 and xc.AR_SIZES[d] == xc.AR_CAP and (d - c) % 2 == 0
               for c in range(11) for d in range(c + 1, 11))


@pytest.mark.parametrize("world", xc.AR_WORLDS)
def test_integer_payloads_sum_exactly_in_fp32(world):
    """Integer-valued floats whose partial sums stay below 2^24: every order of the sum, and the
    multiply by 2^-3, is exact -- the CPU loop, the int64 sum and the kernel must agree."""
    for c, n in enumerate(xc.AR_SIZES):
        if xc.ar_kind(c) != "int":
            continue
        xs = [xc.ar_payload(world, r, c) for r in range(world)]
        assert all(x.shape == (n,) and torch.equal(x, x.round()) and x.abs().max() <= 2 ** 15 for x in xs)
        part = torch.zeros(n, dtype=torch.int64)
        for x in xs:
            part = part + x.long()
            assert part.abs().max() < 2 ** 24
        assert torch.equal(xc.ar_reference(xs, xc.ar_scale(world, c)).double(), part.double() * xc.INT_SCALE)


@pytest.mark.parametrize("world", xc.AR_WORLDS)
def test_real_payloads_have_no_denormals_and_the_planted_values(world):
    tiny = torch.finfo(torch.float32).tiny
    for c, n in enumerate(xc.AR_SIZES):
        if xc.ar_kind(c) != "normal":
            continue
        xs = [xc.ar_payload(world, r, c) for r in range(world)]
        ref = xc.ar_reference(xs, xc.ar_scale(world, c))
        for x in xs + [ref]:
            fin = x[torch.isfinite(x) & (x != 0)]
            assert fin.abs().min() >= 2.0 ** -60 > tiny  # and every partial sum is one of these or coarser
        if n >= 1023:  # the scales span 2^-20 .. 2^20
            mag = xs[0].abs()[torch.isfinite(xs[0])]
            assert mag.max() > 2.0 ** 18 and mag.min() < 2.0 ** -18
        if c == xc.AR_SPECIAL_CALL:
            assert n == xc.AR_CAP and torch.isnan(ref).sum() == 4 and torch.isinf(ref).sum() == 3
            assert ref[2] == 0 and not torch.signbit(ref[2])  # -0 from every rank onto the +0 start
            assert all(torch.signbit(x[2]) for x in xs)
        else:
            assert torch.isfinite(ref).all()


def test_late_ranks_differ_and_include_the_highest():
    for world in xc.AR_WORLDS:
        late = [xc.ar_late_rank(world, c) for c in range(len(xc.AR_SIZES))]
        assert late[0] == world - 1 and late[1] is None
        assert len({r for r in late if r is not None}) >= min(world, 5)


def test_same_bits_tells_zero_signs_and_one_ulp():
    a = torch.tensor([1.0, 0.0, float("nan")])
    assert xc.same_bits(a, a.clone())
    assert not xc.same_bits(a, torch.tensor([1.0, -0.0, float("nan")]))
    assert not xc.same_bits(a, torch.tensor([1.0 + 2.0 ** -23, 0.0, float("nan")]))
    assert not xc.same_bits(a, torch.tensor([1.0, 0.0, 0.0]))

"""The split-K plan of the FP8 / MXFP8 GEMMs (host code in libdtp.so, no GPU needed) and the CPU definition
of ``split_k``: the same sum, the forbidden combinations refused."""
import pytest
import torch

from distributed_training_pytorch_amd.ops.fp8 import gemm_fp8
from distributed_training_pytorch_amd.ops.mxfp8 import gemm_mxfp8

from . import fp8_cases as fc


# expected slice counts: gemm_epi.h's rule with kF8SplitMinTiles = 8 (the largest power of two S with
# tiles * S <= 256 and at least 8 128-byte K-tiles in every slice)
@pytest.mark.parametrize("M,N,K,splits", [
    (2048, 2048, 8192, 4),   # dW of a 2048-wide layer, batch 8192: 64 tiles x 4 slices of 16
    (1024, 1024, 8192, 8),   # dW of a 1024-wide layer: 16 tiles x 8 slices of 8
    (520, 264, 4224, 4),     # ragged: 6 tiles, 33 K-tiles -> slices of 8, 8, 8, 9
    (4096, 4096, 8192, 0),   # 256 tiles fill the chip
    (1024, 1024, 1920, 0),   # 15 K-tiles: two slices would drop below 8
])
@pytest.mark.parametrize("which", ["fp8", "mxfp8"])
def test_f8_split_k_plan(which, M, N, K, splits):
    from distributed_training_pytorch_amd import _native as nat

    try:
        lib = nat.load()
    except nat.NativeUnavailable as e:
        pytest.skip(f"native library not built: {e}")
    a, query = ((nat.GemmFp8Args(), lib.dtp_gemm_fp8_workspace) if which == "fp8" else
                (nat.GemmMxArgs(), lib.dtp_gemm_mxfp8_workspace))
    a.M, a.N, a.K, a.out_dtype = M, N, K, nat.DT_F32
    assert query(a) == 4 * splits * M * N
    if not splits:
        return
    a.out_dtype = nat.DT_BF16  # a bf16 output never splits
    assert query(a) == 0
    a.out_dtype, a.aux = nat.DT_F32, 256  # nor one with an aux operand (nothing is dereferenced)
    assert query(a) == 0
    a.aux = None
    if which == "mxfp8":  # K <= 2048 goes to the short-K instance unless instance = 1
        a.M, a.N, a.K = 256, 256, 2048
        assert query(a) == 0
        a.instance = 1
        assert query(a) == 4 * 2 * 256 * 256  # 16 K-tiles: two slices of 8


@pytest.mark.parametrize("fmt_a", ["e4m3", "e5m2"])
def test_split_k_on_cpu_tensors_is_the_same_sum(fmt_a):
    a, b, kw, want = fc.fp8_case(272, 264, 400, fmt_a, "none", "fwd")
    assert torch.equal(gemm_fp8(a, b, split_k=3, **kw), gemm_fp8(a, b, **kw))
    assert torch.equal(gemm_fp8(a, b, split_k=3, **kw), want)
    a, b, kw, want = fc.mx_case(256, 256, 416, fmt_a, "none", "fwd")
    assert torch.equal(gemm_mxfp8(a, b, split_k=2, instance=1, **kw), gemm_mxfp8(a, b, **kw))


@pytest.mark.parametrize("which,K,kw", [
    ("fp8", 400, dict(split_k=0)),
    ("fp8", 400, dict(split_k=2, act=True)),
    ("fp8", 400, dict(split_k=2, out_dtype=torch.bfloat16)),
    ("fp8", 400, dict(split_k=2, mfma=1)),
    ("fp8", 400, dict(split_k=5)),    # 4 K-tiles
    ("fp8", 256, dict(split_k=2)),    # the short-K instance
    ("mxfp8", 416, dict(split_k=2)),  # K <= 2048 without instance = 1
], ids=str)
def test_split_k_forbidden_combinations_on_cpu(which, K, kw):
    a, b, base, _ = (fc.fp8_case if which == "fp8" else fc.mx_case)(16, 16, K, "e4m3", "none", "fwd")
    with pytest.raises(ValueError):
        (gemm_fp8 if which == "fp8" else gemm_mxfp8)(a, b, **{**base, **kw})

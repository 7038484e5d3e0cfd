// MXFP8 quantiser for gfx950 (CDNA4): OCP e4m3 / e5m2 with one E8M0 power-of-two scale per 32
// elements along the contraction, the operands of gemm_mxfp8.hip.  For a block with a = max|x|:
//   s = a == 0 ? 127 : max(expfield(a) - emax, 0)         (emax 8 / 15; expfield <= 254, so s <= 246)
//   q = cvt_rne(clamp(x * 2^(127 - s), -fmax, fmax))      (the multiplier is built from its bits)
// A block's scale depends on that block alone: one launch, no workspace, no host read, so the
// call can sit in a captured graph.  ops/mxfp8.py holds the torch definition of the same bits.
//
// Design: one workgroup (256 threads) per 64 (M) x 128 (K) tile of x.
//  * load: x is read once, 16-byte vectors, lane-linear along K (vector v = tid + 256 j is chunk
//    v % VPR of row v / VPR; VPR = 32 f32 / 16 bf16 vectors per tile row).  An MX block is 8 (f32)
//    or 4 (bf16) adjacent lanes of one wave: the row-block maximum of the |x| bit patterns is
//    2-3 xor-shuffles, every lane of the block then holds the scale byte, casts its own vector
//    and drops the FP8 word(s) into a byte image of the tile (row stride 144 B).  The first
//    lane of a block writes the scale byte into a [64][4] byte image: a tile row's four scales
//    are one aligned dword, the four scales of a 128-byte GEMM K-tile.
//  * the same vector is parked in LDS in source precision (row stride 128 * elsize + 16 B,
//    16-byte aligned for the ds_write_b128): the transposed copy is quantised for ITS
//    contraction, blocks of 32 along M, so it needs the unrounded values, not the row-major bytes.
//  * row-major copy: 16-byte reads of the byte image, lane-linear, 16-byte stores (two per
//    thread); scales: one dword store per tile row.  Scale bytes past K / 32 are 127: inside the
//    tile they are the scales of all-zero blocks, and the last K-tile fills the rest of the row.
//  * transposed copy: thread (mb = tid >> 7, k = tid & 127) owns the column block rows
//    32 mb .. +32 of column k: 32 LDS reads down the column.  mb is uniform in a wave and the 64
//    lanes read 64 consecutive elements of one tile row, 256 (f32) or 128 (bf16) contiguous
//    bytes: conflict-free whatever the row stride, which is why the stride only has to keep the
//    vector writes aligned.  Rows past M are zeros in the image, so a ragged last block takes its
//    scale from its valid elements and its padding bytes are zeros.  The 32 bytes leave as two
//    16-byte stores to qT[k][m0 + 32 mb ..]; the two scale bytes of a column meet in LDS and
//    leave as one 2-byte store (the last M-tile fills the row with 127s).
#include "dtp_api.h"
#include "dtp_common.h"

namespace dtp {
namespace mxq {

constexpr int kTM = 64, kTK = 128;
constexpr int kImgW = 36;  // byte image row stride in 4-byte words (128 B + 16)

// |x| bit patterns of one 16-byte vector, as f32 bit patterns
template <int DT>
DTP_DEV uint32_t vec_absmax(const uint4& g) {
  const uint32_t w[4] = {g.x, g.y, g.z, g.w};
  uint32_t m = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if constexpr (DT == DTP_DT_F32) m = max(m, w[q] & 0x7fffffffu);
    else m = max(m, max((w[q] << 16) & 0x7fff0000u, w[q] & 0x7fff0000u));
  }
  return m;
}

// 16 bytes of x: one vector load, or element loads where x is only element-aligned (a weight
// that is a view into a flat parameter buffer at an odd offset)
template <int DT, bool VEC>
DTP_DEV uint4 load16(const char* p) {
  if constexpr (VEC) {
    return *reinterpret_cast<const uint4*>(p);
  } else if constexpr (DT == DTP_DT_F32) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
    return make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    const uint16_t* h = reinterpret_cast<const uint16_t*>(p);
    return make_uint4(h[0] | (uint32_t(h[1]) << 16), h[2] | (uint32_t(h[3]) << 16), h[4] | (uint32_t(h[5]) << 16),
                      h[6] | (uint32_t(h[7]) << 16));
  }
}

// the E8M0 byte of a block whose largest |x| has the f32 bit pattern `am`
template <int FMT>
DTP_DEV uint32_t scale_byte(uint32_t am) {
  constexpr int emax = FMT == DTP_FP8_E4M3 ? 8 : 15;
  return am == 0 ? 127u : static_cast<uint32_t>(max(static_cast<int>(am >> 23) - emax, 0));
}

// 2^(127 - s): exponent field 254 - s >= 8, always a normal number
DTP_DEV float scale_mul(uint32_t s) { return __uint_as_float((254u - s) << 23); }

template <int FMT>
DTP_DEV uint32_t cvt4(float a, float b, float c, float d, float mul) {
  constexpr float fmax = FMT == DTP_FP8_E4M3 ? 448.f : 57344.f;
  a = fminf(fmaxf(a * mul, -fmax), fmax);
  b = fminf(fmaxf(b * mul, -fmax), fmax);
  c = fminf(fmaxf(c * mul, -fmax), fmax);
  d = fminf(fmaxf(d * mul, -fmax), fmax);
  int w = 0;
  if constexpr (FMT == DTP_FP8_E4M3) {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
  }
  return static_cast<uint32_t>(w);
}

template <int DT, int FMT, bool VEC>
__global__ __launch_bounds__(256) void quantize_kernel(const char* x, long long ldx, int M, int K, uint8_t* q, long long ldq,
                                                       uint8_t* s, long long lds, uint8_t* qT, long long ldt, uint8_t* sT,
                                                       long long ldst) {
  constexpr int ES = DT == DTP_DT_F32 ? 4 : 2, EPV = 16 / ES;
  constexpr int VPR = kTK / EPV;         // vectors per tile row
  constexpr int NV = kTM * VPR / 256;    // vectors per thread
  constexpr int LPB = 32 / EPV;          // lanes per MX block
  constexpr int SB = kTK * ES + 16;      // source image row stride in bytes
  __shared__ __align__(16) char src[kTM * SB];
  __shared__ __align__(16) uint32_t img[kTM * kImgW];
  __shared__ uint32_t srow[kTM];
  __shared__ uint16_t scol[kTK];
  const int tid = threadIdx.x;
  const int k0 = blockIdx.x * kTK, m0 = blockIdx.y * kTM;

#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = tid + 256 * j, row = v / VPR, c = v % VPR;
    uint4 g = make_uint4(0, 0, 0, 0);
    if (m0 + row < M && k0 + c * EPV < K)
      g = load16<DT, VEC>(x + (static_cast<long long>(m0 + row) * ldx + k0 + c * EPV) * ES);
    *reinterpret_cast<uint4*>(src + row * SB + c * 16) = g;
    uint32_t am = vec_absmax<DT>(g);
#pragma unroll
    for (int o = 1; o < LPB; o <<= 1) am = max(am, static_cast<uint32_t>(__shfl_xor(static_cast<int>(am), o, kWave)));
    const uint32_t sb = scale_byte<FMT>(am);
    const float mul = scale_mul(sb);
    const uint32_t h[4] = {g.x, g.y, g.z, g.w};
    if constexpr (DT == DTP_DT_F32) {
      img[row * kImgW + c] =
          cvt4<FMT>(__uint_as_float(h[0]), __uint_as_float(h[1]), __uint_as_float(h[2]), __uint_as_float(h[3]), mul);
    } else {
      float f[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f[2 * e] = __uint_as_float(h[e] << 16);
        f[2 * e + 1] = __uint_as_float(h[e] & 0xffff0000u);
      }
      img[row * kImgW + 2 * c] = cvt4<FMT>(f[0], f[1], f[2], f[3], mul);
      img[row * kImgW + 2 * c + 1] = cvt4<FMT>(f[4], f[5], f[6], f[7], mul);
    }
    if (c % LPB == 0) reinterpret_cast<uint8_t*>(srow)[row * 4 + c / LPB] = static_cast<uint8_t>(sb);
  }
  __syncthreads();

  // row-major copy: 16 k of one row per vector, lane-linear
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int v = tid + 256 * j, row = v >> 3, c = v & 7;
    if (m0 + row < M && k0 + 16 * c < K)
      *reinterpret_cast<uint4*>(q + static_cast<long long>(m0 + row) * ldq + k0 + 16 * c) =
          *reinterpret_cast<const uint4*>(img + row * kImgW + 4 * c);
  }
  if (tid < kTM && m0 + tid < M) {
    uint32_t* srow_g = reinterpret_cast<uint32_t*>(s + static_cast<long long>(m0 + tid) * lds);
    srow_g[blockIdx.x] = srow[tid];
    if (blockIdx.x == gridDim.x - 1)
      for (int d = gridDim.x; d < static_cast<int>(lds >> 2); ++d) srow_g[d] = 0x7f7f7f7fu;
  }
  if (!qT) return;  // (uniform)

  // transposed copy: one column block (32 rows of one k) per thread
  const int mb = tid >> 7, k = tid & 127;
  const int Mp = (M + 31) & ~31;
  float f[32];
  uint32_t am = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const char* p = src + (32 * mb + i) * SB + k * ES;
    uint32_t bits;
    if constexpr (DT == DTP_DT_F32) bits = *reinterpret_cast<const uint32_t*>(p);
    else bits = static_cast<uint32_t>(*reinterpret_cast<const uint16_t*>(p)) << 16;
    f[i] = __uint_as_float(bits);
    am = max(am, bits & 0x7fffffffu);
  }
  const uint32_t sb = scale_byte<FMT>(am);
  const float mul = scale_mul(sb);
  reinterpret_cast<uint8_t*>(scol)[2 * k + mb] = static_cast<uint8_t>(sb);
  if (k0 + k < K && m0 + 32 * mb < Mp) {
    uint32_t w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = cvt4<FMT>(f[4 * e], f[4 * e + 1], f[4 * e + 2], f[4 * e + 3], mul);
    uint4* o = reinterpret_cast<uint4*>(qT + static_cast<long long>(k0 + k) * ldt + m0 + 32 * mb);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
  __syncthreads();
  if (tid < kTK && k0 + tid < K) {
    uint16_t* scol_g = reinterpret_cast<uint16_t*>(sT + static_cast<long long>(k0 + tid) * ldst);
    scol_g[blockIdx.y] = scol[tid];
    if (blockIdx.y == gridDim.y - 1)
      for (int d = gridDim.y; d < static_cast<int>(ldst >> 1); ++d) scol_g[d] = 0x7f7fu;
  }
}

template <int DT, bool VEC>
static void launch(const void* x, long long ldx, int M, int K, int fmt, void* q, long long ldq, void* s, long long lds,
                   void* qT, long long ldt, void* sT, long long ldst, hipStream_t st) {
  const dim3 g((K + kTK - 1) / kTK, (M + kTM - 1) / kTM);
  const char* xc = static_cast<const char*>(x);
  auto *q8 = static_cast<uint8_t*>(q), *s8 = static_cast<uint8_t*>(s), *t8 = static_cast<uint8_t*>(qT),
       *st8 = static_cast<uint8_t*>(sT);
  if (fmt == DTP_FP8_E4M3)
    hipLaunchKernelGGL((quantize_kernel<DT, DTP_FP8_E4M3, VEC>), g, dim3(256), 0, st, xc, ldx, M, K, q8, ldq, s8, lds, t8, ldt,
                       st8, ldst);
  else
    hipLaunchKernelGGL((quantize_kernel<DT, DTP_FP8_E5M2, VEC>), g, dim3(256), 0, st, xc, ldx, M, K, q8, ldq, s8, lds, t8, ldt,
                       st8, ldst);
}

}  // namespace mxq
}  // namespace dtp

extern "C" int dtp_mxfp8_quantize(const void* x, long long ldx, int M, int K, int dtype, int fmt, void* q, long long ldq,
                                  void* s, long long lds, void* qT, long long ldt, void* sT, long long ldst, void* stream) {
  using namespace dtp;
  if (!x || !q || !s || M <= 0 || K <= 0) return set_err(1, "dtp_mxfp8_quantize: bad arguments");
  if (dtype != DTP_DT_F32 && dtype != DTP_DT_BF16) return set_err(1, "dtp_mxfp8_quantize: x must be f32 or bf16");
  if (fmt != DTP_FP8_E4M3 && fmt != DTP_FP8_E5M2) return set_err(1, "dtp_mxfp8_quantize: format must be e4m3 or e5m2");
  const int epv = dtype == DTP_DT_F32 ? 4 : 8;
  auto al = [](const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
  if (K % 32 || ldx < K || ldq < K || ldq % 16 || !al(q, 16))
    return set_err(1, "dtp_mxfp8_quantize: K must be a multiple of 32 and every output row 16-byte aligned");
  if (lds % 4 || lds < 4 * ((K + 127) / 128) || !al(s, 4))
    return set_err(1, "dtp_mxfp8_quantize: scale rows must be 4-byte aligned and hold 4 bytes per 128 of K");
  const bool vec = ldx % epv == 0 && al(x, 16);  // else x is read element by element
  if (qT) {
    const int Mp = (M + 31) / 32 * 32;
    if (!sT || ldt % 16 || ldt < Mp || !al(qT, 16) || ldst % 4 || ldst < 4 * ((Mp + 127) / 128) || !al(sT, 4))
      return set_err(1, "dtp_mxfp8_quantize: the transposed copy needs rows of M rounded up to 32 bytes and its scale rows");
  }
  if ((M + mxq::kTM - 1) / mxq::kTM > 65535) return set_err(1, "dtp_mxfp8_quantize: M too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == DTP_DT_F32)
    vec ? mxq::launch<DTP_DT_F32, true>(x, ldx, M, K, fmt, q, ldq, s, lds, qT, ldt, sT, ldst, st)
        : mxq::launch<DTP_DT_F32, false>(x, ldx, M, K, fmt, q, ldq, s, lds, qT, ldt, sT, ldst, st);
  else
    vec ? mxq::launch<DTP_DT_BF16, true>(x, ldx, M, K, fmt, q, ldq, s, lds, qT, ldt, sT, ldst, st)
        : mxq::launch<DTP_DT_BF16, false>(x, ldx, M, K, fmt, q, ldq, s, lds, qT, ldt, sT, ldst, st);
  return check_launch("dtp_mxfp8_quantize");
}

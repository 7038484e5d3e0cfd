// Per-tensor scaled FP8 quantiser for gfx950 (CDNA4): OCP e4m3 / e5m2, the operand
// formats of gemm_fp8.hip.  q = cvt(x * scale), scale = min(fmax / amax|x|, 2^126) formed and
// kept on the device (no host read: the pair of launches can sit in a captured graph).
//
//  * amax_kernel: at most 1024 workgroups walk x in 16-byte vectors and each writes the
//    maximum of its |x| bit patterns (an unsigned compare orders non-negative floats) to
//    its own workspace slot: no atomics, no slot to clear, and max is order-independent,
//    so the result is deterministic.
//  * quantize_kernel: every workgroup first reduces the <= 1024 partials itself (4 loads
//    per thread, L2 hits) and forms the scale; workgroup (0, 0) publishes scale and
//    1 / scale.  Then one 64 x 64 tile per workgroup: x is read once in 16-byte vectors,
//    scaled in fp32, converted by the packed hardware convert (round to nearest even) and
//    parked in LDS as a [64][64] byte image (row stride 68 B).  The row-major copy leaves as
//    one 16-byte store per thread (16 k of one row); the transposed copy as one 16-byte
//    store per thread too: 16 rows of one k, gathered from the image by byte reads
//    (lanes 4 k .. 4 k + 3 read one word, the stride-17-word rows spread the k).
//    The GEMM then only ever sees K-contiguous operands.
//  * qT rows are padded to a multiple of 16 bytes by the caller (ldt); the bytes past M are
//    written as zeros, so a GEMM over the padded row adds exact zeros.
//
// Delayed scaling (the scale from the amaxes of earlier steps, DtpFp8ScaleRec): the scale is known
// before the tensor is, so one launch suffices.
//  * quantize_kernel<.., GIVEN = true> reads the scale from a device pointer, clamps x * scale to
//    +-fmax (a stale scale must saturate, not turn into NaN / infinity) and writes the amax of its
//    own 64 x 64 tile as one partial: x is read once where the current-amax recipe reads it twice.
//  * amax_kernel<.., COUNT = true> is the first launch on its own, in the record's layout (seeding).
//  * scale_update_kernel: one workgroup per record reduces the partials, pushes the amax into the
//    record's ring and forms the scale from the ring's maximum with the same capped division.
#include <algorithm>

#include "dtp_api.h"
#include "dtp_common.h"

namespace dtp {
namespace fp8 {

constexpr int kParts = DTP_FP8_WS_FLOATS - 2;
constexpr int kTile = 64;
constexpr int kStrideW = 17;  // LDS row stride in 4-byte words

DTP_DEV uint32_t block_max(uint32_t v, uint32_t* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o, kWave)));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  v = max(max(red[0], red[1]), max(red[2], red[3]));
  __syncthreads();
  return v;
}

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

// COUNT: the record layout of DtpFp8ScaleRec::partials (word 0 the count, then the partials)
template <int DT, bool VEC, bool COUNT = false>
__global__ __launch_bounds__(256) void amax_kernel(const char* x, long long ldx, int M, int K, uint32_t* part) {
  __shared__ uint32_t red[4];
  constexpr int ES = DT == DTP_DT_F32 ? 4 : 2, EPV = 16 / ES;
  const int vpr = K / EPV;  // vectors per row
  const long long total = static_cast<long long>(M) * vpr;
  uint32_t m = 0;
  for (long long v = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; v < total; v += 256LL * gridDim.x) {
    const long long row = v / vpr;
    const int c = static_cast<int>(v - row * vpr);
    m = max(m, vec_absmax<DT>(load16<DT, VEC>(x + (row * ldx + c * EPV) * ES)));
  }
  m = block_max(m, red, threadIdx.x);
  if constexpr (COUNT) {
    if (threadIdx.x == 0) part[1 + blockIdx.x] = m;
    if (threadIdx.x == 0 && blockIdx.x == 0) part[0] = gridDim.x;
  } else {
    if (threadIdx.x == 0) part[blockIdx.x] = m;
  }
}

template <int FMT>
DTP_DEV uint32_t cvt4(float a, float b, float c, float d) {
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

DTP_DEV float clamp_abs(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// GIVEN = false: ws = {scale, 1 / scale, nparts amax partials}, the scale formed here.
// GIVEN = true: ws points at the scale (read only); x * scale is clamped to +-fmax and the tile's amax goes
// to part[1 + tile], the tile count to part[0] (the layout of DtpFp8ScaleRec::partials).
template <int DT, int FMT, bool VEC, bool GIVEN = false>
__global__ __launch_bounds__(256) void quantize_kernel(const char* x, long long ldx, int M, int K, uint8_t* q,
                                                       long long ldq, uint8_t* qT, long long ldt, float* ws, int nparts,
                                                       uint32_t* part_out) {
  __shared__ uint32_t red[4];
  __shared__ uint32_t tile[kTile * kStrideW];
  const int tid = threadIdx.x;
  constexpr float fmax = FMT == DTP_FP8_E4M3 ? 448.f : 57344.f;
  float scale;
  if constexpr (GIVEN) {
    scale = *ws;
  } else {
    const uint32_t* part = reinterpret_cast<const uint32_t*>(ws + 2);
    uint32_t mb = 0;
    for (int i = tid; i < nparts; i += 256) mb = max(mb, part[i]);
    const float amax = __uint_as_float(block_max(mb, red, tid));
    // capped at 2^126: below amax = fmax / FLT_MAX the quotient is infinite, 1 / scale then 0 and
    // every output 0 * inf = NaN; with the cap 1 / scale stays a normal number
    scale = amax > 0.f ? fminf(fmax / amax, 0x1p126f) : 1.f;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
      ws[0] = scale;
      ws[1] = 1.f / scale;
    }
  }
  // GIVEN: x * scale clamped (a no-op otherwise: |x| scale <= fmax by the scale's definition)
  auto sc = [&](float v) { return GIVEN ? clamp_abs(v * scale, fmax) : v * scale; };
  uint32_t tmax = 0;  // GIVEN: the |x| bit patterns this thread loaded
  const int k0 = blockIdx.x * kTile, m0 = blockIdx.y * kTile;

  // x tile -> fp8 words in LDS (rows past M and columns past K as zero bytes)
  if constexpr (DT == DTP_DT_F32) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = tid + 256 * j, row = v >> 4, c = v & 15;
      uint32_t w = 0;
      if (m0 + row < M && k0 + 4 * c < K) {
        const uint4 f = load16<DT, VEC>(x + (static_cast<long long>(m0 + row) * ldx + k0 + 4 * c) * 4);
        if constexpr (GIVEN) tmax = max(tmax, vec_absmax<DT>(f));
        w = cvt4<FMT>(sc(__uint_as_float(f.x)), sc(__uint_as_float(f.y)), sc(__uint_as_float(f.z)), sc(__uint_as_float(f.w)));
      }
      tile[row * kStrideW + c] = w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = tid + 256 * j, row = v >> 3, c = v & 7;
      uint32_t w0 = 0, w1 = 0;
      if (m0 + row < M && k0 + 8 * c < K) {
        const uint4 g = load16<DT, VEC>(x + (static_cast<long long>(m0 + row) * ldx + k0 + 8 * c) * 2);
        const uint32_t h[4] = {g.x, g.y, g.z, g.w};
        if constexpr (GIVEN) tmax = max(tmax, vec_absmax<DT>(g));
        float f[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f[2 * e] = sc(__uint_as_float(h[e] << 16));
          f[2 * e + 1] = sc(__uint_as_float(h[e] & 0xffff0000u));
        }
        w0 = cvt4<FMT>(f[0], f[1], f[2], f[3]);
        w1 = cvt4<FMT>(f[4], f[5], f[6], f[7]);
      }
      tile[row * kStrideW + 2 * c] = w0;
      tile[row * kStrideW + 2 * c + 1] = w1;
    }
  }
  if constexpr (GIVEN) {  // (block_max ends with a barrier: the tile image is complete behind it)
    tmax = block_max(tmax, red, tid);
    if (tid == 0) part_out[1 + blockIdx.y * gridDim.x + blockIdx.x] = tmax;
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) part_out[0] = gridDim.x * gridDim.y;
  } else {
    __syncthreads();
  }

  {  // row-major copy: 16 k of one row per thread
    const int row = tid >> 2, seg = tid & 3;
    if (m0 + row < M && k0 + 16 * seg < K) {
      const uint32_t* t = tile + row * kStrideW + 4 * seg;
      *reinterpret_cast<uint4*>(q + static_cast<long long>(m0 + row) * ldq + k0 + 16 * seg) = make_uint4(t[0], t[1], t[2], t[3]);
    }
  }
  if (qT) {  // transposed copy: 16 rows of one k per thread
    const int k = tid >> 2, mg = tid & 3;
    if (k0 + k < K && m0 + 16 * mg < M) {
      const uint8_t* tb = reinterpret_cast<const uint8_t*>(tile) + (16 * mg) * (kStrideW * 4) + k;
      uint32_t w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        w[e] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w[e] |= static_cast<uint32_t>(tb[(4 * e + b) * (kStrideW * 4)]) << (8 * b);
      }
      *reinterpret_cast<uint4*>(qT + static_cast<long long>(k0 + k) * ldt + m0 + 16 * mg) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

template <int DT, bool VEC>
static void launch(const void* x, long long ldx, int M, int K, int fmt, void* q, long long ldq, void* qT, long long ldt,
                   float* ws, hipStream_t s) {
  constexpr int EPV = DT == DTP_DT_F32 ? 4 : 8;
  const long long vecs = static_cast<long long>(M) * (K / EPV);
  const int nparts = static_cast<int>(std::min<long long>(kParts, (vecs + 1023) / 1024));  // >= 4 vectors per thread
  const char* xc = static_cast<const char*>(x);
  hipLaunchKernelGGL((amax_kernel<DT, VEC>), dim3(nparts), dim3(256), 0, s, xc, ldx, M, K, reinterpret_cast<uint32_t*>(ws + 2));
  const dim3 g((K + kTile - 1) / kTile, (M + kTile - 1) / kTile);
  auto* q8 = static_cast<uint8_t*>(q);
  auto* t8 = static_cast<uint8_t*>(qT);
  if (fmt == DTP_FP8_E4M3)
    hipLaunchKernelGGL((quantize_kernel<DT, DTP_FP8_E4M3, VEC>), g, dim3(256), 0, s, xc, ldx, M, K, q8, ldq, t8, ldt, ws, nparts,
                       nullptr);
  else
    hipLaunchKernelGGL((quantize_kernel<DT, DTP_FP8_E5M2, VEC>), g, dim3(256), 0, s, xc, ldx, M, K, q8, ldq, t8, ldt, ws, nparts,
                       nullptr);
}

template <int DT, bool VEC>
static int launch_amax(const void* x, long long ldx, int M, int K, uint32_t* part, int cap, hipStream_t s) {
  constexpr int EPV = DT == DTP_DT_F32 ? 4 : 8;
  const long long vecs = static_cast<long long>(M) * (K / EPV);
  const int nparts = static_cast<int>(std::min<long long>(kParts, (vecs + 1023) / 1024));
  if (nparts > cap) return set_err(1, "dtp_fp8_amax: the partials buffer is too small");
  hipLaunchKernelGGL((amax_kernel<DT, VEC, true>), dim3(nparts), dim3(256), 0, s, static_cast<const char*>(x), ldx, M, K, part);
  return check_launch("dtp_fp8_amax");
}

template <int DT, bool VEC>
static void launch_scaled(const void* x, long long ldx, int M, int K, int fmt, void* q, long long ldq, void* qT,
                          long long ldt, const float* scale, uint32_t* part, hipStream_t s) {
  const dim3 g((K + kTile - 1) / kTile, (M + kTile - 1) / kTile);
  const char* xc = static_cast<const char*>(x);
  auto* q8 = static_cast<uint8_t*>(q);
  auto* t8 = static_cast<uint8_t*>(qT);
  float* sp = const_cast<float*>(scale);  // (read only in the GIVEN instances)
  if (fmt == DTP_FP8_E4M3)
    hipLaunchKernelGGL((quantize_kernel<DT, DTP_FP8_E4M3, VEC, true>), g, dim3(256), 0, s, xc, ldx, M, K, q8, ldq, t8, ldt, sp, 0, part);
  else
    hipLaunchKernelGGL((quantize_kernel<DT, DTP_FP8_E5M2, VEC, true>), g, dim3(256), 0, s, xc, ldx, M, K, q8, ldq, t8, ldt, sp, 0, part);
}

// One workgroup per record, a thread per partial / ring slot (strided where there are more than 256).
__global__ __launch_bounds__(256) void scale_update_kernel(DtpFp8ScaleRec* recs) {
  __shared__ uint32_t red[4];
  const DtpFp8ScaleRec r = recs[blockIdx.x];
  const int tid = threadIdx.x;
  const int n = min(static_cast<int>(r.partials[0]), r.cap);
  uint32_t m = 0;
  for (int i = tid; i < n; i += 256) m = max(m, r.partials[1 + i]);
  m = block_max(m, red, tid);  // (its barriers: every thread has read the count before thread 0 clears it)
  if (tid == 0 && n > 0) {
    const int p = *r.pos;
    r.history[p] = __uint_as_float(m);
    *r.pos = p + 1 < r.H ? p + 1 : 0;
    r.partials[0] = 0;
  }
  __syncthreads();  // the pushed amax is visible to the workgroup
  uint32_t h = 0;
  for (int i = tid; i < r.H; i += 256) h = max(h, __float_as_uint(r.history[i]) & 0x7fffffffu);
  const float amax = __uint_as_float(block_max(h, red, tid));
  if (tid == 0) {
    const float scale = amax > 0.f ? fminf(r.fmax / amax, 0x1p126f) : 1.f;  // the division and cap of quantize_kernel
    r.scale[0] = scale;
    r.scale[1] = 1.f / scale;
  }
}

}  // namespace fp8
}  // namespace dtp

extern "C" int dtp_fp8_quantize(const void* x, long long ldx, int M, int K, int dtype, int fmt, void* q, long long ldq,
                                void* qT, long long ldt, float* ws, void* stream) {
  using namespace dtp;
  if (!x || !q || !ws || M <= 0 || K <= 0) return set_err(1, "dtp_fp8_quantize: bad arguments");
  if (dtype != DTP_DT_F32 && dtype != DTP_DT_BF16) return set_err(1, "dtp_fp8_quantize: x must be f32 or bf16");
  if (fmt != DTP_FP8_E4M3 && fmt != DTP_FP8_E5M2) return set_err(1, "dtp_fp8_quantize: format must be e4m3 or e5m2");
  const int epv = dtype == DTP_DT_F32 ? 4 : 8;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (K % 16 || ldx < K || ldq < K || ldq % 16 || !al16(q))
    return set_err(1, "dtp_fp8_quantize: K must be a multiple of 16 and every output row 16-byte aligned");
  const bool vec = ldx % epv == 0 && al16(x);  // else x is read element by element
  if (qT && (ldt % 16 || ldt < (M + 15) / 16 * 16 || !al16(qT)))
    return set_err(1, "dtp_fp8_quantize: the transposed copy needs rows of M rounded up to 16 bytes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == DTP_DT_F32)
    vec ? fp8::launch<DTP_DT_F32, true>(x, ldx, M, K, fmt, q, ldq, qT, ldt, ws, s)
        : fp8::launch<DTP_DT_F32, false>(x, ldx, M, K, fmt, q, ldq, qT, ldt, ws, s);
  else
    vec ? fp8::launch<DTP_DT_BF16, true>(x, ldx, M, K, fmt, q, ldq, qT, ldt, ws, s)
        : fp8::launch<DTP_DT_BF16, false>(x, ldx, M, K, fmt, q, ldq, qT, ldt, ws, s);
  return check_launch("dtp_fp8_quantize");
}

extern "C" int dtp_fp8_amax(const void* x, long long ldx, int M, int K, int dtype, unsigned* part, int cap, void* stream) {
  using namespace dtp;
  if (!x || !part || M <= 0 || K <= 0 || K % 16 || ldx < K) return set_err(1, "dtp_fp8_amax: bad arguments");
  if (dtype != DTP_DT_F32 && dtype != DTP_DT_BF16) return set_err(1, "dtp_fp8_amax: x must be f32 or bf16");
  const bool vec = ldx % (dtype == DTP_DT_F32 ? 4 : 8) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == DTP_DT_F32)
    return vec ? fp8::launch_amax<DTP_DT_F32, true>(x, ldx, M, K, part, cap, s) : fp8::launch_amax<DTP_DT_F32, false>(x, ldx, M, K, part, cap, s);
  return vec ? fp8::launch_amax<DTP_DT_BF16, true>(x, ldx, M, K, part, cap, s) : fp8::launch_amax<DTP_DT_BF16, false>(x, ldx, M, K, part, cap, s);
}

extern "C" int dtp_fp8_quantize_scaled(const void* x, long long ldx, int M, int K, int dtype, int fmt, void* q, long long ldq,
                                       void* qT, long long ldt, const float* scale, unsigned* part, int cap, void* stream) {
  using namespace dtp;
  if (!x || !q || !scale || !part || M <= 0 || K <= 0) return set_err(1, "dtp_fp8_quantize_scaled: bad arguments");
  if (dtype != DTP_DT_F32 && dtype != DTP_DT_BF16) return set_err(1, "dtp_fp8_quantize_scaled: x must be f32 or bf16");
  if (fmt != DTP_FP8_E4M3 && fmt != DTP_FP8_E5M2) return set_err(1, "dtp_fp8_quantize_scaled: format must be e4m3 or e5m2");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (K % 16 || ldx < K || ldq < K || ldq % 16 || !al16(q))
    return set_err(1, "dtp_fp8_quantize_scaled: K must be a multiple of 16 and every output row 16-byte aligned");
  if (qT && (ldt % 16 || ldt < (M + 15) / 16 * 16 || !al16(qT)))
    return set_err(1, "dtp_fp8_quantize_scaled: the transposed copy needs rows of M rounded up to 16 bytes");
  const long long tiles = static_cast<long long>((K + fp8::kTile - 1) / fp8::kTile) * ((M + fp8::kTile - 1) / fp8::kTile);
  if (tiles > cap) return set_err(1, "dtp_fp8_quantize_scaled: the partials buffer is too small");
  const bool vec = ldx % (dtype == DTP_DT_F32 ? 4 : 8) == 0 && al16(x);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == DTP_DT_F32)
    vec ? fp8::launch_scaled<DTP_DT_F32, true>(x, ldx, M, K, fmt, q, ldq, qT, ldt, scale, part, s)
        : fp8::launch_scaled<DTP_DT_F32, false>(x, ldx, M, K, fmt, q, ldq, qT, ldt, scale, part, s);
  else
    vec ? fp8::launch_scaled<DTP_DT_BF16, true>(x, ldx, M, K, fmt, q, ldq, qT, ldt, scale, part, s)
        : fp8::launch_scaled<DTP_DT_BF16, false>(x, ldx, M, K, fmt, q, ldq, qT, ldt, scale, part, s);
  return check_launch("dtp_fp8_quantize_scaled");
}

extern "C" int dtp_fp8_scale_update(DtpFp8ScaleRec* recs, int n_recs, void* stream) {
  using namespace dtp;
  if (!recs || n_recs <= 0) return set_err(1, "dtp_fp8_scale_update: no records");
  hipLaunchKernelGGL(fp8::scale_update_kernel, dim3(n_recs), dim3(256), 0, static_cast<hipStream_t>(stream), recs);
  return check_launch("dtp_fp8_scale_update");
}

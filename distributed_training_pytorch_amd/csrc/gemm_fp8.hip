// FP8 GEMM for gfx950 (CDNA4): the wide-MLP layer GEMMs on OCP e4m3 / e5m2 operands
// with per-tensor scales, fp32 accumulation and the fused Linear epilogues of gemm_epi.h:
//   C[M,N] (+)= epi(sa_inv * sb_inv * A(m,:) . B(n,:)),  A [M,K] and B [N,K] both K-contiguous
// (fp8_quant.hip writes the transposed copies, so no operand is ever read across its rows).
//
// Design: the eight-phase geometry of gemm_ph8.hip with K counted in bytes.
//  * block tile 256 x 256 x 128 B, 8 waves as 2 (M) x 4 (N); wave (wr, wc) owns rows
//    {wr*64 + [0,64)} and {128 + wr*64 + [0,64)}, columns {wc*32 + [0,32)} and
//    {128 + wc*32 + [0,32)}: 8 x 4 fragments, 128 accumulators, in four quadrants (qm, qn).
//  * matrix instruction: v_mfma_scale_f32_16x16x128_f8f6f4, operand formats in cbsz / blgp
//    (A e4m3 or e5m2, B e4m3), both block scales the E8M0 byte 127 = 1.0.  One instruction
//    eats a whole 128-byte K-tile of a 16 x 16 fragment: 8 per quadrant where the bf16
//    kernel issues 16, fed by the same number of LDS bytes.  The 16x16x32 fp8 / bf8 MFMAs
//    are the other instance (DtpGemmFp8Args::mfma = 1, four per fragment pair): measured
//    in this kernel at W = 4096 they reach 1599 / 1639 / 1743 TF/s (forward / dx / dW)
//    where f8f6f4 reaches 2064 / 2072 / 2270, with bit-identical results, so f8f6f4 is
//    the default (profiles/fp8_gemm/).  Neither accumulates one instruction's products
//    in full fp32: they are aligned to the largest and about 15 bits below it survive.
//  * operands by LDS-DMA (global_load_lds_dwordx4), four 16 KiB parts per K-tile (A0, A1,
//    B0, B1 = 128 rows x 128 B), two K-tile buffers + a sink: one part issued per phase,
//    s_waitcnt vmcnt(6) keeps the three youngest in flight across every barrier; waves
//    4-7 run one barrier behind their SIMD partners (the ph8 stagger).
//  * LDS image of a part: [128 rows][8 x 16-B chunks], chunk c of row r at c ^ fswz(r),
//    the swizzle applied on the DMA source address.  A lane (row lr = lane & 15, group
//    lg = lane >> 4) feeds the MFMA its 32 K-bytes as chunks lg and 4 + lg: two
//    conflict-free ds_read_b128.  Which 32 of the 128 K-bytes a lane group holds is free
//    as long as A and B agree (the sum over k commutes), so the grouping is chosen for the
//    LDS banks, not for the instruction's nominal k order.
//  * ragged M / N: rows clamped on load, guarded on store.  K % 128 != 0: the chunks of the
//    last K-tile past K are fetched from a 16-byte zero block instead (both operands: a
//    stray NaN byte times zero would still be NaN).
//  * split-K (SPLIT instances, dtp_gemm_fp8 with splitk > 1): a weight gradient of a 1024-2048-wide
//    layer is 16-64 tiles with K = batch, one workgroup per tile leaves most CUs idle.  The grid
//    becomes tiles x S, each block runs a K-slice (whole K-tiles, possibly uneven) through the
//    unchanged pipeline and stores raw fp32 partial sums to a workspace; one reduction launch
//    (f8_splitk_reduce_kernel, gemm_epi.h) sums the slices in order and applies the epilogue.
//    f8_split_plan picks S.
//  * quantised output (gemm_fp8_qout_kernel, dtp_gemm_fp8_quant): delayed scaling knows the output's scale
//    before the GEMM starts, so the epilogue also writes the FP8 copy of C, its transpose and the tile's
//    amax (gemm_epi_quant.h): the next layer's operand without a quantiser launch.  Same main loop.
//  * K <= 256 does not come here: dtp_gemm_fp8 sends short sums to gemm_fp8_short_kernel (below),
//    which decodes the same FP8 operands to f32 for the exact-fp32 MFMA.
#include <string>

#include "gemm_epi.h"
#include "gemm_epi_quant.h"

namespace dtp {
namespace gemm {
namespace f8 {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void gbl_void_t;
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 512;
constexpr int kPart = 128 * 128;     // one operand part of one K-tile (16 KiB)
constexpr int kBuf = 4 * kPart;      // parts A0, A1, B0, B1
constexpr int kSink = 2 * kBuf;      // DMA sink for the slots past the last K-tile
constexpr int kLds = kSink + kPart;  // 144 KiB
static_assert(8 * kEpiWaveFloats * 4 <= kLds, "epilogue staging must fit the operand LDS");
constexpr int kOne = 0x7f7f7f7f;     // E8M0 1.0 in every byte: the block scale whatever opsel picks

__device__ uint4 g_zero_chunk;  // source of the K-tail chunks (zero-initialised, never written)

DTP_DEV int fswz(int x) { return (x & 3) | ((x >> 1) & 4); }

// Per-lane DMA source offsets (bytes from the block's first operand row r0 at the K-tile's
// first byte) of the two wave-instructions that fill part p: instruction i of wave w
// fills part bytes [(8 i + w) KiB, +1 KiB) = 8 rows x 128 B.
DTP_DEV void part_sources(uint32_t (&off)[2][2], long long ld, int r0, int R, int wave, int lane) {
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (8 * i + wave) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ fswz(row);
      const int rr = min(r0 + 128 * p + row, R - 1) - r0;
      off[p][i] = static_cast<uint32_t>(static_cast<long long>(rr) * ld + c * 16);
    }
}

// inline asm: hipcc treats a plain LDS load as possibly aliasing the in-flight LDS-DMA and
// drains vmcnt(0) before it, which would empty the DMA pipeline every phase.  The reads
// complete under mid()'s lgkmcnt(0), pinned by its sched_barrier.
DTP_DEV i32x8 frag(const char* part, const int (&off)[2], int f) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  i32x4 lo, hi;
  const uint32_t p0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_void_t*)(part + off[0] + f * 2048)));
  const uint32_t p1 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_void_t*)(part + off[1] + f * 2048)));
  asm volatile("ds_read_b128 %0, %1" : "=v"(lo) : "v"(p0));
  asm volatile("ds_read_b128 %0, %1" : "=v"(hi) : "v"(p1));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

DTP_DEV void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// One fragment pair through the matrix unit.  X32 = false: one 16x16x128 f8f6f4 MFMA; true:
// the lane's 32 K-bytes as four 8-byte pieces through four 16x16x32 fp8 / bf8 MFMAs.
template <int FA, bool X32>
DTP_DEV f32x4 mma_frag(const i32x8& x, const i32x8& y, f32x4 c) {
  if constexpr (!X32) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(x, y, c, FA == DTP_FP8_E5M2 ? 1 : 0, 0, 0, kOne, 0, kOne);
  } else {
    typedef long i64x4 __attribute__((ext_vector_type(4)));
    const i64x4 xl = __builtin_bit_cast(i64x4, x), yl = __builtin_bit_cast(i64x4, y);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (FA == DTP_FP8_E5M2) c = __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8(xl[q], yl[q], c, 0, 0, 0);
      else c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(xl[q], yl[q], c, 0, 0, 0);
    }
    return c;
  }
}

// FA: format of A (DTP_FP8_*); B is e4m3.  X32: the 16x16x32 MFMAs instead of the 16x16x128 one.
// SPLIT: grid = tiles x a.splitk, neighbouring blocks are one tile's K-slices (f8_slice: they share
// the operand rows in L2 and differ in K offset); the block runs its slice's K-tiles through the
// same pipeline and stores raw fp32 partial sums to a.work[ks][M][N] (plain stores: the workspace
// is uninitialised and no atomic target); f8_splitk_reduce_kernel applies the epilogue.
template <int FA, bool X32, bool SPLIT>
__global__ __launch_bounds__(kThreads) void gemm_fp8_kernel(DtpGemmFp8Args a) {
  static_assert(!(X32 && SPLIT), "the 16x16x32 instance has no split twin");
#include "gemm_fp8_body.h"
  fast_epilogue_pass<0>(e, acc, ebuf, bias, m0 + wr * 64, ncol, vec, lane);
  fast_epilogue_pass<1>(e, acc, ebuf, bias, m0 + 128 + wr * 64, ncol, vec, lane);
}

// The same with the quantising epilogue (gemm_epi_quant.h): unsplit, bf16 C, no accumulate; the host sends
// only problems where the vector epilogue applies to every lane.
template <int FA, bool X32>
__global__ __launch_bounds__(kThreads) void gemm_fp8_qout_kernel(DtpGemmFp8Args a, DtpFp8QuantOut q) {
  constexpr bool SPLIT = false;
#include "gemm_fp8_body.h"
  (void)vec;
  const QuantOut qo{static_cast<uint8_t*>(q.q), static_cast<uint8_t*>(q.qT), q.ldq, q.ldqt, *q.scale, q.fmt};
  uint32_t amax = 0;
  quant_epilogue_pass<0>(e, qo, acc, ebuf, bias, m0 + wr * 64, ncol, lane, amax);
  quant_epilogue_pass<1>(e, qo, acc, ebuf, bias, m0 + 128 + wr * 64, ncol, lane, amax);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = max(amax, static_cast<uint32_t>(__shfl_xor(static_cast<int>(amax), o, kWave)));
  // one word per (tile, wave): every launch writes all of them and the count, nothing to clear, no atomics
  if (lane == 0) q.part[1 + blockIdx.x * 8 + wave] = amax;
  if (tid == 0 && blockIdx.x == 0) q.part[0] = gridDim.x * 8;
}

// Short-K instance (K <= kShortK).  The FP8 matrix unit does not sum one instruction's products
// in fp32: it aligns them to the largest and keeps about 15 bits below it, an error of up to
// ~2^-15 of that product per instruction whatever K is.  A long sum buries that under its own
// fp32 accumulation error (K 2^-23 of the magnitude sum); a short one does not (K = 16: measured
// 1.4e-4 of the magnitude sum where fp32 accumulation allows 2e-6), and below K = 2^8 the 2^-15
// can exceed K 2^-23 on benign data.  Such problems are bandwidth- and launch-bound anyway, so they
// decode the FP8 bytes to f32 (exact) and run on the exact-fp32 v_mfma_f32_16x16x4_f32:
//  * 64 x 64 tile, 4 waves, wave w rows 16 w .. +16 and all four 16-column fragments; no LDS:
//    K is at most four 64-byte blocks, every operand byte is read once per wave from L2.
//  * per 64-byte K block, lane (lr, lg) loads the 16 bytes [16 lg, +16) of its A row and of each
//    B row (clamped rows, zero bytes past K), converts them with v_cvt_pk_f32_fp8 / bf8, and
//    MFMA t of 16 takes byte t of every lane group: the same k in A and B, which is all the sum
//    needs.  The epilogue is the per-element one of gemm_epi.h.
constexpr int kShortK = 256;

template <int FMT>
DTP_DEV void decode16(const uint4& g, float (&f)[16]) {
  const int w[4] = {(int)g.x, (int)g.y, (int)g.z, (int)g.w};
  typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x2 lo, hi;
    if constexpr (FMT == DTP_FP8_E4M3) {
      lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[q], false);
      hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[q], true);
    } else {
      lo = __builtin_amdgcn_cvt_pk_f32_bf8(w[q], false);
      hi = __builtin_amdgcn_cvt_pk_f32_bf8(w[q], true);
    }
    f[4 * q] = lo[0];
    f[4 * q + 1] = lo[1];
    f[4 * q + 2] = hi[0];
    f[4 * q + 3] = hi[1];
  }
}

template <int FA>
__global__ __launch_bounds__(256) void gemm_fp8_short_kernel(DtpGemmFp8Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.y * 64 + 16 * wave, n0 = blockIdx.x * 64;
  if (m0 >= a.M) return;  // (no barriers in this kernel)
  DtpGemmArgs e{};
  e.ldc = a.ldc;
  e.ldaux = a.ldaux;
  e.M = a.M;
  e.N = a.N;
  e.out_dtype = a.out_dtype;
  e.act = a.act;
  e.accumulate = a.accumulate;
  e.splitk = 1;
  e.slope = a.slope;
  e.alpha = *a.sa_inv * *a.sb_inv;
  const char* arow = static_cast<const char*>(a.A) + static_cast<long long>(min(m0 + lr, a.M - 1)) * a.lda;
  const char* brow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    brow[j] = static_cast<const char*>(a.B) + static_cast<long long>(min(n0 + 16 * j + lr, a.N - 1)) * a.ldb;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < a.K; kb += 64) {  // uniform trip count: MFMAs are wave-wide
    const int k = kb + 16 * lg;
    const bool live = k < a.K;
    float fa[16], fb[16];
    decode16<FA>(live ? *reinterpret_cast<const uint4*>(arow + k) : make_uint4(0, 0, 0, 0), fa);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      decode16<DTP_FP8_E4M3>(live ? *reinterpret_cast<const uint4*>(brow[j] + k) : make_uint4(0, 0, 0, 0), fb);
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t], fb[t], acc[j], 0, 0, 0);
    }
  }
  // fragment layout: acc[j][r] is row 4 lg + r, column 16 j + lr
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + 16 * j + lr;
    if (n >= a.N) continue;
    const float bias = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 4 * lg + r;
      if (m < a.M)
        epilogue_store<DTP_DT_BF16>(e, static_cast<char*>(a.C), static_cast<const char*>(a.aux), m, n, acc[j][r], bias);
    }
  }
}

}  // namespace f8
}  // namespace gemm
}  // namespace dtp

// the call goes to the pipelined kernel's f8f6f4 instance: the one with a split twin
static bool fp8_splittable(const DtpGemmFp8Args& a) { return a.K > dtp::gemm::f8::kShortK && a.mfma != 1; }

extern "C" long long dtp_gemm_fp8_workspace(const DtpGemmFp8Args* in) {
  if (!in || in->splitk != 0 || in->M <= 0 || in->N <= 0 || in->K <= 0) return 0;
  const int sp = dtp::gemm::f8_split_plan(in->M, in->N, in->K, in->out_dtype, in->act, in->aux, fp8_splittable(*in));
  return sp > 1 ? 4LL * sp * in->M * in->N : 0;
}

extern "C" int dtp_gemm_fp8(const DtpGemmFp8Args* in, void* stream) { return dtp_gemm_fp8_quant(in, nullptr, stream); }

extern "C" int dtp_gemm_fp8_quant(const DtpGemmFp8Args* in, const DtpFp8QuantOut* qin, void* stream) {
  using namespace dtp;
  if (!in) return set_err(1, "dtp_gemm_fp8: null args");
  DtpGemmFp8Args a = *in;
  const DtpFp8QuantOut q = qin ? *qin : DtpFp8QuantOut{};
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return set_err(1, "dtp_gemm_fp8: empty problem");
  if (!a.A || !a.B || !a.C || !a.sa_inv || !a.sb_inv) return set_err(1, "dtp_gemm_fp8: null operand or scale");
  if (a.fmt_b != DTP_FP8_E4M3 || (a.fmt_a != DTP_FP8_E4M3 && a.fmt_a != DTP_FP8_E5M2))
    return set_err(1, "dtp_gemm_fp8: operand formats must be e4m3 x e4m3 or e5m2 x e4m3");
  if (a.out_dtype != DTP_DT_F32 && a.out_dtype != DTP_DT_BF16) return set_err(1, "dtp_gemm_fp8: bad out dtype");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (a.K % 16 || a.lda % 16 || a.ldb % 16 || a.lda < a.K || a.ldb < a.K || !al16(a.A) || !al16(a.B))
    return set_err(1, "dtp_gemm_fp8: K and both leading dimensions must be multiples of 16, operands 16-byte aligned");
  if (a.ldc < a.N || (a.aux && a.ldaux < a.N)) return set_err(1, "dtp_gemm_fp8: C / aux rows shorter than N");
  const long long two_gib = 1LL << 31;
  if (a.M * a.lda >= two_gib || a.N * a.ldb >= two_gib) return set_err(1, "dtp_gemm_fp8: operands must be under 2 GiB");
  // quantised output: the qout instances where the vector epilogue applies to every lane; otherwise the plain
  // GEMM and then the given-scale quantiser on C, which writes the same bits
  bool fused_q = false;
  if (qin) {
    if (!q.q || !q.scale || !q.part) return set_err(1, "dtp_gemm_fp8: a quantised output needs its scale and partials");
    if (a.out_dtype != DTP_DT_BF16 || a.accumulate || (a.splitk != 0 && a.splitk != 1))
      return set_err(1, "dtp_gemm_fp8: a quantised output needs a bf16 C without accumulate or split-K");
    if (q.fmt != DTP_FP8_E4M3 && q.fmt != DTP_FP8_E5M2) return set_err(1, "dtp_gemm_fp8: bad format of the quantised output");
    if (a.N % 16 || q.ldq % 16 || q.ldq < a.N || !al16(q.q) ||
        (q.qT && (q.ldqt % 16 || q.ldqt < (a.M + 15) / 16 * 16 || !al16(q.qT))))
      return set_err(1, "dtp_gemm_fp8: a quantised output needs N % 16 == 0 and 16-byte aligned rows (qT: M rounded up to 16)");
    fused_q = a.K > gemm::f8::kShortK && a.ldc % 8 == 0 && al16(a.C) && (!a.aux || (a.ldaux % 8 == 0 && al16(a.aux)));
    const long long need = fused_q ? 8LL * ((a.M + 255) / 256) * ((a.N + 255) / 256) : (long long)((a.M + 63) / 64) * ((a.N + 63) / 64);
    if (need > q.cap) return set_err(1, "dtp_gemm_fp8: the partials buffer of the quantised output is too small");
  }
  auto quantise_c = [&]() {  // the unfused form of the quantised output
    return dtp_fp8_quantize_scaled(a.C, a.ldc, a.M, a.N, DTP_DT_BF16, q.fmt, q.q, q.ldq, q.qT, q.ldqt, q.scale, q.part, q.cap,
                                   stream);
  };
  if (a.splitk == 0) {  // the plan, if the caller brought its workspace
    const int sp = gemm::f8_split_plan(a.M, a.N, a.K, a.out_dtype, a.act, a.aux, fp8_splittable(a));
    a.splitk = (sp > 1 && a.M <= 65535 && a.work && a.work_bytes >= 4LL * sp * a.M * a.N) ? sp : 1;
  }
  if (const char* why = gemm::f8_split_refusal(a.M, a.N, a.K, a.out_dtype, a.act, a.aux, fp8_splittable(a), a.splitk,
                                               a.work, a.work_bytes))
    return set_err(-1, (std::string("dtp_gemm_fp8: ") + why).c_str());
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.K <= gemm::f8::kShortK) {  // short sums: the exact-fp32 instance (see gemm_fp8_short_kernel)
    const dim3 gs((a.N + 63) / 64, (a.M + 63) / 64), bs(256);
    if (gs.y > 65535) return set_err(1, "dtp_gemm_fp8: M too large for the short-K instance");
    if (a.fmt_a == DTP_FP8_E4M3) hipLaunchKernelGGL(gemm::f8::gemm_fp8_short_kernel<DTP_FP8_E4M3>, gs, bs, 0, s, a);
    else hipLaunchKernelGGL(gemm::f8::gemm_fp8_short_kernel<DTP_FP8_E5M2>, gs, bs, 0, s, a);
    if (int err = check_launch("dtp_gemm_fp8(short K)")) return err;
    return qin ? quantise_c() : 0;
  }
  const long long tiles = (long long)((a.M + 255) / 256) * ((a.N + 255) / 256);
  const dim3 b(gemm::f8::kThreads);
  if (a.splitk > 1) {  // tiles x S workgroups of partial sums, then the reduction with the epilogue
    const dim3 g((unsigned)(tiles * a.splitk));
    if (a.fmt_a == DTP_FP8_E4M3) hipLaunchKernelGGL((gemm::f8::gemm_fp8_kernel<DTP_FP8_E4M3, false, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((gemm::f8::gemm_fp8_kernel<DTP_FP8_E5M2, false, true>), g, b, 0, s, a);
    if (int err = check_launch("dtp_gemm_fp8(256x256x128, split-K)")) return err;
    const gemm::F8ReduceArgs r{static_cast<const float*>(a.work), static_cast<float*>(a.C), a.bias, a.sa_inv, a.sb_inv,
                               a.ldc, a.M, a.N, a.splitk, a.accumulate};
    hipLaunchKernelGGL(gemm::f8_splitk_reduce_kernel<true>, dim3((a.N + 1023) / 1024, a.M), dim3(256), 0, s, r);
    return check_launch("dtp_gemm_fp8(split-K reduction)");
  }
  const dim3 g((unsigned)tiles);
  if (fused_q) {
    switch ((a.fmt_a == DTP_FP8_E5M2 ? 2 : 0) | (a.mfma == 1 ? 1 : 0)) {
      case 0: hipLaunchKernelGGL((gemm::f8::gemm_fp8_qout_kernel<DTP_FP8_E4M3, false>), g, b, 0, s, a, q); break;
      case 1: hipLaunchKernelGGL((gemm::f8::gemm_fp8_qout_kernel<DTP_FP8_E4M3, true>), g, b, 0, s, a, q); break;
      case 2: hipLaunchKernelGGL((gemm::f8::gemm_fp8_qout_kernel<DTP_FP8_E5M2, false>), g, b, 0, s, a, q); break;
      default: hipLaunchKernelGGL((gemm::f8::gemm_fp8_qout_kernel<DTP_FP8_E5M2, true>), g, b, 0, s, a, q); break;
    }
    return check_launch("dtp_gemm_fp8(256x256x128, quantised output)");
  }
  switch ((a.fmt_a == DTP_FP8_E5M2 ? 2 : 0) | (a.mfma == 1 ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((gemm::f8::gemm_fp8_kernel<DTP_FP8_E4M3, false, false>), g, b, 0, s, a); break;
    case 1: hipLaunchKernelGGL((gemm::f8::gemm_fp8_kernel<DTP_FP8_E4M3, true, false>), g, b, 0, s, a); break;
    case 2: hipLaunchKernelGGL((gemm::f8::gemm_fp8_kernel<DTP_FP8_E5M2, false, false>), g, b, 0, s, a); break;
    default: hipLaunchKernelGGL((gemm::f8::gemm_fp8_kernel<DTP_FP8_E5M2, true, false>), g, b, 0, s, a); break;
  }
  if (int err = check_launch("dtp_gemm_fp8(256x256x128)")) return err;
  return qin ? quantise_c() : 0;
}

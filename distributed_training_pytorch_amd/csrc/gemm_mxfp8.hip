// MXFP8 GEMM for gfx950 (CDNA4): OCP e4m3 / e5m2 operands with one E8M0 scale byte per 32
// elements along K (mxfp8_quant.hip), fp32 accumulation and the fused Linear epilogues of gemm_epi.h:
//   C[M,N] (+)= epi(sum_k A(m,k) 2^(sa(m,k/32)-127) . B(n,k) 2^(sb(n,k/32)-127))
// A [M,K] and B [N,K] both K-contiguous, sa [M][ldsa] and sb [N][ldsb] bytes, K % 32 == 0.
//
// Pipelined instance (K > kShortK): the 256 x 256 x 128-byte eight-phase LDS-DMA geometry of
// gemm_fp8.hip (8 waves as 2 x 4, four quadrants, one operand part staged per phase, waves 4-7
// one barrier behind), with v_mfma_scale_f32_16x16x128_f8f6f4 fed real block scales.  What differs:
//  * fragment layout.  Measured on the instruction (one-hot blocks of ones against scale bytes
//    127 + j, profiles/mxfp8/README.md): the 8 operand VGPRs of lane (lr = lane & 15,
//    lg = lane >> 4) are K-bytes 16 lg .. +16 (VGPRs 0-3) and 64 + 16 lg .. +16 (VGPRs 4-7) of
//    row lr, and the scale byte of lane (lr, b) applies to K-bytes 32 b .. +32 of row lr: the
//    scale lanes follow the MX blocks, the data lanes do not.  A lane's 32 bytes are therefore
//    NOT one block (its halves belong to blocks lg >> 1 and 2 + (lg >> 1)), and a layout that
//    gives lane group lg the chunks 2 lg, 2 lg + 1 puts half of every block under a
//    neighbour's scale (measured: 16 s0 + 16 s2 where 32 s0 was due).  With real scales the
//    k order inside the instruction is no longer free: chunks lg and 4 + lg it must be.
//  * swizzle.  That is the pairing gemm_fp8.hip's fswz(r) = (r & 3) | ((r >> 1) & 4) was chosen
//    for: chunk c of row r at c ^ fswz(r), applied on the DMA source address.  Bank argument:
//    a ds_read_b128 is served in four 16-lane groups, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
//    and the same + 32; a 256-byte bank row is 16 slots of 16 B, two image rows, slot
//    8 bit0(lr) + (c ^ fswz(lr)).  A group holds every lr once: rows {0-3, 12-15} with chunk c
//    from one lane group and rows {4-11} with chunk c ^ 1 from its neighbour; fswz of the even
//    rows 0, 2, 12, 14 is 0, 2, 4, 6 and of 4, 6, 8, 10 xor 1 is 1, 3, 5, 7: eight slots, the
//    odd rows take the other eight, and the second read (4 + lg) only xors 4 in.
//  * scales.  Each K-tile adds 4 bytes per operand row, 512 B per part, 1/32 of the operand
//    bytes.  They travel as one more LDS-DMA instruction per part (global_load_lds_dword: lane
//    l of wave w fetches the aligned dword sa[row 64 (w & 1) + l][4 tile .. +4), so waves
//    0 / 1 fill the part's [128 rows][4 B] scale image and the other six write the same bytes
//    again: every wave issues the same number of loads), into scale buffers that rotate with
//    the operand buffers (two K-tiles + a sink, 4.5 KiB after the operand LDS).  Lane (lr, lg)
//    then reads byte lg of row lr's dword with the fragment itself (ds_read_u8: the four lane
//    groups hit one bank per row, 16 rows 16 banks, the rest is broadcast) into bits 0-7 of a
//    VGPR, which op_sel 0 names.  Scale VGPRs live exactly as long as their fragments: 8.
//    (Plain global loads one K-tile ahead need 24 VGPRs in ping-pong on top of the 229 of this
//    geometry: they spilled, and every scratch reload drains vmcnt.)
//  * wait counts.  Loads retire in order and every part is now 3 DMA instructions (2 data +
//    1 scale), issued together, so a part's scales land with its bytes.  Keeping the three
//    youngest parts in flight across a barrier is s_waitcnt vmcnt(9) (gemm_fp8.hip: 6), in the
//    prologue (5 parts issued, B0 and A0 of tile 0 retired) as in every phase.  The scale
//    bytes are read under the same barrier / lgkmcnt(0) discipline as the fragments, so the
//    buffer-reuse (WAR) argument of the operand parts covers them unchanged.
//  * split-K (SPLIT instances, splitk > 1): as gemm_fp8.hip -- grid tiles x S, each block one K-slice
//    of whole K-tiles, raw fp32 partial sums to a workspace, f8_splitk_reduce_kernel for the
//    epilogue.  A slice's scale DMA starts 4 bytes per K-tile of its offset into the same rows.
//    Splitting changes neither the set of matrix instructions nor their products, only which
//    workgroup issues them: the short-K rule stays a function of the whole K.
//  * K % 128 != 0: the dead chunks of the last K-tile come from a zero block, as in gemm_fp8.hip;
//    their scale bytes are the 127s the quantiser wrote.  Rows past M / N are clamped on load
//    (data and scales), guarded on store.
//
// Short-K instance (K <= kShortK = 2048): the matrix unit keeps about 15 bits below the largest
// product of one instruction, scales included, so one loud block costs its quiet neighbours
// their low bits; a short sum cannot hide that under K 2^-23 of the magnitude sum.  gemm_fp8_short_kernel's plan (64 x 64 tile, 4 waves, no LDS, FP8 bytes decoded
// to f32 for the exact-fp32 v_mfma_f32_16x16x4_f32) with each decoded value multiplied by a power
// of two from its block's scale (scale_shift() below), which is exact: the 16 bytes [64 kb + 16 lg, +16)
// a lane loads are half of MX block 2 kb + (lg >> 1).
#include <string>

#include "gemm_epi.h"

namespace dtp {
namespace gemm {
namespace mx {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void gbl_void_t;
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 512;
constexpr int kPart = 128 * 128;     // one operand part of one K-tile (16 KiB)
constexpr int kBuf = 4 * kPart;      // parts A0, A1, B0, B1
constexpr int kSink = 2 * kBuf;      // DMA sink for the slots past the last K-tile
constexpr int kScale = kSink + kPart;  // scale images: [2 K-tiles][4 parts][128 rows][4 B], then a 512-B sink
constexpr int kSPart = 128 * 4;
constexpr int kLds = kScale + 9 * kSPart;  // 148.5 KiB
static_assert(8 * kEpiWaveFloats * 4 <= kLds, "epilogue staging must fit the operand LDS");
// per-tensor FP8 switches at 256.  Here one loud element (500 next to values of a few units, which
// the format clamps to 448 and keeps) dominates its instruction and costs the other 127 products
// their low bits: measured up to 1.7e-4 of the magnitude sum whatever K is, against a bound of
// (K + 1) 2^-23 = 6.5e-5 at K = 544 and 2.4e-4 at 2048; blocks spread over 2^-6 .. 2^6 alone
// measure 3-5e-5 up to K = 512 (profiles/mxfp8/accuracy_probe.txt).  The bound stays, the
// threshold moves.
constexpr int kShortK = 2048;

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
// drains vmcnt(0) before it.  The reads complete under mid()'s lgkmcnt(0).
DTP_DEV i32x8 frag(const char* part, const int (&off)[2], int f) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  i32x4 lo, hi;
  const uint32_t p0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_void_t*)(part + off[0] + f * 2048)));
  const uint32_t p1 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_void_t*)(part + off[1] + f * 2048)));
  asm volatile("ds_read_b128 %0, %1" : "=v"(lo) : "v"(p0));
  asm volatile("ds_read_b128 %0, %1" : "=v"(hi) : "v"(p1));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// byte `off` of a part's scale image (see frag() for why this is inline asm)
DTP_DEV int scale_byte(const char* img, int off) {
  int r;
  const uint32_t p = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_void_t*)(img + off)));
  asm volatile("ds_read_u8 %0, %1" : "=v"(r) : "v"(p));
  return r;
}

DTP_DEV void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

DTP_DEV DtpGemmArgs epi_args(const DtpGemmMxArgs& a) {
  DtpGemmArgs e{};  // the epilogue's view of the problem (gemm_epi.h)
  e.C = a.C;
  e.bias = a.bias;
  e.aux = a.aux;
  e.ldc = a.ldc;
  e.ldaux = a.ldaux;
  e.M = a.M;
  e.N = a.N;
  e.K = a.K;
  e.dtype = DTP_DT_BF16;
  e.out_dtype = a.out_dtype;
  e.act = a.act;
  e.accumulate = a.accumulate;
  e.splitk = 1;
  e.slope = a.slope;
  e.alpha = 1.f;
  return e;
}

// FA: format of A (DTP_FP8_*); B is e4m3.  SPLIT: grid = tiles x a.splitk, the block runs K-slice
// id.ks (f8_slice) and stores raw fp32 partial sums to a.work[ks][M][N]
template <int FA, bool SPLIT>
__global__ __launch_bounds__(kThreads) void gemm_mxfp8_kernel(DtpGemmMxArgs a) {
  __shared__ __align__(16) char lds[kLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 2, wc = wave & 3;
  DtpGemmArgs e{};
  if constexpr (SPLIT) {  // raw partial sums: no bias, aux, act or accumulate, alpha = 1
    e.M = a.M;
    e.N = a.N;
    e.K = a.K;
    e.dtype = DTP_DT_BF16;
    e.ldc = a.N;
    e.out_dtype = DTP_DT_F32;
    e.splitk = a.splitk;  // (for decode_tile; 1 again before the stores)
    e.alpha = 1.f;
  } else {
    e = epi_args(a);
  }

  const TileId id = decode_tile<256, 256>(e);
  const int m0 = id.m0, n0 = id.n0;
  const int ktail = a.K & 127;  // valid bytes of the last K-tile (0: all 128)
  // this block's K-tiles: nk of them from tile kt0 on; the global last K-tile, the only ragged one,
  // is its tile ktl (>= nk: in another slice)
  int nk = (a.K + 127) >> 7, kt0 = 0;
  int ktl = nk - 1;
  if constexpr (SPLIT) {
    const F8Slice sl = f8_slice(nk, a.splitk, id.ks);
    nk = sl.nkt;
    kt0 = sl.t0;
    ktl -= sl.t0;
    e.C = static_cast<float*>(a.work) + static_cast<long long>(id.ks) * a.M * a.N;
    e.splitk = 1;
  }

  uint32_t oSA[2][2], oSB[2][2];
  part_sources(oSA, a.lda, m0, a.M, wave, lane);
  part_sources(oSB, a.ldb, n0, a.N, wave, lane);
  const char* gA = static_cast<const char*>(a.A) + m0 * a.lda + static_cast<uint32_t>(kt0) * 128u;
  const char* gB = static_cast<const char*>(a.B) + n0 * a.ldb + static_cast<uint32_t>(kt0) * 128u;
  // the source chunk of this lane in every DMA instruction (fswz reads row bits 0, 1, 3 =
  // lane bits 3, 4 and wave bit 0: the same for both instructions and both parts)
  const int csrc = (lane & 7) ^ fswz((wave * 8 + (lane >> 3)) & 15);
  const bool dead = ktail && csrc * 16 >= ktail;
  // scale rows of this lane in the scale DMA of parts A0, A1, B0, B1 (clamped as the operand rows),
  // at the dword of the block's first K-tile
  uint32_t oSS[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = 128 * i + (wave & 1) * 64 + lane;
    oSS[i] = static_cast<uint32_t>(min(m0 + r, a.M - 1)) * static_cast<uint32_t>(a.ldsa) + kt0 * 4u;
    oSS[2 + i] = static_cast<uint32_t>(min(n0 + r, a.N - 1)) * static_cast<uint32_t>(a.ldsb) + kt0 * 4u;
  }
  const char* zero = reinterpret_cast<const char*>(&g_zero_chunk);

  // one part (P: 0 = A0, 1 = A1, 2 = B0, 3 = B1) of K-tile `tile` (counted from the block's
  // first) into its buffer, or into the sink past the last tile (same wait accounting every phase)
  auto stage = [&](auto P, int tile) {
    constexpr int p = decltype(P)::value;
    const bool real = tile < nk;
    char* dst = lds + (real ? (tile & 1) * kBuf + p * kPart : kSink) + wave * 1024;
    // 32-bit tile offset (dtp_gemm_mxfp8 requires each operand < 2 GiB)
    const char* g = (p < 2 ? gA : gB) + static_cast<uint32_t>(real ? tile : 0) * 128u;
    const uint32_t* o = p < 2 ? oSA[p & 1] : oSB[p & 1];
    // the ragged K-tile (a sink slot re-reads tile 0): chunks past K come from the zero block
    // (the unsplit instances keep their own form of the same test: ktl = nk - 1 there)
    const bool cut = dead && (SPLIT ? (real ? tile : 0) == ktl : (real ? tile == nk - 1 : nk == 1));
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(cut ? zero : g + o[i]), (lds_void_t*)(dst + i * 8192), 16, 0, 0);
    // the part's scales: this lane's row, the K-tile's aligned dword (a sink slot re-reads tile 0)
    char* sdst = lds + kScale + (real ? ((tile & 1) * 4 + p) * kSPart : 8 * kSPart) + (wave & 1) * 256;
    const unsigned char* sg = (p < 2 ? a.sa : a.sb) + (p < 2 ? oSS[p & 1] : oSS[2 + (p & 1)]) + (real ? tile : 0) * 4u;
    __builtin_amdgcn_global_load_lds((gbl_void_t*)sg, (lds_void_t*)sdst, 4, 0, 0);
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  using P3 = std::integral_constant<int, 3>;

  // byte offsets of this lane's two fragment chunks (lg and 4 + lg: the instruction's own k
  // order) inside a part; fragment f (16 rows) adds 2048 f
  const int lr = lane & 15, lg = lane >> 4;
  int oA[2], oB[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    oA[h] = ((wr * 64 + lr) * 8 + ((4 * h + lg) ^ fswz(lr))) * 16;
    oB[h] = ((wc * 32 + lr) * 8 + ((4 * h + lg) ^ fswz(lr))) * 16;
  }

  // this lane's byte in a part's scale image: row (4 B), block lg; fragment f adds 64 f
  const int oSa = (wr * 64 + lr) * 4 + lg, oSb = (wc * 32 + lr) * 4 + lg;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  i32x8 fa[4], fb0[2], fb1[2];
  int sa[4], sb0[2], sb1[2];
  // part p of buffer `buf` (0 / 1): its fragments and their scale bytes
  auto rdA = [&](int buf, int p) {
    const char* img = lds + kScale + (buf * 4 + p) * kSPart;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      fa[f] = frag(lds + buf * kBuf + p * kPart, oA, f);
      sa[f] = scale_byte(img, oSa + 64 * f);
    }
  };
  auto rdB = [&](int buf, int p, i32x8 (&fb)[2], int (&sb)[2]) {
    const char* img = lds + kScale + (buf * 4 + p) * kSPart;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      fb[g] = frag(lds + buf * kBuf + p * kPart, oB, g);
      sb[g] = scale_byte(img, oSb + 64 * g);
    }
  };
  // end of a phase's load segment: retire the part the next phase reads (all but the three
  // youngest parts, 3 DMA instructions each), meet the partner group, then the quadrant's
  // MFMAs at raised priority
  auto mid = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
  };
  auto end = [&]() {
    __builtin_amdgcn_s_setprio(0);
    barrier();
  };
  auto mma = [&](auto QM, auto QN, const i32x8 (&fb)[2], const int (&sb)[2]) {
    constexpr int qm = decltype(QM)::value, qn = decltype(QN)::value;
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int g = 0; g < 2; ++g)
        acc[4 * qm + f][2 * qn + g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            fa[f], fb[g], acc[4 * qm + f][2 * qn + g], FA == DTP_FP8_E5M2 ? 1 : 0, 0, 0, sa[f], 0, sb[g]);
  };
  using Q0 = std::integral_constant<int, 0>;
  using Q1 = std::integral_constant<int, 1>;

  // prologue: B0, A0, B1, A1 of tile 0 and B0 of tile 1 (the order the loop's phases
  // -5 .. -1 would have staged them); vmcnt(9) retires B0 and A0 of tile 0
  stage(P2{}, 0);
  stage(P0{}, 0);
  stage(P3{}, 0);
  stage(P1{}, 0);
  stage(P2{}, 1);
  asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
  barrier();
  if (wave >= 4) barrier();  // stagger: waves 4-7 one barrier behind

  for (int u = 0; u < nk; ++u) {
    const int buf = u & 1;
    // phase 0: quadrant (0,0)
    rdB(buf, 2, fb0, sb0);
    rdA(buf, 0);
    stage(P0{}, u + 1);
    mid();
    mma(Q0{}, Q0{}, fb0, sb0);
    end();
    // phase 1: quadrant (0,1)
    rdB(buf, 3, fb1, sb1);
    stage(P3{}, u + 1);
    mid();
    mma(Q0{}, Q1{}, fb1, sb1);
    end();
    // phase 2: quadrant (1,1)
    rdA(buf, 1);
    stage(P1{}, u + 1);
    mid();
    mma(Q1{}, Q1{}, fb1, sb1);
    end();
    // phase 3: quadrant (1,0), fragments already in registers
    stage(P2{}, u + 2);
    mid();
    mma(Q1{}, Q0{}, fb0, sb0);
    end();
  }
  if (wave < 4) barrier();  // end of the stagger: equal barrier counts
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  barrier();

  // epilogue: LDS-staged 16-byte rows, one pass per row quadrant; the lane's 8 staged
  // columns 8 (lane & 7) .. +8 sit in column quadrant (lane & 7) >> 2
  float* ebuf = reinterpret_cast<float*>(lds) + wave * kEpiWaveFloats;
  const int c8 = lane & 7;
  const int ncol = n0 + (c8 >> 2) * 128 + wc * 32 + 8 * (c8 & 3);
  const uintptr_t cp = reinterpret_cast<uintptr_t>(e.C), ap = reinterpret_cast<uintptr_t>(e.aux);
  const bool vec = ncol + 8 <= e.N && e.ldc % 8 == 0 && (cp & 15) == 0 && (!e.aux || (e.ldaux % 8 == 0 && (ap & 15) == 0));
  float bias[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) bias[c] = (e.bias && ncol + c < e.N) ? e.bias[ncol + c] : 0.f;
  fast_epilogue_pass<0>(e, acc, ebuf, bias, m0 + wr * 64, ncol, vec, lane);
  fast_epilogue_pass<1>(e, acc, ebuf, bias, m0 + 128 + wr * 64, ncol, vec, lane);
}

// 16 FP8 bytes to f32, each times `mul` (a power of two: exact)
template <int FMT>
DTP_DEV void decode16(const uint4& g, float mul, float (&f)[16]) {
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
    f[4 * q] = lo[0] * mul;
    f[4 * q + 1] = lo[1] * mul;
    f[4 * q + 2] = hi[0] * mul;
    f[4 * q + 3] = hi[1] * mul;
  }
}

// 2^e by v_ldexp_f32: e = -127 (byte 0) gives the subnormal 2^-127, which the fp32 MFMA keeps.
DTP_DEV float pow2(int e) { return ldexpf(1.f, min(e, 127)); }

// How the two scales of one MX block reach the fp32 MFMA.  Each operand is multiplied by its own
// 2^(s - 127): exact for every byte the quantiser writes (0 .. 246; 0 .. 239 for e5m2), whatever the
// other rows of the fragment carry, since s = 0 times the smallest FP8 subnormal is still an fp32
// subnormal and the largest byte times fmax is still finite.  Only bytes past that range (up to 254,
// which the format allows and the block-scaled MFMA of the pipelined instance takes) would overflow
// on their own although the product with a small scale on the other side is an ordinary number.  For
// those, and only for those, a power of two t moves from one operand to the other: with samax the
// largest A byte of the wave's 16 rows and sbmax the largest B byte of the tile's 64 rows in this
// block, t = max(samax - top(A), 0) - max(sbmax - 246, 0), A times 2^(sa - 127 - t), B times
// 2^(sb - 127 + t).  t is the same for every lane that feeds one k, so each product is unchanged;
// it is 0 for every quantised tensor, and then this is the plain per-operand scaling.  (Both sides
// past their range at once: t = 0, the product is past fp32 anyway.)
template <int FA>
DTP_DEV int scale_shift(int sa, const int (&sb)[4]) {
  constexpr int top_a = FA == DTP_FP8_E5M2 ? 239 : 246;  // largest byte with 2^(s - 127) fmax finite
  int samax = sa, sbmax = max(max(sb[0], sb[1]), max(sb[2], sb[3]));
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {  // over lr: the 16 lanes of one lane group share the block
    samax = max(samax, __shfl_xor(samax, o, kWave));
    sbmax = max(sbmax, __shfl_xor(sbmax, o, kWave));
  }
  const int ta = max(samax - top_a, 0), tb = max(sbmax - 246, 0);
  return ta && tb ? 0 : ta - tb;
}

template <int FA>
__global__ __launch_bounds__(256) void gemm_mxfp8_short_kernel(DtpGemmMxArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.y * 64 + 16 * wave, n0 = blockIdx.x * 64;
  if (m0 >= a.M) return;  // (no barriers in this kernel)
  const DtpGemmArgs e = epi_args(a);
  const long long ra = min(m0 + lr, a.M - 1);
  const char* arow = static_cast<const char*>(a.A) + ra * a.lda;
  const uint8_t* sarow = a.sa + ra * a.ldsa;
  const char* brow[4];
  const uint8_t* sbrow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long rb = min(n0 + 16 * j + lr, a.N - 1);
    brow[j] = static_cast<const char*>(a.B) + rb * a.ldb;
    sbrow[j] = a.sb + rb * a.ldsb;
  }
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < a.K; kb += 64) {  // uniform trip count: MFMAs are wave-wide
    const int k = kb + 16 * lg;
    const bool live = k < a.K;
    const int blk = live ? k >> 5 : 0;  // the MX block these 16 bytes are half of
    const int sa = sarow[blk];
    int sb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sb[j] = sbrow[j][blk];
    const int sh = scale_shift<FA>(sa, sb);  // (outside any divergence: every lane takes part)
    float fa[16], fb[16];
    decode16<FA>(live ? *reinterpret_cast<const uint4*>(arow + k) : make_uint4(0, 0, 0, 0), pow2(sa - 127 - sh), fa);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      decode16<DTP_FP8_E4M3>(live ? *reinterpret_cast<const uint4*>(brow[j] + k) : make_uint4(0, 0, 0, 0),
                             pow2(sb[j] - 127 + sh), fb);
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

}  // namespace mx
}  // namespace gemm
}  // namespace dtp

// the call goes to the pipelined instance: the one with a split twin
static bool mx_pipelined(const DtpGemmMxArgs& a) {
  return !(a.instance == 2 || (a.instance != 1 && a.K <= dtp::gemm::mx::kShortK));
}

extern "C" long long dtp_gemm_mxfp8_workspace(const DtpGemmMxArgs* in) {
  if (!in || in->splitk != 0 || in->M <= 0 || in->N <= 0 || in->K <= 0) return 0;
  const int sp = dtp::gemm::f8_split_plan(in->M, in->N, in->K, in->out_dtype, in->act, in->aux, mx_pipelined(*in));
  return sp > 1 ? 4LL * sp * in->M * in->N : 0;
}

extern "C" int dtp_gemm_mxfp8(const DtpGemmMxArgs* in, void* stream) {
  using namespace dtp;
  if (!in) return set_err(1, "dtp_gemm_mxfp8: null args");
  DtpGemmMxArgs a = *in;
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return set_err(1, "dtp_gemm_mxfp8: empty problem");
  if (!a.A || !a.B || !a.C || !a.sa || !a.sb) return set_err(1, "dtp_gemm_mxfp8: null operand or scale");
  if (a.fmt_b != DTP_FP8_E4M3 || (a.fmt_a != DTP_FP8_E4M3 && a.fmt_a != DTP_FP8_E5M2))
    return set_err(1, "dtp_gemm_mxfp8: operand formats must be e4m3 x e4m3 or e5m2 x e4m3");
  if (a.out_dtype != DTP_DT_F32 && a.out_dtype != DTP_DT_BF16) return set_err(1, "dtp_gemm_mxfp8: bad out dtype");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (a.K % 32 || a.lda % 16 || a.ldb % 16 || a.lda < a.K || a.ldb < a.K || !al16(a.A) || !al16(a.B))
    return set_err(1, "dtp_gemm_mxfp8: K must be a multiple of 32, both leading dimensions of 16, operands 16-byte aligned");
  const int sk = 4 * ((a.K + 127) / 128);
  auto al4 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; };
  if (a.ldsa < sk || a.ldsb < sk || a.ldsa % 4 || a.ldsb % 4 || !al4(a.sa) || !al4(a.sb))
    return set_err(1, "dtp_gemm_mxfp8: scale rows must be 4-byte aligned and hold 4 bytes per 128 of K");
  if (a.ldc < a.N || (a.aux && a.ldaux < a.N)) return set_err(1, "dtp_gemm_mxfp8: C / aux rows shorter than N");
  const long long two_gib = 1LL << 31;
  if (a.M * a.lda >= two_gib || a.N * a.ldb >= two_gib || a.M * a.ldsa >= two_gib || a.N * a.ldsb >= two_gib)
    return set_err(1, "dtp_gemm_mxfp8: operands must be under 2 GiB");
  const bool short_k = !mx_pipelined(a);
  if (a.splitk == 0) {  // the plan, if the caller brought its workspace
    const int sp = gemm::f8_split_plan(a.M, a.N, a.K, a.out_dtype, a.act, a.aux, !short_k);
    a.splitk = (sp > 1 && a.M <= 65535 && a.work && a.work_bytes >= 4LL * sp * a.M * a.N) ? sp : 1;
  }
  if (const char* why = gemm::f8_split_refusal(a.M, a.N, a.K, a.out_dtype, a.act, a.aux, !short_k, a.splitk, a.work,
                                               a.work_bytes))
    return set_err(-1, (std::string("dtp_gemm_mxfp8: ") + why).c_str());
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (short_k) {  // short sums: the exact-fp32 instance (see gemm_mxfp8_short_kernel)
    const dim3 gs((a.N + 63) / 64, (a.M + 63) / 64), bs(256);
    if (gs.y > 65535) return set_err(1, "dtp_gemm_mxfp8: M too large for the short-K instance");
    if (a.fmt_a == DTP_FP8_E4M3) hipLaunchKernelGGL(gemm::mx::gemm_mxfp8_short_kernel<DTP_FP8_E4M3>, gs, bs, 0, s, a);
    else hipLaunchKernelGGL(gemm::mx::gemm_mxfp8_short_kernel<DTP_FP8_E5M2>, gs, bs, 0, s, a);
    return check_launch("dtp_gemm_mxfp8(short K)");
  }
  const long long tiles = (long long)((a.M + 255) / 256) * ((a.N + 255) / 256);
  const dim3 b(gemm::mx::kThreads);
  if (a.splitk > 1) {  // tiles x S workgroups of partial sums, then the reduction with the epilogue
    const dim3 g((unsigned)(tiles * a.splitk));
    if (a.fmt_a == DTP_FP8_E4M3) hipLaunchKernelGGL((gemm::mx::gemm_mxfp8_kernel<DTP_FP8_E4M3, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((gemm::mx::gemm_mxfp8_kernel<DTP_FP8_E5M2, true>), g, b, 0, s, a);
    if (int err = check_launch("dtp_gemm_mxfp8(256x256x128, split-K)")) return err;
    const gemm::F8ReduceArgs r{static_cast<const float*>(a.work), static_cast<float*>(a.C), a.bias, nullptr, nullptr,
                               a.ldc, a.M, a.N, a.splitk, a.accumulate};
    hipLaunchKernelGGL(gemm::f8_splitk_reduce_kernel<false>, dim3((a.N + 1023) / 1024, a.M), dim3(256), 0, s, r);
    return check_launch("dtp_gemm_mxfp8(split-K reduction)");
  }
  const dim3 g((unsigned)tiles);
  if (a.fmt_a == DTP_FP8_E4M3) hipLaunchKernelGGL((gemm::mx::gemm_mxfp8_kernel<DTP_FP8_E4M3, false>), g, b, 0, s, a);
  else hipLaunchKernelGGL((gemm::mx::gemm_mxfp8_kernel<DTP_FP8_E5M2, false>), g, b, 0, s, a);
  return check_launch("dtp_gemm_mxfp8(256x256x128)");
}

// Quantising epilogue of the pipelined FP8 GEMM (gemm_fp8.hip, the QOUT instances): delayed scaling.
// The scale of the output tensor is known before the GEMM starts (it comes from the amaxes of
// earlier steps), so the pass that holds the finished tile writes, next to the bf16 C,
//   q [M][ldq]   = cvt_rne(clamp(C_bf16 * scale, -fmax, fmax))   the next GEMM's row-major operand
//   qT[N][ldqt]  the same bytes transposed                        its K-contiguous twin for dW / dx
//   one amax word per (tile, wave)                                the next step's scale
// and the activation is never read back to be quantised.  What is quantised is the bf16-rounded
// value, bit for bit what C holds: q == quantise(C, scale) exactly.
//
// One pass = one wave's 64 rows x 64 columns (fast_epilogue_pass's geometry, gemm_epi.h):
//  1. the f32 fragments are parked in the wave's LDS region (row stride 68 floats) and read back
//     row-major: lane (rl = lane >> 3, c8 = lane & 7) holds columns 8 c8 .. +8 of rows rl + 8 t.
//  2. per row: bias / LeakyReLU'(aux) / LeakyReLU, round to bf16, one 16-byte store to C; the
//     rounded values times the scale, clamped, through the packed convert: 8 bytes, one 8-byte
//     store to q.  The |c| bit patterns are folded into the lane's running maximum (rows < M only;
//     the host sends only N % 16 == 0 here, so a lane's 8 columns are all inside N or all outside).
//  3. the lane keeps its 8 rows x 8 bytes in 16 registers until every f32 read of the pass is done,
//     then the wave overwrites the head of its own region with the [64 rows][64 B] byte image,
//     row stride 68 B as fp8_quant.hip's tile (rows past M as zero bytes: they become the zero pad
//     of qT up to M rounded up to 16).
//  4. qT leaves as 16-byte stores of 16 rows of one column: store s of 4, lane L takes column
//     k = 16 s + (L >> 2) and row group mg = L & 3, so four neighbouring lanes write 64 contiguous
//     bytes of one qT row.  Its 16 bytes are gathered by byte reads at (16 mg + i) 68 + k: word
//     (16 mg + i) 17 + (k >> 2), i.e. bank 16 mg + 17 i + (L >> 4) + 4 s (mod 64): the four row
//     groups sit 16 banks apart and the four lanes of one (mg, k >> 2) read one word (a broadcast),
//     so one read instruction touches 16 distinct words in 16 distinct banks.  (The writes of step 3,
//     word (rl + 8 t) 17 + 2 c8 + j, are not conflict-free: rows rl and rl + 4 overlap in up to 6 banks.
//     16 four-byte writes per pass against 64 byte reads: left as it is.)
// The region is the wave's own and LDS is in order per wave: no workgroup barrier anywhere.
#pragma once

#include "gemm_epi.h"

namespace dtp {
namespace gemm {

struct QuantOut {
  uint8_t* q;
  uint8_t* qT;  // or null
  long long ldq, ldqt;
  float scale;
  int fmt;  // DTP_FP8_*
};

DTP_DEV uint32_t quant4(int fmt, float lim, float scale, float a, float b, float c, float d) {
  a = fminf(fmaxf(a * scale, -lim), lim);
  b = fminf(fmaxf(b * scale, -lim), lim);
  c = fminf(fmaxf(c * scale, -lim), lim);
  d = fminf(fmaxf(d * scale, -lim), lim);
  int w = 0;
  if (fmt == DTP_FP8_E4M3) {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
  }
  return static_cast<uint32_t>(w);
}

// H: the row half (fragment rows 4H .. 4H+3).  a: a bf16 C without accumulate, C / aux 16-byte aligned with
// row strides that are multiples of 8, N % 16 == 0 (the host checks).  amax: the lane's running maximum
// of |C_bf16| as f32 bit patterns.
template <int H>
DTP_DEV void quant_epilogue_pass(const DtpGemmArgs& a, const QuantOut& qo, const f32x4 (&acc)[8][4], float* buf,
                                 const float (&bias)[8], int row0, int ncol, int lane, uint32_t& amax) {
  const int lr = lane & 15, lg = lane >> 4, c8 = lane & 7, rl = lane >> 3;
  char* C = static_cast<char*>(a.C);
  const uint16_t* aux = static_cast<const uint16_t*>(a.aux);
  const bool live = ncol < a.N;  // all 8 columns, or none
  const float lim = qo.fmt == DTP_FP8_E4M3 ? 448.f : 57344.f;
#pragma unroll
  for (int ii = 0; ii < 4; ++ii)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) buf[(16 * ii + 4 * lg + r) * kEpiStride + 16 * j + lr] = acc[4 * H + ii][j][r];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's stores land before its own reads
  uint32_t img[8][2];  // the lane's FP8 bytes: row rl + 8 t, columns 8 c8 .. +8
#pragma unroll
  for (int t0 = 0; t0 < 8; t0 += 4) {
    float v[4][8];
    uint4 g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int lrow = rl + 8 * (t0 + u);
      const float4 x0 = *reinterpret_cast<const float4*>(buf + lrow * kEpiStride + 8 * c8);
      const float4 x1 = *reinterpret_cast<const float4*>(buf + lrow * kEpiStride + 8 * c8 + 4);
      const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
      for (int c = 0; c < 8; ++c) v[u][c] = xs[c];
      // (rows past M clamped, never stored; a dead lane reads column 0 of its row)
      if (aux) g[u] = *reinterpret_cast<const uint4*>(aux + min(row0 + lrow, a.M - 1) * a.ldaux + (live ? ncol : 0));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int mrow = row0 + rl + 8 * (t0 + u);
      float y[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) y[c] = a.alpha * v[u][c] + bias[c];
      if (aux) {
        float gv[8];
        bf16x8_to_f32(g[u], gv);
#pragma unroll
        for (int c = 0; c < 8; ++c) y[c] *= leaky_grad_from_out(gv[c], a.slope);
      }
      if (a.act) {
#pragma unroll
        for (int c = 0; c < 8; ++c) y[c] = leaky(y[c], a.slope);
      }
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = uint32_t(f32_to_bf16(y[2 * q])) | (uint32_t(f32_to_bf16(y[2 * q + 1])) << 16);
      const bool in = live && mrow < a.M;
      float cf[8];  // the stored values, back in f32
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        cf[2 * q] = __uint_as_float(o[q] << 16);
        cf[2 * q + 1] = __uint_as_float(o[q] & 0xffff0000u);
      }
      const uint32_t w0 = in ? quant4(qo.fmt, lim, qo.scale, cf[0], cf[1], cf[2], cf[3]) : 0u;
      const uint32_t w1 = in ? quant4(qo.fmt, lim, qo.scale, cf[4], cf[5], cf[6], cf[7]) : 0u;
      img[t0 + u][0] = w0;
      img[t0 + u][1] = w1;
      if (in) {
#pragma unroll
        for (int q = 0; q < 4; ++q) amax = max(amax, max((o[q] << 16) & 0x7fff0000u, o[q] & 0x7fff0000u));
        *reinterpret_cast<uint4*>(C + (static_cast<long long>(mrow) * a.ldc + ncol) * 2) = make_uint4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<uint2*>(qo.q + static_cast<long long>(mrow) * qo.ldq + ncol) = make_uint2(w0, w1);
      }
    }
  }
  if (qo.qT) {
    // the byte image over the head of the staging region, once every f32 read of the pass has returned
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      buf[(rl + 8 * t) * 17 + 2 * c8] = __uint_as_float(img[t][0]);
      buf[(rl + 8 * t) * 17 + 2 * c8 + 1] = __uint_as_float(img[t][1]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const uint8_t* image = reinterpret_cast<const uint8_t*>(buf);
    const int mg = lane & 3;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = 16 * s + (lane >> 2);  // staged column: column quadrant k >> 5, column k & 31 of the wave's 32
      const int n = ncol - 8 * (c8 & 3) - (c8 >> 2) * 128 + (k >> 5) * 128 + (k & 31);
      const int m = row0 + 16 * mg;
      const uint8_t* tb = image + (16 * mg) * 68 + k;
      uint32_t w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        w[e] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w[e] |= static_cast<uint32_t>(tb[(4 * e + b) * 68]) << (8 * b);
      }
      if (n < a.N && m < a.M)
        *reinterpret_cast<uint4*>(qo.qT + static_cast<long long>(n) * qo.ldqt + m) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads of this pass done before the next pass overwrites
}

}  // namespace gemm
}  // namespace dtp

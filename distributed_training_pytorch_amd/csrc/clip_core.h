// Gradient clipping inside the fused step kernels (mlp_train_one.hip, mlp_train_lanes.hip):
// the clip twins of the update instances.
//
// Behind the step's reductions (the waves' sums, the split-batch members', the ranks') every
// thread holds the final gradient of its NPT owned parameters in registers, bitwise the same
// on every member and rank, so each workgroup clips on its own: nothing new crosses the chip
// or xGMI, no atomics, no host work (a 1000-step persistent launch and a graph replay clip
// every step).
//
//   by norm  (max_norm > 0):   x_k = g_k * grad_scale; the block's sum of x_k^2 in fp64 -- a
//                              thread's owned slots (k ascending, fma), the xor butterfly within
//                              a wave (in registers: DPP and lane swaps), one LDS double per
//                              wave, ONE barrier, the waves in order -- then
//                              x_k * clip_coef(norm, max_norm), one fp32 multiply
//   by value (clip_value > 0): clamp_value(x_k, clip_value); no reduction, no barrier
//
// which of the two is read from the argument block (a wave-uniform branch): one twin per
// update instance serves both.  The twin is a bit on the kernels' MODE template argument
// (kModeClip), so the plain instances keep their names and their device code.
#pragma once
#include "dtp_common.h"
#include "optim_core.h"

namespace dtp {

// internal: MODE | kModeClip instantiates the clip twin of an update mode (DtpTrainMode
// itself stays 0..4)
constexpr int kModeClip = 8;
constexpr int mode_base(int mode) { return mode & (kModeClip - 1); }
constexpr bool mode_clip(int mode) { return (mode & kModeClip) != 0; }

// The xor butterfly's exchanges without a trip through the LDS crossbar: as six dependent
// ds_bpermute pairs (__shfl_xor on a double) clipping by norm cost the 2.58 us split-batch step
// 0.61 us, this way 0.35 (profiles/fused_clip/).  Behind the steps before it every group of
// 2^k lanes holds one value (a + b == b + a bit for bit), so any lane of the partner group
// stands for lane ^ 2^k: DPP quad_perm for xor 1 and 2, row_half_mirror (lane 7 - i) for xor 4,
// row_mirror (15 - i) for xor 8, and gfx950's v_permlane16_swap / v_permlane32_swap for xor 16
// and 32 -- called with one value as both operands they return {own, partner} in the even rows
// (lower half) and {partner, own} in the odd rows (upper half): their sum either way.
template <int CTRL>
DTP_DEV double dpp_f64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)u, CTRL, 0xF, 0xF, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <bool HALVES>  // rows of 16 lanes (xor 16), or the wave's halves (xor 32)
DTP_DEV double swap_sum_f64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
  const auto a = HALVES ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false)
                        : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto b = HALVES ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false)
                        : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const double d0 = __longlong_as_double((long long)(((unsigned long long)b[0] << 32) | a[0]));
  const double d1 = __longlong_as_double((long long)(((unsigned long long)b[1] << 32) | a[1]));
  return d0 + d1;
}
// the sum of v over the wave's 64 lanes, the same bits on every lane: the xor butterfly's tree
DTP_DEV double wave_sum_f64(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror
  v = swap_sum_f64<false>(v);
  return swap_sum_f64<true>(v);
}

// L2 norm of the workgroup's gradient x (slot k of thread tid is parameter NPT tid + k; slots
// at or past P are not part of it, whatever they hold), the same bits on every thread.
// Every thread of the NW-wave workgroup calls it (one barrier).  The LDS doubles are written
// again only behind the step's closing barrier.
template <int NPT, int NW>
DTP_DEV float clip_block_norm(const float (&x)[NPT], int P, int tid) {
  __shared__ double wsum[NW];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const double xd = NPT * tid + k < P ? (double)x[k] : 0.0;
    s = fma(xd, xd, s);
  }
  s = wave_sum_f64(s);
  if ((tid & (kWave - 1)) == 0) wsum[tid / kWave] = s;
  __syncthreads();
  double t = wsum[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += wsum[w];
  return (float)sqrt(t);
}

// x_k = g_k * grad_scale, clipped as the argument block asks; returns the norm before
// clipping (by norm), else `norm` unchanged
template <int NPT, int NW>
DTP_DEV float clip_gradient(const DtpTrainArgs& a, const float (&g)[NPT], float (&x)[NPT], int P, int tid, float norm) {
#pragma unroll
  for (int k = 0; k < NPT; ++k) x[k] = g[k] * a.hp.grad_scale;
  if (a.max_norm > 0.f) {
    norm = clip_block_norm<NPT, NW>(x, P, tid);
    const float coef = clip_coef(norm, a.max_norm);
#pragma unroll
    for (int k = 0; k < NPT; ++k) x[k] = x[k] * coef;
  } else {
#pragma unroll
    for (int k = 0; k < NPT; ++k) x[k] = clamp_value(x[k], a.clip_value);
  }
  return norm;
}

}  // namespace dtp

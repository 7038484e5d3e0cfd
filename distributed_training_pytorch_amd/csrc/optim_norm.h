// Per-row gradient norm (clip by norm), shared by the flat optimizer kernels (optim.hip,
// optim_fp8.hip).
// The squares are summed in fp64 (a float squared is exact there) in an order fixed by P
// alone: every thread's chains, the xor butterfly within a wave (every lane ends with the
// same tree), the four waves as (w0 + w1) + (w2 + w3), and the per-block partials by the
// same block sum again.  No floating-point atomics: the norm is bitwise the same from run
// to run, in every block that forms it, and on every data-parallel replica.
#pragma once
#include "dtp_api.h"
#include "dtp_common.h"

namespace dtp {

constexpr int kNormUnroll = 4;                            // float4 loads in flight per thread
constexpr int kNormChunk = kNormUnroll * 4 * kBlock;      // elements per block and grid-stride iteration
constexpr int kNormMaxBlocks = 256;                       // per row: one block per CU, <= kBlock partials
constexpr int kOneBlockP = 16 * kBlock;                   // rows up to this take one block (norm + update fused)

__host__ __device__ inline int norm_blocks(int P) {
  const int nb = (P + kNormChunk - 1) / kNormChunk;
  return nb < kNormMaxBlocks ? nb : kNormMaxBlocks;
}

DTP_DEV double block_sum(double v) {
  __shared__ double wsum[kBlock / kWave];
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = v;
  __syncthreads();
  return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// this thread's share of sum((g[i] * gs)^2) over one row, as block `blk` of `nblk`.
// float4 loads with the update's head / tail treatment (an odd P leaves row 1 off a
// 16-byte boundary); the head and tail elements go to the first block's first threads.
DTP_DEV double row_sumsq(const float* g, int P, float gs, int blk, int nblk) {
  const uintptr_t ph = (uintptr_t)g & 15;
  const int head = min((int)((16 - ph) & 15) >> 2, P);
  const int P4 = (P - head) >> 2, tail0 = head + 4 * P4;
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (long long base = (long long)blk * (kNormUnroll * kBlock); base < P4; base += (long long)nblk * (kNormUnroll * kBlock)) {
    float4 q[kNormUnroll];
#pragma unroll
    for (int u = 0; u < kNormUnroll; ++u) {
      const long long i = base + u * kBlock + threadIdx.x;
      q[u] = i < P4 ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kNormUnroll; ++u) {
      const double x = (double)(q[u].x * gs), y = (double)(q[u].y * gs), z = (double)(q[u].z * gs), w = (double)(q[u].w * gs);
      a0 = fma(x, x, a0);
      a1 = fma(y, y, a1);
      a2 = fma(z, z, a2);
      a3 = fma(w, w, a3);
    }
  }
  const int e = blk == 0 ? (int)threadIdx.x : 1 << 30;
  const int idx = e < head ? e : (e - head < P - tail0 ? tail0 + e - head : -1);
  if (idx >= 0) {
    const double x = (double)(g[idx] * gs);
    a0 = fma(x, x, a0);
  }
  return (a0 + a1) + (a2 + a3);
}

// the row's sum of squares from its nb (<= kNormMaxBlocks <= kBlock) per-block partials
DTP_DEV double partials_sum(const double* ws, int nb) {
  static_assert(kNormMaxBlocks <= kBlock, "one partial per thread");
  return block_sum((int)threadIdx.x < nb ? ws[threadIdx.x] : 0.0);
}

// the whole block ends with the same value: the row's L2 norm.  ws == null: this block
// reads the whole row itself (one-block rows), else the norm kernel's partials.
DTP_DEV float row_norm(const float* g, int P, float gs, const double* ws) {
  const double s = ws ? partials_sum(ws, norm_blocks(P)) : block_sum(row_sumsq(g, P, gs, 0, 1));
  return (float)sqrt(s);
}

// the launches of optim.hip's kernels that optim_fp8.hip shares (host side, defined in optim.hip):
// rows of more than kOneBlockP elements: per-block fp64 partials into ws, [n_models][norm_blocks(P)]
void launch_norm_partials(const float* grad, int n_models, int P, float scale, double* ws, hipStream_t st);
// out[i] = row i's norm, from the partials (ws) or the row itself (ws == null)
void launch_norm_finish(const float* grad, int n_models, int P, float scale, const double* ws, float* out, hipStream_t st);
// step[i] += 1 behind a launch of more than one block per row
void launch_advance_steps(int* step, int n_models, hipStream_t st);

}  // namespace dtp

// Flat optimizer over [n_models][P] parameters after an external (RCCL)
// gradient all-reduce: one launch updates every model (the reference runs
// ~7 elementwise kernels per parameter tensor x 10 tensors x 2 models,
// SURVEY.md §2.6 K11).  The DDP 1/W averaging and the loss bookkeeping are
// fused in, and so is the bf16 compute copy of the weights (`shadow`): the
// bf16-compute GEMM path reads its weight operands from it instead of casting the
// fp32 masters before every forward (2 B/parameter written here vs a 6 B/parameter
// cast pass and one launch per weight tensor).
// Gradient clipping per row (clip_grad_norm_ / clip_grad_value_ semantics, one row = one
// optimizer) is a second instance of the same kernel body: the row's norm is formed in
// the optimizer's own launch (rows of one block) or from a norm launch's fp64 partials.
#include "dtp_api.h"
#include <type_traits>
#include "optim_core.h"

namespace dtp {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// ---- per-row gradient norm (clip by norm) ----
// The squares are summed in fp64 (a float squared is exact there) in an order fixed by P
// alone: every thread's chains, the xor butterfly within a wave (every lane ends with the
// same tree), the four waves as (w0 + w1) + (w2 + w3), and the per-block partials by the
// same block sum again.  No floating-point atomics: the norm is bitwise the same from run
// to run, in every block that forms it, and on every data-parallel replica.
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

__global__ __launch_bounds__(kBlock) void grad_norm_partial_kernel(const float* grad, int P, float gs, double* ws) {
  const double s = block_sum(row_sumsq(grad + (size_t)blockIdx.y * P, P, gs, blockIdx.x, gridDim.x));
  if (threadIdx.x == 0) ws[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// one block per row: out = the norm, from the partials (ws) or the row itself (ws == null)
__global__ __launch_bounds__(kBlock) void grad_norm_finish_kernel(const float* grad, int P, float gs, const double* ws,
                                                                  float* out) {
  const float n = row_norm(grad + (size_t)blockIdx.y * P, P, gs, ws ? ws + (size_t)blockIdx.y * norm_blocks(P) : nullptr);
  if (threadIdx.x == 0) out[blockIdx.y] = n;
}

// grad[row, :] *= clip_coef(norm, max_norm) in place (clip_grad_norm_ for users of a torch
// optimizer over the flat gradient); block 0 of every row publishes the norm.  Every lane
// is past the norm's reads (the barriers of the block sum) before the first store.
__global__ __launch_bounds__(kBlock) void grad_clip_scale_kernel(float* grad, int P, float max_norm, const double* ws,
                                                                 float* out) {
  float* g = grad + (size_t)blockIdx.y * P;
  const float n = row_norm(g, P, 1.f, ws ? ws + (size_t)blockIdx.y * norm_blocks(P) : nullptr);
  if (blockIdx.x == 0 && threadIdx.x == 0) out[blockIdx.y] = n;
  const float c = clip_coef(n, max_norm);
  if (c == 1.f) return;  // block-uniform: nothing to scale
  const uintptr_t ph = (uintptr_t)g & 15;
  const int head = min((int)((16 - ph) & 15) >> 2, P);
  const int P4 = (P - head) >> 2, tail0 = head + 4 * P4;
  float4* g4 = reinterpret_cast<float4*>(g + head);
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < P4; i += gridDim.x * kBlock) {
    float4 q = g4[i];
    q.x *= c, q.y *= c, q.z *= c, q.w *= c;
    g4[i] = q;
  }
  const int e = blockIdx.x == 0 ? (int)threadIdx.x : 1 << 30;
  const int idx = e < head ? e : (e - head < P - tail0 ? tail0 + e - head : -1);
  if (idx >= 0) g[idx] *= c;
}

// CLIP: the gradient-clipping instance (max_norm or clip_value set).  The plain instance
// compiles to what it was before clipping existed: every clip statement is `if constexpr`.
template <bool CLIP>
DTP_DEV void flat_optimizer_body(const DtpOptArgs& a) {
  const int model = blockIdx.y;
  const long long t = a.step[model];
  // what the update consumes: the averaged gradient, clipped by value or scaled by the
  // row's norm coefficient (formed below, before the first parameter is written)
  [[maybe_unused]] float coef = 1.f;
  const auto gx = [&](float raw) {
    const float s = raw * a.hp.grad_scale;
    if constexpr (CLIP) return a.clip_value > 0.f ? clamp_value(s, a.clip_value) : s * coef;
    else return s;
  };
  float* p = a.params + (size_t)model * a.P;
  float* m = a.opt_m + (size_t)model * a.P;
  float* v = a.opt_v ? a.opt_v + (size_t)model * a.P : nullptr;
  const float* g = a.grad + (size_t)model * a.P;
  // DTP_OPT_ZERO_GRAD: the consumed gradient is zeroed in the same pass (the Trainer's
  // module path then needs no zero_grad fill launch before the next backward)
  const bool zg = a.flags & DTP_OPT_ZERO_GRAD;
  float* const gz = const_cast<float*>(g);
  __bf16* sh = a.shadow ? reinterpret_cast<__bf16*>(a.shadow) + (size_t)model * a.shadow_ld : nullptr;
  if constexpr (CLIP) {
    // one-block rows: the norm over the row, then the update, in this launch -- the block
    // sum's barriers put every lane past its norm reads before any lane writes a parameter
    // or zeroes a gradient element.  Larger rows: every block sums the norm kernel's
    // partials in the same order, so all of them scale by the same coefficient.
    if (a.max_norm > 0.f) {
      const float n = row_norm(g, a.P, a.hp.grad_scale,
                               gridDim.x == 1 ? nullptr : a.norm_ws + (size_t)model * norm_blocks(a.P));
      if (blockIdx.x == 0 && threadIdx.x == 0) a.norm_out[model] = n;
      coef = clip_coef(n, a.max_norm);
    }
  }
  // float4 body: the four rows share their offset within 16 bytes (same [n][P] layout
  // on 16-byte aligned bases), so `head` scalar elements (0-3) bring every row to a
  // 16-byte boundary, the body runs 4 elements per thread and load, and at most 3
  // elements remain (the update is HBM-bound: 28 B per parameter). With an odd P the
  // second model's row starts off a 16-byte boundary: before the head peel it ran
  // the element-wise loop.
  const uintptr_t ph = (uintptr_t)p & 15;
  const bool vec = v && (((uintptr_t)m & 15) == ph) && (((uintptr_t)v & 15) == ph) && (((uintptr_t)g & 15) == ph) &&
                   (ph & 3) == 0 && (!sh || (ph == 0 && (a.P & 3) == 0 && ((uintptr_t)sh & 7) == 0));
  // The Adam rows in two versions behind one block-uniform test: DEC = false is the loop as
  // it was before AdamW existed (what a launch with weight_decay == 0 or the coupled decay
  // runs), DEC = true scales each parameter by the step's d_t first (optim_core.h)
  const auto adam_rows = [&](auto DEC) {
  constexpr bool kDec = decltype(DEC)::value;
  if (vec) {
    const AdamScalars s = adam_scalars_v<kDec>(a.hp, t + 1);
    const int head = min((int)((16 - ph) & 15) >> 2, a.P);
    const int P4 = (a.P - head) >> 2, tail0 = head + 4 * P4;
    float4* p4 = reinterpret_cast<float4*>(p + head);
    float4* m4 = reinterpret_cast<float4*>(m + head);
    float4* v4 = reinterpret_cast<float4*>(v + head);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < P4; i += gridDim.x * kBlock) {
      float4 w = p4[i], mi = m4[i], vi = v4[i];
      const float4 gi = g4[i];
      if (zg) reinterpret_cast<float4*>(gz + head)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      adamw_update_v<kDec>(w.x, mi.x, vi.x, gx(gi.x), s);
      adamw_update_v<kDec>(w.y, mi.y, vi.y, gx(gi.y), s);
      adamw_update_v<kDec>(w.z, mi.z, vi.z, gx(gi.z), s);
      adamw_update_v<kDec>(w.w, mi.w, vi.w, gx(gi.w), s);
      p4[i] = w;
      m4[i] = mi;
      v4[i] = vi;
      if (sh) reinterpret_cast<bf16x4*>(sh)[i] = bf16x4{(__bf16)w.x, (__bf16)w.y, (__bf16)w.z, (__bf16)w.w};
    }
    // the head and tail elements (at most 6), one per thread of the first block
    const int e = blockIdx.x == 0 ? (int)threadIdx.x : 1 << 30;
    const int idx = e < head ? e : (e - head < a.P - tail0 ? tail0 + e - head : -1);
    if (idx >= 0) {
      float w = p[idx], mi = m[idx], vi = v[idx];
      const float gv = g[idx];
      if (zg) gz[idx] = 0.f;
      adamw_update_v<kDec>(w, mi, vi, gx(gv), s);
      p[idx] = w;
      m[idx] = mi;
      v[idx] = vi;
      if (sh) sh[idx] = (__bf16)w;
    }
  } else if (sh) {
    // unaligned rows (odd P: every bias-terminated MLP) with a shadow: two elements per
    // thread, so the shadow is written as one 4-byte bf16 pair per lane (the shadow's
    // rows are 512-byte aligned, ComputeShadow); single 2-byte stores per lane ran the
    // whole kernel 15 % slower
    const AdamScalars s = adam_scalars_v<kDec>(a.hp, t + 1);
    const int P2 = (a.P + 1) >> 1;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < P2; j += gridDim.x * kBlock) {
      const int i = 2 * j;
      const bool two = i + 1 < a.P;
      float w0 = p[i], m0 = m[i], v0 = v[i];
      const float g0 = g[i];
      float w1 = 0.f, m1 = 0.f, v1 = 0.f, g1 = 0.f;
      if (two) w1 = p[i + 1], m1 = m[i + 1], v1 = v[i + 1], g1 = g[i + 1];
      if (zg) {
        gz[i] = 0.f;
        if (two) gz[i + 1] = 0.f;
      }
      adamw_update_v<kDec>(w0, m0, v0, gx(g0), s);
      p[i] = w0;
      m[i] = m0;
      v[i] = v0;
      if (two) {
        adamw_update_v<kDec>(w1, m1, v1, gx(g1), s);
        p[i + 1] = w1;
        m[i + 1] = m1;
        v[i + 1] = v1;
        *reinterpret_cast<bf16x2*>(sh + i) = bf16x2{(__bf16)w0, (__bf16)w1};
      } else {
        sh[i] = (__bf16)w0;
      }
    }
  } else {
    const AdamScalars s = adam_scalars_v<kDec>(a.hp, t + 1);
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.P; i += gridDim.x * kBlock) {
      float w = p[i], mi = m[i], vi = v[i];
      const float gv = g[i];
      if (zg) gz[i] = 0.f;
      adamw_update_v<kDec>(w, mi, vi, gx(gv), s);
      p[i] = w;
      m[i] = mi;
      v[i] = vi;
    }
  }
  };
  if (a.kind == DTP_MODE_ADAM) {
    if (decoupled_on(a.hp)) adam_rows(std::true_type{});
    else adam_rows(std::false_type{});
  } else {
    const float lr = (float)lr_of(a.hp, t), mom = (float)a.hp.momentum, wd = (float)a.hp.weight_decay;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.P; i += gridDim.x * kBlock) {
      float w = p[i], bi = m[i];
      const float gv = g[i];
      if (zg) gz[i] = 0.f;
      sgd_update(w, bi, gx(gv), lr, mom, wd, t == 0);
      p[i] = w;
      m[i] = bi;
      if (sh) sh[i] = (__bf16)w;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (a.loss_log)
      a.loss_log[(size_t)(t % a.loss_log_cap) * a.n_models + model] = a.grad[(size_t)a.n_models * a.P + model] * a.loss_scale;
  }
  // the step counter is read by every block of this model: advance it only
  // after the grid is done -> done by the last block via a ticket would cost a
  // fence; instead the counter is advanced by a 1-block follow-up in the same
  // stream when gridDim.x > 1 (see launcher).
  if (gridDim.x == 1 && threadIdx.x == 0) a.step[model] = (int)(t + 1);
}

__global__ __launch_bounds__(kBlock) void flat_optimizer_kernel(DtpOptArgs a) { flat_optimizer_body<false>(a); }
__global__ __launch_bounds__(kBlock) void flat_optimizer_clip_kernel(DtpOptArgs a) { flat_optimizer_body<true>(a); }

__global__ void advance_steps_kernel(int* step, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) step[i] += 1;
}

}  // namespace dtp

namespace {
using dtp::check_launch;
using dtp::set_err;

// rows of more than kOneBlockP elements: per-block fp64 partials into ws, [n_models][norm_blocks(P)]
void launch_norm_partials(const float* grad, int n_models, int P, float scale, double* ws, hipStream_t st) {
  hipLaunchKernelGGL(dtp::grad_norm_partial_kernel, dim3(dtp::norm_blocks(P), n_models), dim3(dtp::kBlock), 0, st, grad, P,
                     scale, ws);
}
}  // namespace

extern "C" long long dtp_grad_norm_ws_bytes(int P) {
  return P > dtp::kOneBlockP ? (long long)dtp::norm_blocks(P) * (long long)sizeof(double) : 0;
}

extern "C" int dtp_grad_norm(const float* grad, int n_models, int P, float scale, double* ws, float* out, void* stream) {
  if (!grad || !out || P <= 0 || n_models <= 0 || n_models > 65535) return set_err(-1, "grad_norm: bad arguments");
  const bool multi = P > dtp::kOneBlockP;
  if (multi && !ws) return set_err(-5, "grad_norm: rows of more than 4096 elements need the workspace");
  hipStream_t st = (hipStream_t)stream;
  if (multi) launch_norm_partials(grad, n_models, P, scale, ws, st);
  hipLaunchKernelGGL(dtp::grad_norm_finish_kernel, dim3(1, n_models), dim3(dtp::kBlock), 0, st, grad, P, scale,
                     multi ? (const double*)ws : nullptr, out);
  return check_launch("grad_norm_kernel");
}

extern "C" int dtp_clip_grad_norm(float* grad, int n_models, int P, float max_norm, double* ws, float* out, void* stream) {
  if (!grad || !out || P <= 0 || n_models <= 0 || n_models > 65535 || !(max_norm > 0.f))
    return set_err(-1, "clip_grad_norm: bad arguments (max_norm must be > 0)");
  const bool multi = P > dtp::kOneBlockP;
  if (multi && !ws) return set_err(-5, "clip_grad_norm: rows of more than 4096 elements need the workspace");
  hipStream_t st = (hipStream_t)stream;
  if (multi) launch_norm_partials(grad, n_models, P, 1.f, ws, st);
  int nblk = multi ? (P + 4 * dtp::kBlock - 1) / (4 * dtp::kBlock) : 1;
  if (nblk > 1024) nblk = 1024;
  hipLaunchKernelGGL(dtp::grad_clip_scale_kernel, dim3(nblk, n_models), dim3(dtp::kBlock), 0, st, grad, P, max_norm,
                     multi ? (const double*)ws : nullptr, out);
  return check_launch("grad_clip_scale_kernel");
}

extern "C" int dtp_flat_optimizer(const DtpOptArgs* a, void* stream) {
  if (!a || a->P <= 0 || a->n_models <= 0) return -1;
  if (a->kind != DTP_MODE_ADAM && a->kind != DTP_MODE_SGD) return -2;
  if (a->hp.decoupled_wd && a->kind != DTP_MODE_ADAM)
    return set_err(-1, "flat_optimizer: decoupled weight decay (AdamW) is Adam's: SGD has no decoupled form");
  if (a->hp.lr_tab && a->hp.lr_tab_len <= 0) return set_err(-6, "flat_optimizer: a learning-rate table needs at least one entry");
  hipStream_t st = (hipStream_t)stream;
  // small models (the toy's 371 parameters): one block per model loops over its
  // parameters and advances the step counter itself -- no follow-up launch
  int nblk = a->P <= dtp::kOneBlockP ? 1 : (a->P + dtp::kBlock - 1) / dtp::kBlock;
  if (nblk > 1024) nblk = 1024;
  dim3 grid(nblk, a->n_models), block(dtp::kBlock);
  const bool by_norm = a->max_norm > 0.f, by_value = a->clip_value > 0.f;
  if (by_norm && by_value) return set_err(-4, "flat_optimizer: max_norm and clip_value are exclusive");
  if (by_norm && (!a->norm_out || (nblk > 1 && !a->norm_ws)))
    return set_err(-5, "flat_optimizer: clipping by norm needs norm_out (and norm_ws for rows of more than 4096 elements)");
  if (by_norm || by_value) {
    // the clipped instance; rows of more than one block get their norm's partials from a
    // launch of its own first (the grid of the update is not the grid of the norm)
    if (by_norm && nblk > 1) launch_norm_partials(a->grad, a->n_models, a->P, a->hp.grad_scale, a->norm_ws, st);
    hipLaunchKernelGGL(dtp::flat_optimizer_clip_kernel, grid, block, 0, st, *a);
  } else {
    hipLaunchKernelGGL(dtp::flat_optimizer_kernel, grid, block, 0, st, *a);
  }
  // one thread per model: a single 64-thread block left the counters of models 64.. at
  // their old step (those models then kept the first step's bias correction)
  if (nblk > 1)
    hipLaunchKernelGGL(dtp::advance_steps_kernel, dim3((a->n_models + 63) / 64), dim3(64), 0, st, a->step, a->n_models);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

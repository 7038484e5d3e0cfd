// The flat optimizer that also writes the FP8 weight operands of the delayed-scaling recipe.
//
// Under delayed scaling a weight's scale is known before the weight is, and the optimizer holds the new
// fp32 master in registers one launch before the forward would read it back to quantise it.  So this
// launch does dtp_flat_optimizer's update over [n_models][P] and, for every shadowed weight (a contiguous
// [out][in] matrix inside a row, both widths multiples of 16), what dtp_fp8_quantize_scaled would do to the
// updated matrix: the e4m3 copy, its transpose, and the |p| amax partials of the scale record.
//
// How the work is split: one launch over a device table of work items, one workgroup (256 threads) each.
//  * Tile items: a 64 x 64 tile of a shadowed weight.  A thread owns four 16-byte vectors of the tile (rows
//    tid / 16 + 16 j, 4 consecutive k): it loads p, g, m, v of each (element loads where the matrix starts off
//    a 16-byte boundary: an odd P puts every second row of the bank there), updates, stores p, m, v, and keeps
//    the new p: its |p| bit pattern goes into the thread's running maximum, cvt(clamp(p * scale, +-448)) as one
//    packed word into the LDS image of the tile ([64] rows of 17 words: the odd stride spreads the byte gather
//    of the transpose over the banks, as in fp8_quant.hip).  Behind the block maximum's barriers every thread
//    writes 16 bytes of one row of q and gathers 16 bytes of one row of qT (16 m of one k) from the image.
//    64 x 64 and not larger: the tile is also the granule of the amax partials (DtpFp8ScaleRec::partials,
//    one word per tile, the count in word 0), which the given-scale quantiser writes in the same geometry,
//    and 16 KB of fp32 per array per workgroup already keeps 16 vector loads per thread in flight.
//  * Span items: every other element of the row (biases, the first and last layer, layers of other widths) in
//    chunks, element by element: dtp_flat_optimizer's update, the same bits.
// The update itself is optim_core.h's (this source builds with -ffp-contract=off, as optim.hip) and the
// quantiser's product and clamp are single fp32 operations (no packed fp32 forms, as fp8_quant.hip).
// The scale: read from the slot through the record; tile 0 of a weight copies {scale, 1 / scale} into the
// record's `used` pair, since the slot's scale is formed again before the forward's GEMM reads the operand.
// Clipping by norm: the norm comes from a launch of its own first (other workgroups of the row zero and
// consume the gradient, so no workgroup may read the whole row here): its partials, summed by every workgroup
// in the same order, for rows of more than 4096 elements, else the finished norm in norm_out.
#include "dtp_api.h"
#include <type_traits>
#include "optim_core.h"
#include "optim_norm.h"

namespace dtp {
namespace optfp8 {

constexpr int kTile = 64;
constexpr int kStrideW = 17;  // LDS row stride in 4-byte words
constexpr float kFmax = 448.f;

enum { kAdam = 0, kAdamW = 1, kSgd = 2 };

// what every element's update needs, block-uniform
struct Ctx {
  AdamScalars s;
  float lr, mom, wd;
  bool first_step;
  float gs, coef, clip_value;
  bool zg;
};

template <int MODE>
DTP_DEV void update(float& w, float& m, float& v, float raw, const Ctx& c) {
  // the gradient treatment of flat_optimizer_body's gx(): averaged, then clipped by value or by the row's norm
  const float s = raw * c.gs;
  const float g = c.clip_value > 0.f ? clamp_value(s, c.clip_value) : s * c.coef;
  if constexpr (MODE == kSgd) sgd_update(w, m, g, c.lr, c.mom, c.wd, c.first_step);
  else adamw_update_v<MODE == kAdamW>(w, m, v, g, c.s);
}

template <bool VEC>
DTP_DEV void load4(const float* p, float (&x)[4]) {
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
  } else {
    x[0] = p[0], x[1] = p[1], x[2] = p[2], x[3] = p[3];
  }
}

template <bool VEC>
DTP_DEV void store4(float* p, const float (&x)[4]) {
  if constexpr (VEC) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  else p[0] = x[0], p[1] = x[1], p[2] = x[2], p[3] = x[3];
}

DTP_DEV uint32_t block_max(uint32_t v, uint32_t* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o, kWave)));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  v = max(max(red[0], red[1]), max(red[2], red[3]));
  __syncthreads();
  return v;
}

DTP_DEV float clamp_abs(float v, float lim) { return fminf(fmaxf(v, -lim), lim); }

// four e4m3 bytes, round to nearest even (the packed hardware convert)
DTP_DEV uint32_t cvt4_e4m3(float a, float b, float c, float d) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return static_cast<uint32_t>(w);
}

template <int MODE, bool VEC>
DTP_DEV void tile_item(const DtpOptArgs& a, const DtpFp8ShadowRec& r, int tile, const Ctx& c, uint32_t* img, uint32_t* red) {
  const int tid = threadIdx.x;
  const int tk = (r.in + kTile - 1) / kTile, tm = (r.out + kTile - 1) / kTile;
  const int k0 = (tile % tk) * kTile, m0 = (tile / tk) * kTile;
  const float scale = r.scale[0];
  float* p = a.params + r.offset;
  float* m = a.opt_m + r.offset;
  float* v = MODE == kSgd ? nullptr : a.opt_v + r.offset;
  float* g = const_cast<float*>(a.grad) + r.offset;
  uint32_t tmax = 0;  // the |p_new| bit patterns of this thread (an unsigned compare orders non-negative floats)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int vi = tid + 256 * j, row = vi >> 4, cc = vi & 15;
    uint32_t word = 0;  // rows past `out` and columns past `in` stay zero bytes in the image
    if (m0 + row < r.out && k0 + 4 * cc < r.in) {
      const long long e = static_cast<long long>(m0 + row) * r.in + k0 + 4 * cc;
      float w[4], mi[4], vv[4] = {0.f, 0.f, 0.f, 0.f}, gi[4];
      load4<VEC>(p + e, w);
      load4<VEC>(m + e, mi);
      if constexpr (MODE != kSgd) load4<VEC>(v + e, vv);
      load4<VEC>(g + e, gi);
      if (c.zg) {
        const float z[4] = {0.f, 0.f, 0.f, 0.f};
        store4<VEC>(g + e, z);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) update<MODE>(w[q], mi[q], vv[q], gi[q], c);
      store4<VEC>(p + e, w);
      store4<VEC>(m + e, mi);
      if constexpr (MODE != kSgd) store4<VEC>(v + e, vv);
#pragma unroll
      for (int q = 0; q < 4; ++q) tmax = max(tmax, __float_as_uint(w[q]) & 0x7fffffffu);
      word = cvt4_e4m3(clamp_abs(w[0] * scale, kFmax), clamp_abs(w[1] * scale, kFmax), clamp_abs(w[2] * scale, kFmax),
                       clamp_abs(w[3] * scale, kFmax));
    }
    img[row * kStrideW + cc] = word;
  }
  tmax = block_max(tmax, red, tid);  // (ends with a barrier: the image is complete behind it)
  if (tid == 0) r.partials[1 + tile] = tmax;
  if (tid == 0 && tile == 0) {
    r.partials[0] = static_cast<unsigned>(tk * tm);
    r.used[0] = scale;
    r.used[1] = r.scale[1];
  }
  uint8_t* q8 = static_cast<uint8_t*>(r.q);
  uint8_t* t8 = static_cast<uint8_t*>(r.qT);
  {  // row-major copy: 16 k of one row per thread
    const int row = tid >> 2, seg = tid & 3;
    if (m0 + row < r.out && k0 + 16 * seg < r.in) {
      const uint32_t* t = img + row * kStrideW + 4 * seg;
      *reinterpret_cast<uint4*>(q8 + static_cast<long long>(m0 + row) * r.in + k0 + 16 * seg) = make_uint4(t[0], t[1], t[2], t[3]);
    }
  }
  {  // transposed copy: 16 rows of one k per thread, gathered from the image by byte reads
    const int k = tid >> 2, mg = tid & 3;
    if (k0 + k < r.in && m0 + 16 * mg < r.out) {
      const uint8_t* tb = reinterpret_cast<const uint8_t*>(img) + (16 * mg) * (kStrideW * 4) + k;
      uint32_t w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        w[e] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w[e] |= static_cast<uint32_t>(tb[(4 * e + b) * (kStrideW * 4)]) << (8 * b);
      }
      *reinterpret_cast<uint4*>(t8 + static_cast<long long>(k0 + k) * r.out + m0 + 16 * mg) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

template <int MODE>
DTP_DEV void span_item(const DtpOptArgs& a, const DtpFp8WorkItem& it, const Ctx& c) {
  const size_t row = static_cast<size_t>(it.model) * a.P;
  float* p = a.params + row;
  float* m = a.opt_m + row;
  float* v = MODE == kSgd ? nullptr : a.opt_v + row;
  float* g = const_cast<float*>(a.grad) + row;
  const int lo = max(it.a, 0), hi = static_cast<int>(min(static_cast<long long>(it.a) + it.b, static_cast<long long>(a.P)));
  for (int i = lo + static_cast<int>(threadIdx.x); i < hi; i += kBlock) {
    float w = p[i], mi = m[i], vv = 0.f;
    if constexpr (MODE != kSgd) vv = v[i];
    const float gv = g[i];
    if (c.zg) g[i] = 0.f;
    update<MODE>(w, mi, vv, gv, c);
    p[i] = w;
    m[i] = mi;
    if constexpr (MODE != kSgd) v[i] = vv;
  }
}

template <int MODE>
DTP_DEV void run_item(const DtpOptArgs& a, const DtpFp8ShadowWork& wk, int n_recs, const DtpFp8WorkItem& it, Ctx& c, long long t,
                      uint32_t* img, uint32_t* red) {
  if constexpr (MODE == kSgd) {
    c.lr = static_cast<float>(lr_of(a.hp, t)), c.mom = static_cast<float>(a.hp.momentum);
    c.wd = static_cast<float>(a.hp.weight_decay), c.first_step = t == 0;
  } else {
    c.s = adam_scalars_v<MODE == kAdamW>(a.hp, t + 1);
  }
  if (it.rec < 0) {
    span_item<MODE>(a, it, c);
    return;
  }
  if (it.rec >= n_recs) return;  // (block-uniform; the host builds the table, this only keeps a bad one in bounds)
  const DtpFp8ShadowRec r = wk.recs[it.rec];
  if (it.a < 0 || it.a >= ((r.in + kTile - 1) / kTile) * ((r.out + kTile - 1) / kTile)) return;
  // all four arrays share the matrix's offset, and `in` is a multiple of 16: one test for every vector of the tile
  const bool vec = ((reinterpret_cast<uintptr_t>(a.params + r.offset) | reinterpret_cast<uintptr_t>(a.opt_m + r.offset) |
                     reinterpret_cast<uintptr_t>(a.grad + r.offset) |
                     (MODE == kSgd ? 0 : reinterpret_cast<uintptr_t>(a.opt_v + r.offset))) & 15) == 0;
  if (vec) tile_item<MODE, true>(a, r, it.a, c, img, red);
  else tile_item<MODE, false>(a, r, it.a, c, img, red);
}

__global__ __launch_bounds__(kBlock) void flat_optimizer_fp8_kernel(DtpOptArgs a, DtpFp8ShadowWork wk, int n_recs) {
  __shared__ uint32_t red[4];
  __shared__ uint32_t img[kTile * kStrideW];
  const DtpFp8WorkItem it = wk.items[blockIdx.x];
  const int model = it.model;
  if (model < 0 || model >= a.n_models) return;
  const long long t = a.step[model];
  Ctx c;
  c.gs = a.hp.grad_scale, c.coef = 1.f, c.clip_value = a.clip_value, c.zg = a.flags & DTP_OPT_ZERO_GRAD;
  if (a.max_norm > 0.f) {
    const bool multi = a.P > kOneBlockP;
    const float n = multi ? row_norm(a.grad + static_cast<size_t>(model) * a.P, a.P, a.hp.grad_scale,
                                     a.norm_ws + static_cast<size_t>(model) * norm_blocks(a.P))
                          : a.norm_out[model];
    if (multi && it.first && threadIdx.x == 0) a.norm_out[model] = n;
    c.coef = clip_coef(n, a.max_norm);
  }
  if (it.first && threadIdx.x == 0 && a.loss_log)
    a.loss_log[static_cast<size_t>(t % a.loss_log_cap) * a.n_models + model] =
        a.grad[static_cast<size_t>(a.n_models) * a.P + model] * a.loss_scale;
  if (a.kind == DTP_MODE_ADAM) {
    if (decoupled_on(a.hp)) run_item<kAdamW>(a, wk, n_recs, it, c, t, img, red);
    else run_item<kAdam>(a, wk, n_recs, it, c, t, img, red);
  } else {
    run_item<kSgd>(a, wk, n_recs, it, c, t, img, red);
  }
}

}  // namespace optfp8
}  // namespace dtp

extern "C" int dtp_flat_optimizer_fp8(const DtpOptArgs* a, const DtpFp8ShadowRec* recs, int n_recs, const DtpFp8ShadowWork* work,
                                      void* stream) {
  using namespace dtp;
  if (!a || a->P <= 0 || a->n_models <= 0 || !a->params || !a->opt_m || !a->grad || !a->step)
    return set_err(-1, "flat_optimizer_fp8: bad arguments");
  if (a->kind != DTP_MODE_ADAM && a->kind != DTP_MODE_SGD) return set_err(-2, "flat_optimizer_fp8: kind must be Adam or SGD");
  if (a->kind == DTP_MODE_ADAM && !a->opt_v) return set_err(-1, "flat_optimizer_fp8: Adam needs opt_v");
  if (a->hp.decoupled_wd && a->kind != DTP_MODE_ADAM)
    return set_err(-1, "flat_optimizer_fp8: decoupled weight decay (AdamW) is Adam's: SGD has no decoupled form");
  if (a->hp.lr_tab && a->hp.lr_tab_len <= 0) return set_err(-6, "flat_optimizer_fp8: a learning-rate table needs at least one entry");
  if (a->shadow) return set_err(-1, "flat_optimizer_fp8: the bf16 shadow is dtp_flat_optimizer's");
  const bool by_norm = a->max_norm > 0.f, by_value = a->clip_value > 0.f, multi = a->P > kOneBlockP;
  if (by_norm && by_value) return set_err(-4, "flat_optimizer_fp8: max_norm and clip_value are exclusive");
  if (by_norm && (!a->norm_out || (multi && !a->norm_ws)))
    return set_err(-5, "flat_optimizer_fp8: clipping by norm needs norm_out (and norm_ws for rows of more than 4096 elements)");
  if (!recs || n_recs <= 0 || !work || !work->recs || !work->items || work->n_items <= 0)
    return set_err(-7, "flat_optimizer_fp8: no records or no work table");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const long long total = static_cast<long long>(a->n_models) * a->P;
  for (int i = 0; i < n_recs; ++i) {
    const DtpFp8ShadowRec& r = recs[i];
    if (!r.scale || !r.partials || !r.used || !r.q || !r.qT)
      return set_err(-8, "flat_optimizer_fp8: a record needs scale, partials, used, q and qT");
    if (r.out <= 0 || r.in <= 0 || r.out % 16 || r.in % 16)
      return set_err(-9, "flat_optimizer_fp8: both widths of a shadowed weight must be multiples of 16");
    const long long n = static_cast<long long>(r.out) * r.in;
    if (r.offset < 0 || r.offset + n > total || r.offset / a->P != (r.offset + n - 1) / a->P)
      return set_err(-10, "flat_optimizer_fp8: a shadowed weight must lie inside one row of the flat buffer");
    if (!al16(r.q) || !al16(r.qT)) return set_err(-11, "flat_optimizer_fp8: q and qT must be 16-byte aligned");
    const long long tiles = static_cast<long long>((r.out + 63) / 64) * ((r.in + 63) / 64);
    if (tiles > r.cap) return set_err(-12, "flat_optimizer_fp8: more tiles than the partials buffer holds");
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (by_norm) {
    if (multi) launch_norm_partials(a->grad, a->n_models, a->P, a->hp.grad_scale, a->norm_ws, st);
    else launch_norm_finish(a->grad, a->n_models, a->P, a->hp.grad_scale, nullptr, a->norm_out, st);
  }
  hipLaunchKernelGGL(optfp8::flat_optimizer_fp8_kernel, dim3(work->n_items), dim3(kBlock), 0, st, *a, *work, n_recs);
  launch_advance_steps(a->step, a->n_models, st);
  return check_launch("flat_optimizer_fp8_kernel");
}

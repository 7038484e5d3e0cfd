// The several-lanes / split-batch step kernel (mlp_train_lanes_kernel), the families it is
// instantiated for and the helper that fills one variant of a family's table row.  Shared by the
// three sources that instantiate it, one per step variant, so that they compile side by side:
// mlp_train_lanes.hip (the plain instances and the table), mlp_train_lanes_clip.hip and
// mlp_train_lanes_accum.hip (the twins).
#pragma once
#include "mlp_train_common.h"
#include "mlp_lanes.h"
#include "mlp_pipe.h"
#include "mlp_scalar.h"
#include "optim_core.h"
#include "clip_core.h"
#include "accum_core.h"
#include "xgmi_core.h"
#include "grp_core.h"

namespace dtp {

// staging areas of one wave: the packed first/last tile (or the last layer's and the first
// layer's when they do not pack) and ONE area shared by the hidden layers -- a wave's LDS
// operations execute in order, so layer l-1's staging writes land after layer l's MFMA
// operand reads were issued (the constant-1 bias column, written once, is the same
// column in every hidden tile)
template <class S>
DTP_HD constexpr int lane_areas() { return Scal<S>::PACK ? 2 : 3; }
template <class S>
DTP_HD constexpr int lane_area(int l) {
  return (Scal<S>::PACK && (l == 0 || l == S::NL - 1)) ? 0 : (l == S::NL - 1 ? 0 : (l == 0 ? 2 : 1));
}

// payload float of dW tile cell (tile t, row, col): the torch-order parameter whose gradient
// the cell holds (the inverse of lane_pos's tp), P for the loss cell, -1 for a cell of no one
template <class S>
DTP_HD constexpr int lane_row_slot(int t, int row, int col) {
  using SC = Scal<S>;
  for (int l = 0; l < S::NL; ++l) {
    if (SC::tile(l) != t) continue;
    const int j = row - SC::rowoff(l), i = col - SC::coloff(l), I = S::din(l);
    if (j >= 0 && j < S::dout(l) && i >= 0 && i <= I) return i < I ? S::gw(l) + j * I + i : S::gb(l) + j;
  }
  if (t == SC::tile(S::NL - 1) && row == SC::lossrow() && col == SC::losscol()) return S::P;
  return -1;
}
// the map is a bijection from the real tile cells onto [0, P], and sends the cell lane_pos
// gives parameter p (tile(l), rowoff + j, coloff + i) back to p
template <class S>
constexpr bool lane_row_map_ok() {
  using SC = Scal<S>;
  int hits[S::P + 1] = {};
  for (int t = 0; t < SC::NT; ++t)
    for (int row = 0; row < 16; ++row)
      for (int col = 0; col < 16; ++col) {
        const int f = lane_row_slot<S>(t, row, col);
        if (f > S::P) return false;
        if (f >= 0) ++hits[f];
      }
  for (int f = 0; f <= S::P; ++f)
    if (hits[f] != 1) return false;
  for (int l = 0; l < S::NL; ++l)
    for (int j = 0; j < S::dout(l); ++j)
      for (int i = 0; i <= S::din(l); ++i) {
        const int p = i < S::din(l) ? S::gw(l) + j * S::din(l) + i : S::gb(l) + j;
        if (lane_row_slot<S>(SC::tile(l), SC::rowoff(l) + j, SC::coloff(l) + i) != p) return false;
      }
  return true;
}

// ROWS: the per-wave partial dW sums are parked in payload order (grp_core.h):
// one row of grp_row_floats(P) floats per wave, then one sink float per lane for the tile
// cells that hold no parameter
template <class S, int L, int NW, bool GRP = false, bool ROWS = false>
struct LaneSmem {
  using C = LaneCfg<S, L>;
  static constexpr int RSINK = grp_row_floats(S::P);  // a row's sink floats start here
  static constexpr int RSTR = RSINK + kWave;          // row stride
  alignas(16) float wb[C::pad4(C::LW)];
  alignas(16) float stg[NW][lane_areas<S>()][2 * C::AREA];  // per wave, per area: dz operand, h operand
  alignas(16) float red[NW][ROWS ? RSTR : Scal<S>::NT * Scal<S>::TSZ];  // per-wave partial dW tiles (or rows)
  alignas(16) float2 adam_tab[kAdamTab];
  alignas(16) float data[kLaneData];
  float sink[4];
  // the exchanges' LDS, in float2: the on-chip one's (kGrpMax + 1) rows of grp_ps3(P) floats
  // (grp_core.h) or the 3-float xGMI one's xgmi_g3_lds_floats(P) floats (xgmi_core.h)
  // GSLOT: (kGrpMax + 1) slots of 2-float granules, which no exchange here stages in LDS any
  // more; the term still sets the LDS size of the 3-layer, the 15-wide and the 8-wave
  // split-batch instances, and stays until a change that may alter the kernels' descriptors
  static constexpr int GSLOT = xgmi_slot16(S::P, (S::P + 64 * NW - 1) / (64 * NW));
  static constexpr int GX2a = (kGrpMax + 1) * GSLOT > (kGrpMax + 1) * grp_ps3(S::P) / 2
                                  ? (kGrpMax + 1) * GSLOT : (kGrpMax + 1) * grp_ps3(S::P) / 2;
  static constexpr int GX2 = GX2a > xgmi_g3_lds_floats(S::P) / 2 ? GX2a : xgmi_g3_lds_floats(S::P) / 2;
  alignas(16) float2 gx[GRP ? GX2 : 2];
};

// waves per SIMD the register budget is set for: 2 on the 4-wave split-batch instances (256
// VGPRs, 169 used; they still run one wave per SIMD), so that the dW tiles' MFMAs write
// VGPRs -- with the 512 registers of one wave per SIMD the compiler puts their results in
// AGPRs and copies every tile out (8 v_accvgpr_read and the s_nop in front of them per tile)
template <int NW, bool GRP>
constexpr int lanes_wpe = (GRP && NW == 4) ? 2 : NW / 4;

// NW waves per workgroup (4: one per SIMD; 8: two per SIMD, for batches of 256 / L < B <= 512 / L)
// GRP: the batch split over a.groups workgroups per model (grp_core.h): member k of model m
// is block m + 8 k (the members of a model share an XCD under round-robin dispatch), runs
// the step on batch positions [k 64 NW / L, (k + 1) 64 NW / L), and the members' partial
// weight gradients and losses are summed on chip before every member's (identical)
// optimizer step.
// CE: softmax cross-entropy head (class ids as floats in Y) instead of MSE; MODE: Adam or
// SGD (momentum, weight decay), local or with the in-kernel xGMI exchange.
// GRC > 0: the member count of the split-batch step as a constant (a.groups == GRC).
template <class S, int L, int MODE, bool PROF = false, int NW = 4, bool GRP = false, bool CE = false, int GRC = 0>
__global__ __launch_bounds__(64 * NW)
__attribute__((amdgpu_waves_per_eu(lanes_wpe<NW, GRP>, lanes_wpe<NW, GRP>)))
void mlp_train_lanes_kernel(DtpTrainArgs a) {
  using SC = Scal<S>;
  using C = LaneCfg<S, L>;
  constexpr int NTH = 64 * NW;                 // threads of the workgroup
  constexpr int NPT = (S::P + NTH - 1) / NTH;  // parameters owned per thread (optimizer, exchange)
  constexpr int NL = S::NL, P = S::P, NT = SC::NT, NO = C::NO, TS = C::TS, H = S::H;
  // MODE: an update DtpTrainMode, | kModeClip for its clip twin (clip_core.h)
  constexpr int kMode = mode_base(MODE);
  constexpr bool kClip = mode_clip(MODE);
  // | kModeAccum for its accumulation twin (accum_core.h): a.accum micro-batches per optimizer
  // step, clipping behind a run-time branch
  constexpr bool kAccum = mode_accum(MODE);
  static_assert(!kAccum || (NW == 4 && !PROF && !kClip), "accumulation twins: the 4-wave instances; they clip at run time");
  constexpr bool kXgmi = kMode == DTP_MODE_XGMI_ADAM || kMode == DTP_MODE_XGMI_SGD;
  constexpr bool kAdam = kMode == DTP_MODE_ADAM || kMode == DTP_MODE_XGMI_ADAM;
  static_assert(kMode != DTP_MODE_GRAD, "the lanes step serves the optimizer modes");
  static_assert(!kClip || (NW == 4 && !PROF), "clip twins: the 4-wave instances");
  // GRP with kXgmi: ONE flat exchange over world x groups members (xgmi_core.h)
  static_assert(!CE || S::OUT >= 2, "cross-entropy needs >= 2 classes");
  constexpr int YD = CE ? 1 : S::OUT;  // target floats per sample (a class id for CE)
  // the 3-float cross-GPU exchange (xgmi_core.h:xgmi_allreduce_g3), 4-wave instances (the
  // 8-wave ones keep the 2-float owner-thread exchange: their LDS is full)
  constexpr bool kXg3 = NW == 4 && kXgmi;
  // the split-batch members park their dW sums in payload-order rows; the on-chip exchange
  // publishes straight from them and forms the own sums inside (grp_core.h)
  constexpr bool kRows = GRP;
  constexpr bool kRowsPub = kRows && !kXgmi;
  static_assert(!kRows || lane_row_map_ok<S>(), "tile cells -> payload floats: a bijection onto [0, P]");
  static_assert(GRC == 0 || (GRP && !kXgmi && GRC >= 2 && GRC <= kGrpMax), "a constant member count: on-chip exchange");
  // the per-step tail of the on-chip split-batch instances with fewer instructions on the
  // serial path behind the backward (one wave per SIMD: every instruction is an issue slot):
  // the same floating-point operations in the same order, the same loads, stores and barriers
  constexpr bool kDiet = GRP && !kXgmi;
  constexpr int kLossPos = kRows ? grp_row_pos(P) : SC::losspos();  // a wave's loss in sm.red[wave]
  using Smem = LaneSmem<S, L, NW, GRP || kXg3, kRows>;
  __shared__ __align__(16) Smem sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int model = GRP ? (int)(blockIdx.x & 7u) : (int)blockIdx.x;
  const int gk = GRP ? (int)(blockIdx.x >> 3) : 0;  // member of the model's group
  if (GRP && (model >= a.n_models || gk >= a.groups)) return;  // grid = 8 x groups blocks
  const bool lead = gk == 0;                // the member that writes the state back
  const int part = lane & (L - 1);          // this lane's slice of every hidden layer
  const int ws = lane / L;                  // sample slot inside the wave
  const int bk = gk * (NW * C::G) + wave * C::G + ws;  // batch position of this lane's sample
  const GrpCtx gctx{a.grp_buf, a.grp_status, a.groups, gk, a.n_models, a.timeout_us};
  if constexpr (PROF) {  // placement of this block: XCC id (slot 12) and HW_ID (13) of step 0's row
    if (tid == 0) {
      unsigned xcc, hwid;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
      unsigned long long* pr = reinterpret_cast<unsigned long long*>(a.status) + (size_t)blockIdx.x * 8 * 32;
      pr[12] = xcc;
      pr[13] = hwid;
    }
  }
  unsigned long long* prof = reinterpret_cast<unsigned long long*>(a.status);
  const float slope = a.hp.slope;
  // PROF: launch-level stamps in row 0 of this block (thread 0): 20 entry, 18 prologue LDS
  // fills issued, 19 first barrier (global loads consumed), 22 weight scatter, 23 Adam table,
  // 29 loop start, 24 loop end, 21 write-back issued (the lead)
  auto stamp_launch = [&](int slot) {
    if constexpr (PROF) {
      if (tid == 0) {
        unsigned long long t_;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
        __builtin_amdgcn_sched_barrier(0);
        prof[(size_t)blockIdx.x * 8 * 32 + slot] = t_;
      }
    }
  };
  stamp_launch(20);

  // ---- prologue (all global reads issued before the first wait, as in mlp_train_kernel)
  float* __restrict__ gp = a.params + (size_t)model * P;
  const SamplerCfg smp = a.smp;
  int pf[NPT], pb[NPT], tp[NPT];
  float pw[NPT], mr[NPT], vr[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int p = NPT * tid + k;  // blocked ownership in torch order (the exchanges' payload index)
    const bool own = p < P;
    lane_pos<C, S>(own ? p : 0, pf[k], pb[k], tp[k]);
    if constexpr (kRows) tp[k] = own ? grp_row_pos(p) : 0;  // its sums come from the rows
    pw[k] = own ? gp[p] : 0.f;
    mr[k] = own ? a.opt_m[(size_t)model * P + p] : 0.f;
    vr[k] = (kAdam && own) ? a.opt_v[(size_t)model * P + p] : 0.f;
  }
  // row layout: where each of this lane's 4 NT accumulator elements is parked (its payload
  // float's place in the wave's row, or the lane's sink float), fixed for the launch
  int rp[kRows ? NT : 1][4];
  if constexpr (kRows) {
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int f = lane_row_slot<S>(tt, 4 * (lane >> 4) + e, lane & 15);
        // bf16 MFMA tiles: the loss cell saw bf16-truncated values, the wave's fp32 loss is written instead
        const bool real = f >= 0 && !(S::BF && DTP_LANES_BFMMA && f == P);
        rp[tt][e] = real ? grp_row_pos(f) : Smem::RSINK + lane;
      }
    }
  }
  const int t0 = a.host_t0 >= 0 ? a.host_t0 : a.step[model];
  // a schedule always comes as a host table, SGD's rows {lr_t, 1} (see mlp_train_kernel)
  const bool ltab = !kAdam && a.adam_tab && a.hp.lr_tab;
  const bool htab = (kAdam && a.adam_tab && a.host_t0 >= 0) || ltab;
  float2 tabv[kAdamTab / NTH];
  if (htab) adam_tab_load<kAdamTab / NTH, NTH>(a, t0, 0, tid, tabv);
  // accumulation twin: nacc micro-batches per optimizer step; the data position counts
  // micro-steps (t0 * nacc), everything indexed by `it` or t0 stays per optimizer step
  const int nacc = kAccum ? max(a.accum, 1) : 1;
  const int tm0 = kAccum ? t0 * nacc : t0;
  int epoch = tm0 / smp.steps_per_epoch;
  int bi = tm0 - epoch * smp.steps_per_epoch;
  // the sample after next: its permutation word is loaded a whole step before the gather
  // that consumes it, so the word travels raw with `fok` (is this lane's batch position
  // inside that batch?) and the -1 of a position past a ragged batch is formed at the
  // gather -- nothing waits for the load at the end of the step that issued it
  bool fok = true;
  auto fast_index = [&](int ep_, int b_) -> int {
    const int start = b_ * smp.batch;
    const int size = min(smp.batch, smp.num_samples - start);
    int q = smp.rank + (start + bk) * smp.world;
    q = q >= smp.n ? q - smp.n : q;
    q = q < smp.n ? q : smp.n - 1;
    const int di = table_epoch(smp, ep_)[q];
    fok = bk < size;
    return di;
  };
  auto roll = [&](int& ep_, int& b_) {
    const bool r_ = ++b_ == smp.steps_per_epoch;
    b_ = r_ ? 0 : b_;
    ep_ += r_ ? 1 : 0;
  };
  int e2 = epoch, b2 = bi;
  const int fidx0 = fast_index(epoch, bi);
  const bool fok0 = fok;
  roll(e2, b2);
  int fidx = fast_index(e2, b2);
  unsigned xepoch = kXgmi ? a.epoch[model] : (GRP ? a.grp_epoch[model] : 0u);  // GRP + xGMI: the xGMI epochs
  // one model per workgroup: the epoch is the same on every lane (its parity selects the
  // exchange buffer's half through a scalar offset, grp_core.h)
  if constexpr (kDiet) xepoch = (unsigned)__builtin_amdgcn_readfirstlane((int)xepoch);
  // the exchanges' sticky timeout flag, read once per launch with the prologue loads
  const int* xst = kXgmi ? a.status : (GRP ? a.grp_status : nullptr);
  bool xdead = xst ? (__hip_atomic_load(xst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) : false;
  const unsigned xcc = GRP ? grp_xcc_id() : 0u;  // split-batch exchange: plain stores once every member shares it
  bool gplain = false;
  unsigned long long xwait[2] = {0ull, 0ull};
  for (int e = tid; e < C::pad4(C::LW); e += NTH) sm.wb[e] = 0.f;
  // the dataset (inputs then targets) straight into LDS (LDS-DMA; the first barrier waits)
  lds_dma_fill2<NTH>(sm.data, a.X, smp.n * S::IN, a.Y, smp.n * YD, tid);
  const int yoff = smp.n * S::IN;
  stamp_launch(18);
  // this wave's staging areas: zero (unwritten rows / columns stay finite), then the
  // constant-1 bias columns of every tile, written once per launch
  {
    float* s0 = &sm.stg[wave][0][0];
    for (int e = lane; e < lane_areas<S>() * 2 * C::AREA; e += kWave) s0[e] = 0.f;
    static_for<0, NL>([&](auto LC) {
      constexpr int l = decltype(LC)::value;
      constexpr int col = SC::coloff(l) + S::din(l);
      float* hb = &sm.stg[wave][lane_area<S>(l)][C::AREA];
      for (int e = lane; e < 4 * TS; e += kWave) hb[(e / TS) * C::QS + col * TS + e % TS] = 1.f;
    });
  }
  __syncthreads();  // weight blocks zeroed (pads stay 0) before the owners scatter into them
  stamp_launch(19);
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    if (NPT * tid + k < P) {
      const float wv = S::rnd(pw[k]);  // bf16 compute: the matmul operand is the bf16 weight
      sm.wb[pf[k]] = wv;
      if (pb[k] >= 0) sm.wb[pb[k]] = wv;
    }
  }
  stamp_launch(22);
  // kDiet: where the weight scatter after the optimizer writes, as float offsets into sm,
  // fixed for the launch: the parameter's forward and backward copies, or the sink
  // floats for a slot this thread does not own (the last owner of an odd P owns one of two)
  // or a parameter without a backward copy
  constexpr int kSinkOff = (int)(offsetof(Smem, sink) / sizeof(float));
  static_assert(offsetof(Smem, wb) == 0, "the scatter offsets count from sm.wb");
  int wo[NPT][2];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const bool own = NPT * tid + k < P;
    wo[k][0] = own ? pf[k] : kSinkOff;
    wo[k][1] = own && pb[k] >= 0 ? pb[k] : kSinkOff + 1;
  }
  int lslot = a.loss_log ? t0 % a.loss_log_cap : 0;
  // kDiet: the loss log as a running element offset (lslot * n_models + model,
  // advanced by n_models per step, wrapped at the ring's end), one per-launch predicate for
  // its store, and the Adam table's refill counted down
  const bool llog = tid == ((kXgmi || GRP) ? xgmi_loss_tid<NPT>(P, NTH) : 0) && a.loss_log && lead;
  const int lend = a.loss_log ? a.loss_log_cap * a.n_models : a.n_models;
  int loff = lslot * a.n_models + model;
  int refill = kAdamTab;
  auto fast_gather = [&](int di, bool ok, float (&x)[S::IN], float (&y)[S::OUT]) {
    di = ok ? di : -1;
    const bool v = di >= 0;
    di = (unsigned)di < (unsigned)smp.n ? di : 0;
    static_for<0, S::IN>([&](auto IC) {
      constexpr int i = decltype(IC)::value;
      const float t_ = S::rnd(sm.data[di * S::IN + i]);
      x[i] = v ? t_ : 0.f;
    });
    static_for<0, S::OUT>([&](auto JC) {
      constexpr int j = decltype(JC)::value;
      const float t_ = j < YD ? sm.data[yoff + di * YD + j] : 0.f;
      y[j] = v ? t_ : 0.f;
    });
    return v;
  };
  float nx[S::IN], ny[S::OUT];
  bool nvalid = fast_gather(fidx0, fok0, nx, ny);
  auto fill_adam = [&](int base) {
    const int n = min(kAdamTab, a.n_steps - base);
    if (htab) {
      float2 v[kAdamTab / NTH];
      if (base) adam_tab_load<kAdamTab / NTH, NTH>(a, t0, base, tid, v);
      adam_tab_store<kAdamTab / NTH, NTH>(sm.adam_tab, n, tid, base ? v : tabv);
      return;
    }
    for (int e = tid; e < n; e += NTH) {
      const uint64_t t1 = (uint64_t)t0 + (uint64_t)base + (uint64_t)e + 1u;
      const double bc1 = 1.0 - pow_int(a.hp.beta1, t1), bc2 = 1.0 - pow_int(a.hp.beta2, t1);
      sm.adam_tab[e] = make_float2((float)(a.hp.lr / bc1), (float)sqrt(bc2));
    }
  };
  if (kAdam || ltab) fill_adam(0);
  stamp_launch(23);
  // per-lane LDS bases: the part's slice of the partitioned blocks, the sample's slot in a
  // staged operand (+ the part's first column), the MFMA reader's operands
  const float* const wlp = sm.wb + part * C::NOP;
  const int wslot = (ws & 3) * C::QS + (ws >> 2);
  const int wpart = wslot + part * NO * TS;
  const int rdoff = (lane >> 4) * C::QS + (lane & 15) * TS;
  // is slot k of this lane's slice a real unit (k*L + part < H)?
  auto slot_ok = [&](int k) { return C::EXACT || part * NO + k < H; };
  // A staging write of a lane with nothing to stage (a padding slot, a part other than 0
  // for the per-sample rows) goes to row / column 15 of its sample slot when no tile uses
  // it -- D[15][*] and D[*][15] are never read -- so the writes are branch-free
  constexpr bool kSink = H <= 14 && SC::lossrow() <= 14 && (!SC::PACK || S::IN + 1 + H <= 14);
  auto put = [&](float* tl, int area, int off, bool ok, float v) {
    if constexpr (kSink) {
      tl[area + (ok ? off : wslot + 15 * TS)] = v;
    } else {
      if (ok) tl[area + off] = v;
    }
  };
  const bool p0 = part == 0;
  // 1 / (batch size [x OUT]): a batch is full or the epoch's ragged last one, so the two
  // reciprocals are divided once per launch and a step selects by its batch index
  auto inv_of = [&](int b_) {
    const int bsz = min(smp.batch, smp.num_samples - b_ * smp.batch);
    return CE ? 1.f / (float)bsz : 1.f / (float)(bsz * S::OUT);
  };
  const int blast = smp.steps_per_epoch - 1;
  // (pinned in registers by an empty asm: otherwise the select of two quotients is folded
  // into the quotient of a select, back inside the loop)
  float inv_full = inv_of(0), inv_last = inv_of(blast);
  asm volatile("" : "+v"(inv_full), "+v"(inv_last));
  [[maybe_unused]] float gnorm = 0.f;  // clip twin: the last step's norm before clipping
  __syncthreads();
  stamp_launch(29);

  for (int it = 0; it < a.n_steps; ++it) {
    DTP_STAMP(0);
    f32x4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // C::CHAIN: the second K-split accumulator of every hidden tile, added to the first at the
    // park: an add behind a layer's last MFMA would wait for it on the input-gradient chain
    constexpr bool kChain = C::CHAIN;
    f32x4 acc1[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc1[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // park tile tt of this wave (a hidden tile: the sum of its two accumulators)
    auto park = [&](auto TC) {
      constexpr int tt = decltype(TC)::value;
      f32x4 v = acc[tt];
      if constexpr (kChain && tt >= 1 && tt <= NL - 2) v = acc[tt] + acc1[tt];  // tile(l) = l there
      if constexpr (kRows) {  // payload order: every element to its parameter's float (or the sink)
#pragma unroll
        for (int e = 0; e < 4; ++e) sm.red[wave][rp[tt][e]] = v[e];
      } else {
        *reinterpret_cast<f32x4*>(&sm.red[wave][tt * SC::TSZ + SC::tslot(4 * (lane >> 4), lane & 15)]) = v;
      }
    };
    // accumulation twin: the sample of the window's next micro-batch and the index of the one
    // after it (next_sample below without the loss log's slot, which counts optimizer steps)
    auto next_micro = [&]() {
      roll(epoch, bi);
      nvalid = fast_gather(fidx, fok, nx, ny);
      roll(e2, b2);
      fidx = fast_index(e2, b2);
    };
    float inv, lpart;
    [[maybe_unused]] float lacc = 0.f;  // twin, bf16 MFMA tiles: this lane's scaled losses of the window
    [[maybe_unused]] int mic = 0;       // twin: micro-batch of the window
    // one pass per micro-batch of the window (one, but in an accumulation twin): forward, loss
    // and backward into acc / acc1, which are zeroed once per optimizer step
    do {
    inv = bi == blast ? inv_last : inv_full;
    const bool lastm = !kAccum || ++mic >= nacc;  // wave-uniform: the step's tail follows this pass
    const bool valid = nvalid;
    LaneAct<C> st;
    static_for<0, S::IN>([&](auto IC) { st.hin[decltype(IC)::value] = nx[decltype(IC)::value]; });
    float x0[S::IN];
    static_for<0, S::IN>([&](auto IC) { x0[decltype(IC)::value] = nx[decltype(IC)::value]; });

    // ---------------- forward
    LLast<C> last;
    LBBlk<C, NL - 1> bt;
    LBBlk<C, NL - 2> bt2;
    float out[16];
    {
      LFBlk<C, 0> b0;
      b0.template load<0, LFBlk<C, 0>::NR>(sm.wb, wlp);
      DTP_STAMP(1);
      lane_forward<C, 0>(sm.wb, wlp, b0, st, slope, last, bt, bt2, out);
    }
    // ---------------- loss (MSE) -> output gradient (every lane of the sample)
    float dzl[S::OUT];
    lpart = 0.f;
    if constexpr (!CE) {
      static_for<0, S::OUT>([&](auto JC) {
        constexpr int j = decltype(JC)::value;
        const float d = out[j] - ny[j];
        lpart = valid ? fmaf(d, d, lpart) : lpart;
        dzl[j] = valid ? S::rnd(2.f * d * inv) : 0.f;
      });
    } else {  // the one-lane kernel's CE arithmetic (mlp_train_kernel), per lane
      const int cls = valid ? (int)ny[0] : 0;
      float mx = out[0];
      static_for<1, S::OUT>([&](auto JC) { mx = fmaxf(mx, out[decltype(JC)::value]); });
      float se = 0.f, zc = 0.f, ex[S::OUT];  // each exponential once (the same bits as twice)
      static_for<0, S::OUT>([&](auto JC) {
        constexpr int j = decltype(JC)::value;
        ex[j] = __expf(out[j] - mx);
        se += ex[j];
        zc = (j == cls) ? out[j] : zc;
      });
      const float lse = mx + __logf(se);
      const float rs = 1.f / se;
      lpart = valid ? lse - zc : 0.f;
      static_for<0, S::OUT>([&](auto JC) {
        constexpr int j = decltype(JC)::value;
        dzl[j] = valid ? S::rnd((ex[j] * rs - (j == cls ? 1.f : 0.f)) * inv) : 0.f;
      });
    }
    DTP_STAMP(2);
    // accumulation twin: the loss cell sums lpart * inv over the window -- every micro-batch by
    // its own size -- so it holds the sum of the window's mean losses
    const float lstage = kAccum ? lpart * inv : lpart;
    if constexpr (kAccum && S::BF && DTP_LANES_BFMMA) lacc += p0 ? lstage : 0.f;

    // ---------------- backward
    float dzp[C::NOP];  // this lane's slice of the current layer's output gradient
    {  // last layer: stage (dz, loss, own slice of its input), input-gradient slice
      constexpr int l = NL - 1;
      float* tl = &sm.stg[wave][lane_area<S>(l)][0];
      static_for<0, S::OUT>([&](auto JC) {
        put(tl, 0, wslot + (SC::rowoff(l) + decltype(JC)::value) * TS, p0, dzl[decltype(JC)::value]);
      });
      put(tl, 0, wslot + SC::lossrow() * TS, p0, lstage);
      static_for<0, NO>([&](auto KC) {
        constexpr int k = decltype(KC)::value;
        put(tl, C::AREA, wpart + (SC::coloff(l) + k) * TS, slot_ok(k), st.own[l - 1][k]);
      });
      f32x2 g[C::NPR];
      static_for<0, C::NPR>([&](auto RC) { g[decltype(RC)::value] = f32x2{0.f, 0.f}; });
      static_for<0, S::OUT>([&](auto OC) {
        constexpr int o = decltype(OC)::value;
        const f32x2 d = f32x2{dzl[o], dzl[o]};
        static_for<0, C::NPR>([&](auto RC) {
          constexpr int r = decltype(RC)::value;
          g[r] = __builtin_elementwise_fma(quad_pair<r % 2>(bt.w[o][r / 2]), d, g[r]);
        });
      });
      static_for<0, NO>([&](auto KC) {
        constexpr int k = decltype(KC)::value;
        const float v = S::rnd((k & 1) ? g[k / 2].y : g[k / 2].x);
        dzp[k] = S::rnd(v * leaky_grad_from_out(st.own[l - 1][k], slope));
      });
      if constexpr (!SC::PACK) {
        __builtin_amdgcn_wave_barrier();
        const auto to = lane_tile_ops<C>(tl, rdoff);
        acc[SC::tile(l)] = lane_tile<C, S>(to, acc[SC::tile(l)]);
      }
    }
    // hidden layers NL-2 .. 1: block B of layer l in registers, block l-1 prefetched
    auto hidden = [&](auto LC, const auto& B, auto& nb) {
      constexpr int l = decltype(LC)::value;
      float* tl = &sm.stg[wave][lane_area<S>(l)][0];
      // the previous layer's MFMA operand reads of this area were issued before these writes
      __builtin_amdgcn_sched_barrier(0);
      static_for<0, NO>([&](auto KC) {
        constexpr int k = decltype(KC)::value;
        put(tl, 0, wpart + (SC::rowoff(l) + k) * TS, slot_ok(k), dzp[k]);
        put(tl, C::AREA, wpart + (SC::coloff(l) + k) * TS, slot_ok(k), st.own[l - 1][k]);
      });
      __builtin_amdgcn_wave_barrier();
      const auto to = lane_tile_ops<C>(tl, rdoff);
      float dzf[16];
      static_for<0, C::L>([&](auto PC) {
        constexpr int pp = decltype(PC)::value;
        static_for<0, NO>([&](auto KC) {
          constexpr int k = decltype(KC)::value;
          if constexpr (pp * NO + k < H) dzf[pp * NO + k] = part_bcast<C::L, pp>(dzp[k]);
        });
      });
      f32x2 g[C::NPR];
      static_for<0, C::NPR>([&](auto RC) { g[decltype(RC)::value] = f32x2{0.f, 0.f}; });
      f32x4 a0 = acc[SC::tile(l)], a1 = f32x4{0.f, 0.f, 0.f, 0.f};
      // accumulation twin: the second accumulator carries the window's earlier micro-batches too
      if constexpr (kAccum && kChain) a1 = acc1[SC::tile(l)];
      constexpr int J0 = 2;
      LNone none;
      static_for<0, H>([&](auto OC) {
        constexpr int o = decltype(OC)::value;
        if constexpr (S::BF && DTP_LANES_BFMMA) {  // the whole tile on one bf16 MFMA
          if constexpr (o == J0) a0 = lane_tile_bf<C>(to, a0);
        } else if constexpr (o >= J0) {
          constexpr int k0 = TS * (o - J0) / (H - J0), k1 = TS * (o - J0 + 1) / (H - J0);
          static_for<k0, k1>([&](auto KC) { lane_kstep<decltype(KC)::value>(to, a0, a1); });
        }
        const f32x2 d = f32x2{dzf[o], dzf[o]};
        static_for<0, C::NPR>([&](auto RC) {
          constexpr int r = decltype(RC)::value;
          g[r] = __builtin_elementwise_fma(quad_pair<r % 2>(B.w[o][r / 2]), d, g[r]);
        });
        __builtin_amdgcn_sched_barrier(0);
        lchunk<o, H>(sm.wb, wlp, nb, none);
        __builtin_amdgcn_sched_barrier(0);
      });
      if constexpr (kChain) {
        acc[SC::tile(l)] = a0;
        acc1[SC::tile(l)] = a1;
      } else {
        acc[SC::tile(l)] = a0 + a1;
      }
      static_for<0, NO>([&](auto KC) {
        constexpr int k = decltype(KC)::value;
        const float v = S::rnd((k & 1) ? g[k / 2].y : g[k / 2].x);
        dzp[k] = S::rnd(v * leaky_grad_from_out(st.own[l - 1][k], slope));
      });
    };
    auto hidden_rest = [&](auto self, auto LC, const auto& B) -> void {
      constexpr int l = decltype(LC)::value;
      if constexpr (l > 1) {
        LBBlk<C, l - 1> nb;
        hidden(LC, B, nb);
        self(self, std::integral_constant<int, l - 1>{}, nb);
      } else {
        LNone none;
        hidden(LC, B, none);
      }
    };
    hidden_rest(hidden_rest, std::integral_constant<int, NL - 2>{}, bt2);
    {  // layer 0: its dW tile only (packed with the last layer's when they fit)
      float* tl = &sm.stg[wave][lane_area<S>(0)][0];
      static_for<0, NO>([&](auto KC) {
        constexpr int k = decltype(KC)::value;
        put(tl, 0, wpart + (SC::rowoff(0) + k) * TS, slot_ok(k), dzp[k]);
      });
      static_for<0, S::IN>([&](auto IC) {
        put(tl, C::AREA, wslot + (SC::coloff(0) + decltype(IC)::value) * TS, p0, x0[decltype(IC)::value]);
      });
      __builtin_amdgcn_wave_barrier();
      const auto to = lane_tile_ops<C>(tl, rdoff);
      if constexpr (kChain && !kAccum) {
        // every other tile is final: parked while this one's operands travel and its MFMAs run
        // (no write moves into a chain; the wave has nothing else to issue here)
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, NT>([&](auto TC) {
          if constexpr (decltype(TC)::value != SC::tile(0)) park(TC);
        });
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (kChain && kAccum) {  // the same, on the window's last micro-batch only
        if (lastm) {
          static_for<0, NT>([&](auto TC) {
            if constexpr (decltype(TC)::value != SC::tile(0)) park(TC);
          });
        }
      }
      acc[SC::tile(0)] = lane_tile<C, S>(to, acc[SC::tile(0)]);
    }
    if constexpr (kAccum) {
      // not the window's last micro-batch: on to the next one.  No barrier, no park, no LDS
      // write outside this wave's staging areas -- the weights in LDS are the window's
      if (!lastm) {
        next_micro();
        continue;
      }
    }
    break;
    } while (true);
    DTP_STAMP(8 + wave);
    DTP_STAMP(3);
    {
      static_for<0, NT>([&](auto TC) {
        if constexpr (!kChain || decltype(TC)::value == SC::tile(0)) park(TC);
      });
      if constexpr (S::BF && DTP_LANES_BFMMA) {
        // the bf16 MFMA saw the loss row's per-sample values truncated to bf16: the wave's
        // loss goes in from a wave sum of the fp32 values instead (same LDS slot, written after;
        // row layout: the loss cell itself went to the sink)
        // (accumulation twin: of the window's scaled values)
        const float lw = wave_sum(kAccum ? lacc : (p0 ? lpart : 0.f));
        if (lane == 0) sm.red[wave][kLossPos] = lw;
      }
    }
    __syncthreads();
    const float2 adam_sc = (kAdam || ltab) ? sm.adam_tab[it % kAdamTab] : make_float2(0.f, 1.f);
    DTP_STAMP(4);
    float g[NPT];
    float lsum = 0.f;
    // this thread's parameters summed over the waves (and the loss), in wave order
    auto own_sums = [&]() {
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) s += sm.red[ww][tp[k]];
        g[k] = s;
      }
      float ls = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) ls += sm.red[ww][kLossPos];
      lsum = ls;
    };
    // the next step's sample and the index of the one after it (run behind the exchanges)
    const int lslot_now = lslot;
    auto next_sample = [&]() {
      roll(epoch, bi);
      if constexpr (!kDiet) {
        if (a.loss_log && ++lslot == a.loss_log_cap) lslot = 0;
      }
      nvalid = fast_gather(fidx, fok, nx, ny);
      roll(e2, b2);
      fidx = fast_index(e2, b2);
    };
    if constexpr (!kRowsPub) {
      own_sums();
    } else {  // the members' partial sums, on chip (grp_core.h): published from the rows, own_sums
              // runs inside the exchange (wave order: the same bits)
      xepoch += 1u;
      GrpProf gp_;
      lsum = grp_allreduce_rows3<P, NPT, NTH, GRC, NW, Smem::RSTR>(gctx, model, g, lsum, xepoch, tid, xdead,
                                                                   reinterpret_cast<float*>(sm.gx), xcc, gplain,
                                                                   PROF ? &gp_ : nullptr, &sm.red[0][0], own_sums);
      if constexpr (PROF) {  // thread 64, a poller: publish issued (16), first poll consumed (17), last
                             // granule (31), polls (30)
        if (tid == 64 && it < 8) {
          unsigned long long* pr = prof + ((size_t)blockIdx.x * 8 + it) * 32;
          pr[16] = gp_.t_pub;
          pr[17] = gp_.t_first;
          pr[31] = gp_.t_end;
          pr[30] = gp_.polls;
          pr[15] = gp_.rt_end;  // chip-wide clock: this member's last granule
        }
        if (tid == 0 && it < 8)  // the publisher: chip-wide clock when its stores were issued
          prof[((size_t)blockIdx.x * 8 + it) * 32 + 14] = gp_.rt_pub;
      }
    }
    // GRP + xGMI: this member's share of the rank's mean.  Accumulation twin: the sum of the
    // window's mean losses, scaled already; its 1 / nacc is in hp.grad_scale, applied at the log
    const float mean_loss = kAccum ? lsum : lsum * inv;
    DTP_STAMP(5);
    float gloss = mean_loss;
    if constexpr (kXgmi) {
      xepoch += 1u;
      if constexpr (kXg3) {
        const XgmiCtx xc{a.peers, a.status, a.smp.world, a.smp.rank, a.n_models, a.timeout_us};
        gloss = xgmi_allreduce_g3<P, NPT, NTH>(xc, model, g, mean_loss, xepoch, tid, reinterpret_cast<float*>(sm.gx),
                                               xdead, xwait, GRP ? a.groups : 1, gk);
      } else {
        gloss = xgmi_allreduce_model<NPT, NTH>(a, model, P, g, mean_loss, xepoch, tid, xwait, GRP ? a.groups : 1, gk,
                                               &xdead);
      }
    }
    next_sample();
    {
      AdamScalars as = adam_consts(a.hp);
      as.step_size = adam_sc.x;
      as.bc2_sqrt = adam_sc.y;
      if constexpr (kAdam) decoupled_decay_step(a.hp, as, t0 + it, pw);  // AdamW: p *= d_t
      const float lr = ltab ? adam_sc.x : (float)a.hp.lr, mom = (float)a.hp.momentum, wd = (float)a.hp.weight_decay;
      if constexpr (kAccum) {
        // the twin clips behind a run-time branch (block-uniform: it comes from the argument
        // block), as the clip twin does below; off: the plain update's arithmetic
        float x[NPT];
        if (a.max_norm > 0.f || a.clip_value > 0.f) {
          gnorm = clip_gradient<NPT, NW>(a, g, x, P, tid, gnorm);
        } else {
#pragma unroll
          for (int k = 0; k < NPT; ++k) x[k] = g[k] * a.hp.grad_scale;
        }
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          if constexpr (kAdam) adam_update(pw[k], mr[k], vr[k], x[k], as);
          else sgd_update(pw[k], mr[k], x[k], lr, mom, wd, t0 + it == 0);
        }
      } else if constexpr (kClip) {
        // g[] is final here -- summed over waves, members and ranks, the same bits on every
        // member and rank -- so each workgroup clips on its own (clip_core.h).  A slot this
        // thread does not own holds parameter 0's gradient: the norm masks it by index.
        float x[NPT];
        gnorm = clip_gradient<NPT, NW>(a, g, x, P, tid, gnorm);
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          if constexpr (kAdam) adam_update(pw[k], mr[k], vr[k], x[k], as);
          else sgd_update(pw[k], mr[k], x[k], lr, mom, wd, t0 + it == 0);
        }
      } else {
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          if constexpr (kAdam) adam_update(pw[k], mr[k], vr[k], g[k] * a.hp.grad_scale, as);
          else sgd_update(pw[k], mr[k], g[k] * a.hp.grad_scale, lr, mom, wd, t0 + it == 0);
        }
      }
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        const bool own = NPT * tid + k < P;
        const float wv = S::rnd(pw[k]);
        if constexpr (kDiet) {
          float* const smf = reinterpret_cast<float*>(&sm);
          smf[wo[k][0]] = wv;
          smf[wo[k][1]] = wv;
        } else {
          *(own ? &sm.wb[pf[k]] : &sm.sink[0]) = wv;
          *(own && pb[k] >= 0 ? &sm.wb[pb[k]] : &sm.sink[1]) = wv;
        }
      }
    }
    // the thread that holds the summed loss logs it (the loss granule's owner: every other
    // thread of a split-batch member only has its own member's share)
    if constexpr (kDiet) {
      if (llog) a.loss_log[loff] = kAccum ? mean_loss * a.hp.grad_scale : mean_loss;
      loff += a.n_models;
      loff = loff >= lend ? loff - lend : loff;
    } else if (tid == ((kXgmi || GRP) ? xgmi_loss_tid<NPT>(P, NTH) : 0) && a.loss_log && lead) {
      const float lg = kXgmi ? gloss * a.hp.grad_scale : (kAccum ? mean_loss * a.hp.grad_scale : mean_loss);
      a.loss_log[(size_t)lslot_now * a.n_models + model] = lg;
    }
    DTP_STAMP(6);
    __syncthreads();
    if constexpr (kDiet) {
      if ((kAdam || ltab) && --refill == 0 && it + 1 < a.n_steps) {
        refill = kAdamTab;
        fill_adam(it + 1);
        // the refill's predicated table loads are all consumed here, once per kAdamTab steps:
        // none counts as outstanding where this path rejoins the step, whose end would
        // otherwise wait for every load in flight, the next-but-one sample's index included
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        __syncthreads();
      }
    } else if ((kAdam || ltab) && (it + 1) % kAdamTab == 0 && it + 1 < a.n_steps) {
      fill_adam(it + 1);
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), as above
      __syncthreads();
    }
    DTP_STAMP(7);
  }

  stamp_launch(24);
  if constexpr (GRP || kXgmi) {
    // a launch whose exchange timed out on any thread keeps the state from before it (what
    // it summed is incomplete; check_comm raises on the status word), so a checkpoint or a
    // resume never sees it -- one barrier per launch
    if (__syncthreads_or(xdead ? 1 : 0)) return;
  }
  if (!lead) return;  // every member holds the same state: the first writes it back
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int p = NPT * tid + k;
    if (p < P) {
      gp[p] = pw[k];
      a.opt_m[(size_t)model * P + p] = mr[k];
      if (kAdam) a.opt_v[(size_t)model * P + p] = vr[k];
    }
  }
  if (tid == 0) a.step[model] = t0 + a.n_steps;
  if constexpr (kClip || kAccum) {
    if (tid == 0 && a.max_norm > 0.f && a.norm_out) a.norm_out[model] = gnorm;
  }
  if (kXgmi && tid == 0) a.epoch[model] = xepoch;
  if (GRP && !kXgmi && tid == 0) a.grp_epoch[model] = xepoch;
  if (kXgmi && model == 0 && a.status) xgmi_record_wait(a.status, xwait, (unsigned long long)a.n_steps, tid);
  stamp_launch(21);
}

// ------------------------------------------------------------------------------
// The families.  (IN, H, NL, OUT, bf16 compute, CE head, SGD, 8-wave, split-batch, A/B and PROF
// extras): a family has L = 2 and 4, local and xGMI, of its optimizer, in every step variant:
// the plain step, and the clip twin (clip_core.h) and accumulation twin (accum_core.h) of each
// of its 4-wave instances, the split-batch ones included.
#define DTP_LANES_FAMILIES(X)                                                                         \
  X(2, 10, 5, 1, false, false, false, true, true, true)    /* the flagship: toy model, Adam + MSE */  \
  X(2, 10, 5, 1, false, false, true, false, true, false)   /* toy, SGD */                             \
  X(2, 10, 5, 1, true, false, false, false, true, false)   /* toy, bf16 compute */                    \
  X(2, 10, 5, 4, false, true, false, false, true, false)   /* the CE head */                          \
  X(2, 10, 5, 4, false, true, true, false, true, false)                                               \
  X(2, 10, 3, 1, false, false, false, false, false, false) /* the other one-lane shapes, Adam + MSE */ \
  X(2, 10, 5, 4, false, false, false, false, false, false)                                            \
  X(2, 15, 5, 1, false, false, false, false, false, false)

// split-batch step (GRP): member k of model m is block m + 8 k (blocks of absent models exit)
template <class S, int L, int MODE, int NW, bool CE, bool PROF = false, bool GRP = false, int GRC = 0>
void launch_lanes(const DtpTrainArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((mlp_train_lanes_kernel<S, L, MODE, PROF, NW, GRP, CE, GRC>),
                     dim3(GRP ? 8 * a.groups : a.n_models), dim3(64 * NW), 0, st, a);
}

// variant V of a family's 4-wave instances into its row: MODE carries the variant's bit
template <class S, bool CE, bool SGD, bool GRP, StepVariant V>
constexpr void lanes_fill(LanesInst& r) {
  constexpr int BIT = V == kClip ? kModeClip : (V == kAccum ? kModeAccum : 0);
  constexpr int M = (SGD ? DTP_MODE_SGD : DTP_MODE_ADAM) | BIT;
  constexpr int XM = (SGD ? DTP_MODE_XGMI_SGD : DTP_MODE_XGMI_ADAM) | BIT;
  r.lanes[V][0][0][0] = &launch_lanes<S, 2, M, 4, CE>, r.lanes[V][0][0][1] = &launch_lanes<S, 2, XM, 4, CE>;
  r.lanes[V][0][1][0] = &launch_lanes<S, 4, M, 4, CE>, r.lanes[V][0][1][1] = &launch_lanes<S, 4, XM, 4, CE>;
  if constexpr (GRP) {
    // 4 members (batch 256 on one rank) have the count as a constant
    r.grp[V][0] = &launch_lanes<S, 4, M, 4, CE, false, true>;
    r.grp[V][1] = &launch_lanes<S, 4, M, 4, CE, false, true, 4>;
    r.grp[V][2] = &launch_lanes<S, 4, XM, 4, CE, false, true>;
  }
}

// variant V of every family, into the table's rows (in DTP_LANES_FAMILIES order)
template <StepVariant V>
void lanes_fill_families(LanesInst* rows) {
#define X(I, H, N, O, B, CE, SGD, W8, GRP, EXTRA) lanes_fill<Stage<I, H, N, O, false, B>, CE, SGD, GRP, V>(*rows++);
  DTP_LANES_FAMILIES(X)
#undef X
}
// the twins' sources (mlp_train_lanes_clip.hip, mlp_train_lanes_accum.hip)
void lanes_fill_clip(LanesInst* rows);
void lanes_fill_accum(LanesInst* rows);

}  // namespace dtp

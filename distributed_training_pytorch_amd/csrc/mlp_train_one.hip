// The fused train step, one lane per sample, for gfx950 (MI355X), and its instance table.
//
//   mlp_train_kernel : one workgroup per model (the reference trains two independent
//                      ToyModels per iteration, demo.py:104-111), device-side sampler ->
//                      gather -> forward -> MSE/CE -> backward (MFMA weight-gradient
//                      reduction) -> optimizer, optionally for n_steps iterations inside
//                      one launch with weights, dataset and optimizer state resident in
//                      LDS / registers (no launch boundary per step).
//   kOne             : the (shape, precision) pairs it is instantiated for; one_lane_inst()
//                      is the lookup mlp_train.hip dispatches through.
#include "mlp_train_common.h"
#include "mlp_pipe.h"
#include "mlp_scalar.h"
#include "optim_core.h"
#include "clip_core.h"
#include "xgmi_core.h"

namespace dtp {

constexpr int kWaves = kBlock / kWave;

template <class S>
struct TrainSmem {
  float wb[Scal<S>::LW];  // backward + forward weight blocks (mlp_scalar.h)
  float2 adam_tab[kAdamTab];  // per-step Adam scalars {lr / (1 - b1^t), sqrt(1 - b2^t)}
  // per wave: [packed first/last tile | hidden layer] x (dz rows, h rows) -- one hidden
  // buffer suffices: a wave's LDS ops execute in order, so layer l-1's staging
  // writes land after layer l's operand reads were issued; reused for the
  // cross-wave dW tile reduction
  float stage[kWaves][2][2 * kStgArr];
  float data[kDataCache];
  float sink[4];  // target of the optimizer's predicated-off stores (slots past P)
  float lossw[kBlock / kWave];  // bf16 instances: per-wave batch-loss sums (not through a bf16 tile)
  // unused (what an xGMI exchange with LDS staging left behind): 16 bytes of every instance's
  // LDS size, kept until a change that may alter the kernels' descriptors
  alignas(16) float2 xg_stub[2];
};

// One lane's sample of a step: input, target (class index for CE) and validity.
template <class S>
struct SampleRegs {
  float x[S::IN];
  float y[S::OUT];
  bool valid;
};

// Fused train step(s), one workgroup (4 waves, one lane per sample) per model.
// Weights live in LDS blocks read into registers one layer ahead (mlp_pipe.h),
// activations in VGPRs, the dW reduction over the batch runs on MFMA through a per-wave
// LDS staging area, the optimizer owns NPT parameters per thread in registers (params
// and moments).  One wave per SIMD (amdgpu_waves_per_eu(1, 1)): the scheduler may spend
// registers on latency.
// FAST: the common configuration fixed at compile time (MSE, batch <= 256, the
// SAMPLER_TABLE sampler -- the epoch permutations in a device ring the host fills
// ahead, torch's exact DistributedSampler order by default --, dataset cached in LDS,
// 0 <= slope <= 1; fast_path_ok() on the host): each lane's dataset index is loaded
// from the ring a whole step before it is used, so the next step's sample gather
// is straight-line LDS code the scheduler interleaves with the optimizer, and
// LeakyReLU is max(z, slope z).
template <class S, int MODE, bool PROF = false, bool FAST = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 1))) void mlp_train_kernel(DtpTrainArgs a) {
  using SC = Scal<S>;
  constexpr int NL = S::NL, P = S::P, NT = SC::NT, NPT = S::NPT;
  static_assert(NT * SC::TSZ <= 2 * 2 * kStgArr, "a wave's reduction tiles must fit in its staging area");
  static_assert(NL >= 3, "the pipelined forward / backward (mlp_pipe.h) keeps two layers in flight");
  __shared__ __align__(16) TrainSmem<S> sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int model = blockIdx.x;
  // MODE: a DtpTrainMode, | kModeClip for the clip twin of an update mode (clip_core.h)
  constexpr int kMode = mode_base(MODE);
  constexpr bool kClip = mode_clip(MODE);
  constexpr bool kUpdate = kMode != DTP_MODE_GRAD;
  constexpr bool kAdam = kMode == DTP_MODE_ADAM || kMode == DTP_MODE_XGMI_ADAM;
  constexpr bool kXgmi = kMode == DTP_MODE_XGMI_ADAM || kMode == DTP_MODE_XGMI_SGD;
  static_assert(!kClip || (kUpdate && !PROF && !FAST), "clip twins: the generic update instances");
  unsigned long long* prof = reinterpret_cast<unsigned long long*>(a.status);
  // PROF: kernel entry and exit stamps of the launch (slots 20 and 21 of iteration 0)
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
  const bool ce = !FAST && a.loss == DTP_LOSS_CE;  // FAST: MSE
  const int ydim = ce ? 1 : S::OUT;
  const float slope = a.hp.slope;

  // ---- setup. Every global read of the prologue (owned params and moments, step
  // and exchange counters, the dataset) is issued before the first wait, so a
  // launch pays ONE memory round trip before its first step, not three.
  float* __restrict__ gp = a.params + (size_t)model * P;
  const SamplerCfg smp = a.smp;
  const bool cached = FAST || (a.cache_data && smp.n * (S::IN + ydim) <= kDataCache);
  int pf[NPT], pb[NPT], tp[NPT], pfl[NPT];
  float pw[NPT], mr[NPT], vr[NPT];
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int p = NPT * tid + k;  // blocked ownership: thread t holds parameters NPT t .. NPT t + NPT-1
    scal_pos<S>(p < P ? p : 0, pf[k], pb[k], tp[k], pfl[k]);
    const bool own = p < P;
    pw[k] = own ? gp[p] : 0.f;
    mr[k] = (kUpdate && own) ? a.opt_m[(size_t)model * P + p] : 0.f;
    vr[k] = (kAdam && own) ? a.opt_v[(size_t)model * P + p] : 0.f;
  }
  // the step number: from the host when it knows it (the persistent engine), so the
  // first dataset indices can be requested without waiting for the counter's load
  const int t0 = a.host_t0 >= 0 ? a.host_t0 : a.step[model];
  // the host's Adam-scalar table (persistent engine): the first kAdamTab entries are
  // loaded with the prologue's other global reads (one memory round trip for all)
  // A learning-rate schedule (hp.lr_tab set) comes as a host table whose rows carry the
  // step's rate -- Adam {lr_t / (1 - b1^t), sqrt(1 - b2^t)}, SGD {lr_t, 1} -- so the Adam
  // instances are the unscheduled kernels to the instruction: a scheduled Adam launch gives
  // host_t0 (dtp_mlp_train refuses it otherwise).  SGD reads its table with t0 from either
  // source; without a schedule it reads hp.lr as before.
  const bool ltab = kUpdate && !kAdam && a.adam_tab && a.hp.lr_tab;
  const bool htab = (kAdam && a.adam_tab && a.host_t0 >= 0) || ltab;
  float2 tabv[kAdamTab / kBlock];
  if (htab) adam_tab_load<kAdamTab / kBlock>(a, t0, 0, tid, tabv);
  // 32-bit step bookkeeping, advanced incrementally (no 64-bit divisions per step)
  const bool explicit_idx = !FAST && smp.mode == SAMPLER_EXPLICIT;
  int epoch = explicit_idx ? 0 : t0 / smp.steps_per_epoch;
  int bi = explicit_idx ? 0 : t0 - epoch * smp.steps_per_epoch;
  // FAST: this lane's dataset index of the step at (ep_, b_): the padded-list position
  // (padding repeats from the start), looked up in the epoch's slot of the ring; -1
  // past the batch.  The load is issued a step ahead of its use (fidx below).
  auto fast_index = [&](int ep_, int b_) -> int {
    const int start = b_ * smp.batch;
    const int size = min(smp.batch, smp.num_samples - start);
    int q = smp.rank + (start + tid) * smp.world;
    q = q >= smp.n ? q - smp.n : q;
    q = q < smp.n ? q : smp.n - 1;  // lanes past the batch: any in-range position
    const int di = table_epoch(smp, ep_)[q];
    return tid < size ? di : -1;
  };
  auto roll = [&](int& ep_, int& b_) {  // advance a (epoch, batch) cursor by one step, branch-free
    const bool r_ = ++b_ == smp.steps_per_epoch;
    b_ = r_ ? 0 : b_;
    ep_ += r_ ? 1 : 0;
  };
  // FAST: the first step's indices and the second step's (in flight across the
  // prologue), and the cursor of the step after the next one to gather
  int e2 = epoch, b2 = bi, fidx0 = 0, fidx = 0;
  if constexpr (FAST) {
    fidx0 = fast_index(epoch, bi);
    roll(e2, b2);
    fidx = fast_index(e2, b2);
  }
  unsigned xepoch = kXgmi ? a.epoch[model] : 0u;
  // the exchanges' sticky timeout flag, read once per launch with the prologue loads
  bool xdead = (kXgmi && a.status) ? (__hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
                                   : false;
  unsigned long long xwait[2] = {0ull, 0ull};  // exchange-wait / publish ticks of this thread (xgmi_record_wait)
  for (int e = tid; e < SC::LW; e += kBlock) sm.wb[e] = 0.f;
  if (cached) {
    for (int e = tid; e < smp.n * S::IN; e += kBlock) sm.data[e] = a.X[e];
    for (int e = tid; e < smp.n * ydim; e += kBlock) sm.data[smp.n * S::IN + e] = a.Y[e];
  }
  stamp_launch(18);
  const float* __restrict__ Xg = a.X;
  const float* __restrict__ Yg = a.Y;
  const int yoff = smp.n * S::IN;
  __syncthreads();  // weight blocks zeroed (pads stay 0) before the owners scatter into them
  stamp_launch(19);
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    if (NPT * tid + k < P) {
      const float wv = S::rnd(pw[k]);  // bf16 compute: the matmul operand is the bf16 weight
      sm.wb[pfl[k]] = wv;
      if (pb[k] >= 0) sm.wb[pb[k]] = wv;
    }
  }
  stamp_launch(22);
  int lslot = a.loss_log ? t0 % a.loss_log_cap : 0;
  uint32_t keys[4];
  epoch_keys(smp, epoch, keys);
  // sample k of step it (batch geometry bp): index (explicit list or the in-kernel
  // Feistel shuffle, sampler.h) -> input and target from the LDS-resident dataset.
  // The next step's first chunk is gathered while the current step's optimizer
  // runs (the sampler depends on nothing the update writes), so a step starts
  // with its inputs already in registers.
  auto gather = [&](int it_, const BatchPos& bp_, const uint32_t (&keys_)[4], int k, int bsz_) {
    SampleRegs<S> r;
    r.valid = k < bsz_;
    int di = 0;
    if (r.valid) di = explicit_idx ? a.idx[(size_t)it_ * smp.batch + k] : sample_index(smp, bp_, keys_, k);
    static_for<0, S::IN>([&](auto IC) {
      constexpr int i = decltype(IC)::value;
      r.x[i] = r.valid ? S::rnd(cached ? sm.data[di * S::IN + i] : Xg[(size_t)di * S::IN + i]) : 0.f;
    });
    static_for<0, S::OUT>([&](auto JC) {
      constexpr int j = decltype(JC)::value;
      float y = 0.f;
      if (r.valid && j < ydim) y = cached ? sm.data[yoff + di * ydim + j] : Yg[(size_t)di * ydim + j];
      r.y[j] = y;
    });
    return r;
  };
  auto batch_at = [&](int ep, int b) {
    BatchPos bp_;
    bp_.epoch = ep;
    bp_.start = b * smp.batch;
    bp_.size = explicit_idx ? smp.batch : min(smp.batch, smp.num_samples - bp_.start);
    return bp_;
  };
  auto fast_gather = [&](int di) {
    SampleRegs<S> r;
    r.valid = di >= 0;
    di = (unsigned)di < (unsigned)smp.n ? di : 0;  // never index LDS out of range
    static_for<0, S::IN>([&](auto IC) {
      constexpr int i = decltype(IC)::value;
      const float v = S::rnd(sm.data[di * S::IN + i]);
      r.x[i] = r.valid ? v : 0.f;
    });
    static_for<0, S::OUT>([&](auto JC) {
      constexpr int j = decltype(JC)::value;
      const float v = j < ydim ? sm.data[yoff + di * ydim + j] : 0.f;
      r.y[j] = r.valid ? v : 0.f;
    });
    return r;
  };
  SampleRegs<S> nxt;
  if constexpr (FAST) {
    nxt = fast_gather(fidx0);  // the first step's samples (the index loads overlapped the prologue)
  } else {
    nxt = gather(0, batch_at(epoch, bi), keys, tid, batch_at(epoch, bi).size);
  }
  // Adam bias-correction powers beta^t, carried in double like torch's host math
  // table entry e holds the scalars of step number t0 + base + e + 1
  auto fill_adam = [&](int base) {
    const int n = min(kAdamTab, a.n_steps - base);  // short launches (eager / graph) fill only what they use
    if (htab) {
      float2 v[kAdamTab / kBlock];
      if (base) adam_tab_load<kAdamTab / kBlock>(a, t0, base, tid, v);
      adam_tab_store<kAdamTab / kBlock>(sm.adam_tab, n, tid, base ? v : tabv);
      return;
    }
    for (int e = tid; e < n; e += kBlock) {
      const uint64_t t1 = (uint64_t)t0 + (uint64_t)base + (uint64_t)e + 1u;
      const double bc1 = 1.0 - pow_int(a.hp.beta1, t1), bc2 = 1.0 - pow_int(a.hp.beta2, t1);
      sm.adam_tab[e] = make_float2((float)(a.hp.lr / bc1), (float)sqrt(bc2));
    }
  };
  if (kAdam || ltab) fill_adam(0);
  stamp_launch(23);
  float* const stg_pack = &sm.stage[wave][0][0];
  [[maybe_unused]] float gnorm = 0.f;  // clip twin: the last step's norm before clipping
  __syncthreads();  // scattered weight blocks and the Adam table visible to every wave
  stamp_launch(29);

  for (int it = 0; it < a.n_steps; ++it) {
    DTP_STAMP(0);
    const int t = t0 + it;
    const BatchPos bp = batch_at(epoch, bi);
    const int bsz = bp.size;
    const float inv = ce ? 1.f / (float)bsz : 1.f / (float)(bsz * S::OUT);

    f32x4 acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    float lacc = 0.f;  // this lane's loss over the step's chunks (bf16 instances)

    // FAST: batch <= kBlock, one chunk (the loop folds away: fwd, loss and bwd are
    // one straight-line region)
    for (int c0 = 0; c0 < (FAST ? kBlock : bsz); c0 += kBlock) {
      const SampleRegs<S> smpl = c0 == 0 ? nxt : gather(it, bp, keys, c0 + tid, bsz);
      const bool valid = smpl.valid;
      float h[NL + 1][16];
      static_for<0, S::IN>([&](auto IC) { h[0][decltype(IC)::value] = smpl.x[decltype(IC)::value]; });
      BBlk<S, NL - 1> pbt;  // backward blocks prefetched by the pipelined forward
      TopB2<S> pbt2;
      {
        FBlk<S, 0> pb0;
        pb0.template load<0, FBlk<S, 0>::NR>(sm.wb);
        if (c0 == 0) DTP_STAMP(1);
        pipe_forward<S, 0, FAST>(sm.wb, pb0, h, slope, pbt, pbt2);
      }

      // ---------------- loss (MSE / CE) -> dz of the last layer
      constexpr int L = NL - 1;
      float dz[16];
      float lpart = 0.f;
      if (!ce) {
        static_for<0, S::OUT>([&](auto JC) {
          constexpr int j = decltype(JC)::value;
          const float d = h[L + 1][j] - smpl.y[j];
          lpart = valid ? fmaf(d, d, lpart) : lpart;
          dz[j] = valid ? S::rnd(2.f * d * inv) : 0.f;
        });
      } else {
        const int cls = valid ? (int)smpl.y[0] : 0;
        float mx = h[L + 1][0];
        static_for<1, S::OUT>([&](auto JC) { mx = fmaxf(mx, h[L + 1][decltype(JC)::value]); });
        float se = 0.f, zc = 0.f;
        static_for<0, S::OUT>([&](auto JC) {
          constexpr int j = decltype(JC)::value;
          se += __expf(h[L + 1][j] - mx);
          zc = (j == cls) ? h[L + 1][j] : zc;
        });
        const float lse = mx + __logf(se);
        const float rs = 1.f / se;
        lpart = valid ? lse - zc : 0.f;
        static_for<0, S::OUT>([&](auto JC) {
          constexpr int j = decltype(JC)::value;
          dz[j] = valid ? S::rnd((__expf(h[L + 1][j] - mx) * rs - (j == cls ? 1.f : 0.f)) * inv) : 0.f;
        });
      }
      if (c0 == 0) DTP_STAMP(2);
      lacc += lpart;

      // ---------------- backward: dX chain (VALU, LDS weight blocks) + dW tiles (MFMA, K = samples)
      const PipeBwdCtx<S> pc{sm.wb, stg_pack, &sm.stage[wave][1][0], lane, slope, lpart};
      pipe_backward<S>(pc, pbt, pbt2, h, dz, acc);
    }
    if constexpr (S::BF) {
      const float wl = wave_sum(lacc);
      if (lane == 0) sm.lossw[wave] = wl;
    }
    DTP_STAMP(8 + wave);
    DTP_STAMP(3);
    // each wave parks its partial dW tiles in its OWN staging area (no other wave
    // touches it, and this wave's staging reads were issued before these writes),
    // so one barrier publishes them
    {
      const int q = lane >> 4, col = lane & 15;
#pragma unroll
      for (int tt = 0; tt < NT; ++tt)
        *reinterpret_cast<f32x4*>(&sm.stage[wave][0][0] + tt * SC::TSZ + SC::tslot(4 * q, col)) = acc[tt];
    }
    __syncthreads();
    // this step's Adam scalars: requested now, consumed after the reduction
    float2 adam_sc = make_float2(0.f, 1.f);
    if constexpr (kAdam) adam_sc = sm.adam_tab[it % kAdamTab];
    else if (ltab) adam_sc = sm.adam_tab[it % kAdamTab];
    DTP_STAMP(4);

    float g[NPT];
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < kWaves; ++ww) s += sm.stage[ww][0][tp[k]];
      g[k] = s;
    }
    float lsum = 0.f;
#pragma unroll
    for (int ww = 0; ww < kWaves; ++ww)
      lsum += S::BF ? sm.lossw[ww] : sm.stage[ww][0][SC::losspos()];
    const float mean_loss = lsum * inv;
    DTP_STAMP(5);

    float gloss = mean_loss;
    if constexpr (kXgmi) {
      // all-reduce (sum) this model's gradient + loss over every rank through
      // the peers' xGMI-mapped receive buffers, inside the step (xgmi_core.h)
      xepoch += 1u;
      gloss = xgmi_allreduce_model<NPT, kBlock>(a, model, P, g, mean_loss, xepoch, tid, xwait, 1, 0, &xdead);
    }

    // advance the sampler / loss-ring position and gather the next step's first
    // chunk now: its index hashing and LDS reads overlap the optimizer's latency
    // (FAST: the gather is straight-line code in the optimizer's basic block; the
    // loss-log store, a branch of thread 0, comes after the update)
    const int lslot_now = lslot;
    if constexpr (FAST) {
      roll(epoch, bi);
    } else if (!explicit_idx && ++bi == smp.steps_per_epoch) {
      bi = 0;
      ++epoch;
      epoch_keys(smp, epoch, keys);
    }
    if (a.loss_log && ++lslot == a.loss_log_cap) lslot = 0;
    if constexpr (FAST) {
      // the next step's samples from the index loaded a step ago, then the load for the
      // step after it (past the last step: an in-range table read, never used)
      nxt = fast_gather(fidx);
      roll(e2, b2);
      fidx = fast_index(e2, b2);
    } else if (it + 1 < a.n_steps) {
      const BatchPos bpn = batch_at(epoch, bi);
      nxt = gather(it + 1, bpn, keys, tid, bpn.size);
    }

    if constexpr (kMode == DTP_MODE_GRAD) {
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        const int p = NPT * tid + k;
        if (p < P) a.grad_out[(size_t)model * P + p] = g[k] * a.hp.grad_scale;
      }
      if (tid == 0) a.grad_out[(size_t)a.n_models * P + model] = mean_loss;
    } else {
      AdamScalars as = adam_consts(a.hp);
      as.step_size = adam_sc.x;
      as.bc2_sqrt = adam_sc.y;
      if constexpr (kAdam) decoupled_decay_step(a.hp, as, t, pw);  // AdamW: p *= d_t
      const float lr = ltab ? adam_sc.x : (float)a.hp.lr, mom = (float)a.hp.momentum, wd = (float)a.hp.weight_decay;
      // branch-free over the thread's NPT slots (slots past P hold zeros and store
      // into sm.sink), so the compiler can interleave the slots' dependency chains
      if constexpr (kClip) {  // the averaged gradient clipped in front of the update (clip_core.h)
        float x[NPT];
        gnorm = clip_gradient<NPT, kWaves>(a, g, x, P, tid, gnorm);
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          if constexpr (kAdam) adam_update(pw[k], mr[k], vr[k], x[k], as);
          else sgd_update(pw[k], mr[k], x[k], lr, mom, wd, t == 0);
        }
      } else {
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          if constexpr (kAdam) adam_update(pw[k], mr[k], vr[k], g[k] * a.hp.grad_scale, as);
          else sgd_update(pw[k], mr[k], g[k] * a.hp.grad_scale, lr, mom, wd, t == 0);
        }
      }
#pragma unroll
      for (int k = 0; k < NPT; ++k) {
        const bool own = NPT * tid + k < P;
        const float wv = S::rnd(pw[k]);
        *(own ? &sm.wb[pfl[k]] : &sm.sink[0]) = wv;
        *(own && pb[k] >= 0 ? &sm.wb[pb[k]] : &sm.sink[1]) = wv;
      }
    }
    // the thread that holds the global loss logs it (xgmi_core.h: the loss granule's owner)
    if (tid == (kXgmi ? xgmi_loss_tid<NPT>(P, kBlock) : 0) && a.loss_log) {
      const float lg = kXgmi ? gloss * a.hp.grad_scale : mean_loss;
      a.loss_log[(size_t)lslot_now * a.n_models + model] = lg;
    }
    DTP_STAMP(6);
    __syncthreads();  // updated weights visible; reduction tiles consumed
    // the next kAdamTab steps' Adam scalars, once every kAdamTab steps at a step
    // boundary (every wave read this step's entry before the barrier above)
    if ((kAdam || ltab) && (it + 1) % kAdamTab == 0 && it + 1 < a.n_steps) {
      fill_adam(it + 1);
      __syncthreads();
    }
    DTP_STAMP(7);
  }

  if constexpr (kUpdate) {
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
    if constexpr (kClip) {
      if (tid == 0 && a.max_norm > 0.f && a.norm_out) a.norm_out[model] = gnorm;
    }
    if (kXgmi && tid == 0) a.epoch[model] = xepoch;
    if (kXgmi && model == 0 && a.status) xgmi_record_wait(a.status, xwait, (unsigned long long)a.n_steps, tid);
    stamp_launch(21);
  }
}

// ------------------------------------------------------------------------------
// The instance table.  (IN, H, NL, OUT, bf16 compute, PROF): every row has all five modes
// plus the FAST instance of the two Adam modes (the training configuration of the demos and
// bench.py), and the clip twin of the generic instance in the four update modes (a clipped
// launch has no FAST instance: it runs the generic twin).  No accumulation twins: that row of
// OneInst.fn stays null.
#define DTP_ONE_SHAPES(X)                                                        \
  X(2, 10, 5, 1, false, true)  /* the toy model; the phase-stamp diagnostic */   \
  X(2, 10, 5, 1, true, false)                                                    \
  X(2, 10, 3, 1, false, false) /* shallower */                                   \
  X(2, 10, 5, 4, false, false) /* four outputs: multi-target MSE, the CE head */ \
  X(2, 10, 5, 4, true, false)                                                    \
  X(2, 15, 5, 1, false, false) /* wider */

template <class S, int MODE, bool PROF = false, bool FAST = false>
void launch_one(const DtpTrainArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((mlp_train_kernel<S, MODE, PROF, FAST>), dim3(a.n_models), dim3(kBlock), 0, st, a);
}

// variant V (plain or clip twin: MODE carries the variant's bit) of a row's four update modes
template <class S, StepVariant V>
constexpr void one_fill(OneInst& r) {
  constexpr int BIT = V == kClip ? kModeClip : 0;
  r.fn[V][DTP_MODE_ADAM] = &launch_one<S, DTP_MODE_ADAM | BIT>;
  r.fn[V][DTP_MODE_SGD] = &launch_one<S, DTP_MODE_SGD | BIT>;
  r.fn[V][DTP_MODE_XGMI_ADAM] = &launch_one<S, DTP_MODE_XGMI_ADAM | BIT>;
  r.fn[V][DTP_MODE_XGMI_SGD] = &launch_one<S, DTP_MODE_XGMI_SGD | BIT>;
}

template <class S, bool PROF>
constexpr OneInst one_row() {
  OneInst r{S::IN, S::H, S::NL, S::OUT, S::BF, Scal<S>::WS};
  r.fn[kPlain][DTP_MODE_GRAD] = &launch_one<S, DTP_MODE_GRAD>;
  one_fill<S, kPlain>(r);
  one_fill<S, kClip>(r);
  r.fast[DTP_MODE_ADAM] = &launch_one<S, DTP_MODE_ADAM, false, true>;
  r.fast[DTP_MODE_XGMI_ADAM] = &launch_one<S, DTP_MODE_XGMI_ADAM, false, true>;
  if constexpr (PROF) r.prof = &launch_one<S, DTP_MODE_ADAM, true, true>;
  return r;
}

#define X(I, H, N, O, B, PROF) one_row<Stage<I, H, N, O, false, B>, PROF>(),
static const OneInst kOne[] = {DTP_ONE_SHAPES(X)};
#undef X

const OneInst* one_lane_inst(int in, int h, int nl, int out, bool bf16) {
  for (const OneInst& r : kOne)
    if (r.in == in && r.h == h && r.nl == nl && r.out == out && r.bf16 == bf16) return &r;
  return nullptr;
}

}  // namespace dtp

// What the fused train step's sources share (mlp_train.hip: host dispatch, engine and C API;
// mlp_train_one.hip: the one-lane kernel; mlp_train_lanes.hip and its two twin sources: the
// several-lanes / split-batch kernel, mlp_train_lanes_kernel.h): the LDS budgets the host's
// picks test, the Adam-table helpers, the PROF stamp, and the instance tables' entry types with
// their two lookups.
#pragma once
#include "dtp_api.h"
#include "mlp_core.h"

namespace dtp {

// floats of dataset staged in LDS: the whole weak-scaling dataset of an 8-GPU
// node (n = 512 x 8 samples x (2 inputs + 1 target)) stays on-chip
constexpr int kDataCache = 12288;
// Adam bias-correction scalars of the next kAdamTab steps, formed cooperatively in
// f64 (torch's host math) once per kAdamTab steps instead of per step
constexpr int kAdamTab = 1024;

// entries base + tid + j * kBlock (j < J) of the host's Adam table for a launch starting
// at step t0: {lr / (1 - b1^t1), sqrt(1 - b2^t1)} with t1 = t0 + e + 1, clamped to the
// table's saturated last row
// (only the rows the launch's n_steps reach: a 20-step launch loads 20 entries, not 1024)
template <int J, int NTH = kBlock>
DTP_DEV void adam_tab_load(const DtpTrainArgs& a, int t0, int base, int tid, float2 (&v)[J]) {
  const float2* __restrict__ tab = reinterpret_cast<const float2*>(a.adam_tab);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int e = base + tid + j * NTH;
    const long long t1 = (long long)t0 + e + 1;
    v[j] = make_float2(0.f, 1.f);
    if (e < a.n_steps) v[j] = tab[t1 < a.adam_tab_len ? t1 : a.adam_tab_len - 1];
  }
}
template <int J, int NTH = kBlock>
DTP_DEV void adam_tab_store(float2* __restrict__ lds, int n, int tid, const float2 (&v)[J]) {
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (tid + j * NTH < n) lds[tid + j * NTH] = v[j];
}

// floats of dataset staged in LDS by the lanes kernel (strong scaling: n = 512 x 3)
constexpr int kLaneData = 4096;

// In-kernel phase stamps (diagnostic instantiation only, PROF = true): lane 0 of
// wave 0 records s_memtime at phase boundaries of the first 8 iterations; per-wave
// end-of-backward stamps at [8 + wave].  Never used on timed runs.
#define DTP_STAMP(K)                                                                     \
  do {                                                                                   \
    if constexpr (PROF) {                                                                \
      if (lane == 0 && it < 8 && (((K) >= 8 && (K) < 16) || wave == 0)) {                \
        unsigned long long _t;                                                           \
        __builtin_amdgcn_sched_barrier(0);                                               \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");       \
        __builtin_amdgcn_sched_barrier(0);                                               \
        prof[((size_t)blockIdx.x * 8 + it) * 32 + (K)] = _t;                             \
      }                                                                                  \
    }                                                                                    \
  } while (0)

using TrainLaunchFn = void (*)(const DtpTrainArgs&, hipStream_t);

constexpr bool mode_sgd(int mode) { return mode == DTP_MODE_SGD || mode == DTP_MODE_XGMI_SGD; }
constexpr bool mode_xgmi(int mode) { return mode == DTP_MODE_XGMI_ADAM || mode == DTP_MODE_XGMI_SGD; }

// The variant of a step instance: the plain step, its clip twin (clip_core.h: MODE | kModeClip)
// or its accumulation twin (accum_core.h: MODE | kModeAccum, which clips at run time).  A
// dimension of both instance tables; an instance without such a twin has a null entry there.
enum StepVariant { kPlain, kClip, kAccum, kVariants };

// One row of the one-lane table (mlp_train_one.hip): a (shape, precision) and its launchers.
struct OneInst {
  int in, h, nl, out;
  bool bf16;
  int ws;                          // Scal<S>::WS, floats of workspace
  TrainLaunchFn fn[kVariants][5];  // by DtpMode; clip twins: the four update modes; no accumulation twins
  TrainLaunchFn fast[5];           // the FAST instance of the mode (the Adam modes, plain only), else null
  TrainLaunchFn prof;              // PROF instance (FAST Adam), or null
};
const OneInst* one_lane_inst(int in, int h, int nl, int out, bool bf16);

// One row of the lanes table (mlp_train_lanes.hip): a (shape, precision, loss, optimizer
// family) and its launchers; null where the family has no such instance.
struct LanesInst {
  int in, h, nl, out;
  bool bf16, ce, sgd;
  TrainLaunchFn lanes[kVariants][2][2][2];  // [variant][8 waves][L == 4 (else 2)][xGMI]; the twins: 4 waves only
  TrainLaunchFn grp[kVariants][3];          // split-batch: run-time member count, 4 members, xGMI
  TrainLaunchFn grp8;                       // split-batch on 8-wave members (DTP_GRP_NW=8 A/B)
  TrainLaunchFn prof[2][2];                 // PROF lanes instances [8 waves][L == 4]
  TrainLaunchFn grp_prof[2];                // PROF split-batch instances [4 members as a constant]
};
// the family that serves `mode` (an optimizer mode), or null
const LanesInst* lanes_inst(int in, int h, int nl, int out, bool bf16, bool ce, int mode);

}  // namespace dtp

// Host side of the fused train step: which kernel instance a launch takes (the FAST
// preconditions, lanes per sample, the split-batch step; the instances themselves are the
// tables of mlp_train_one.hip and mlp_train_lanes.hip), argument validation, the native
// step engine and the C API; and the sampler probe kernel.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mlp_train_common.h"
#include "grp_core.h"

namespace dtp {

__global__ void sampler_probe_kernel(SamplerCfg s, long long t0, int n_steps, int* out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int st = blockIdx.y;
  if (k >= s.batch || st >= n_steps) return;
  const BatchPos bp = batch_pos(s, t0 + st);
  uint32_t keys[4];
  epoch_keys(s, bp.epoch, keys);
  out[(size_t)st * s.batch + k] = (k < bp.size) ? sample_index(s, bp, keys, k) : -1;
}

}  // namespace dtp

// ------------------------------------------------------------------------------
// the picks
namespace {
using dtp::check_launch;
using dtp::set_err;
using dtp::LanesInst;
using dtp::TrainLaunchFn;
using dtp::StepVariant;
using dtp::kPlain;
using dtp::kClip;
using dtp::kAccum;

// The forcing variables (A/B runs and tests), read once per process.
struct StepEnv {
  bool no_fast = false;     // DTP_FAST=0: no launch takes a FAST, several-lanes or split-batch instance
  bool accum_twin = false;  // DTP_ACCUM_TWIN=1: a launch without accumulation runs the accumulation twin too
  int L = 0, NW = 4;        // DTP_LANES=<L>[x<NW>] as given (L = 0: not a number); lanes_set: given at all
  bool lanes_set = false;
  int groups = -1;          // DTP_GROUPS: unset = the measured policy (-1), "on" = wherever an instance
                            // exists (1), anything else ("off" / "0" / "1") = never (0)
  bool grp_nw8 = false;     // DTP_GRP_NW=8: the split-batch A/B instance on 8-wave members
};
const StepEnv& step_env() {
  static const StepEnv env = [] {
    StepEnv e;
    const char* v;
    if ((v = getenv("DTP_FAST"))) e.no_fast = v[0] == '0';
    if ((v = getenv("DTP_ACCUM_TWIN"))) e.accum_twin = v[0] == '1';
    if ((v = getenv("DTP_LANES"))) {
      e.lanes_set = true;
      e.L = atoi(v);
      if (const char* x = strchr(v, 'x')) e.NW = atoi(x + 1);
    }
    if ((v = getenv("DTP_GROUPS"))) e.groups = strcmp(v, "on") == 0 ? 1 : 0;
    if ((v = getenv("DTP_GRP_NW"))) e.grp_nw8 = atoi(v) == 8;
    return e;
  }();
  return env;
}

// the FAST preconditions on the data path (the kernels' compile-time configuration): the
// SAMPLER_TABLE ring, the dataset cached in LDS, 0 <= slope <= 1, batch <= kBlock.  The
// several-lanes and split-batch steps need these, for every loss and optimizer they serve.
bool fast_base_ok(const DtpTrainArgs& a, int in, int out) {
  if (step_env().no_fast) return false;
  const dtp::SamplerCfg& s = a.smp;
  const int ydim = a.loss == DTP_LOSS_CE ? 1 : out;
  // n >= world: the FAST gather wraps a padded-list position with ONE subtraction of n
  // (positions stay below n + world - 1), where the generic sampler takes q % n
  const bool ring = s.perm && s.perm_epochs > 0 && (s.perm_epochs & (s.perm_epochs - 1)) == 0;
  return a.cache_data && min(s.batch, s.num_samples) <= dtp::kBlock && s.mode == dtp::SAMPLER_TABLE && ring &&
         s.n >= s.world && s.n * (in + ydim) <= dtp::kDataCache && a.hp.slope >= 0.f && a.hp.slope <= 1.f;
}

// may this launch take the one-lane FAST instance?  (the data-path preconditions, Adam, MSE)
bool fast_path_ok(const DtpTrainArgs& a, int in, int out, int mode) {
  return fast_base_ok(a, in, out) && (mode == DTP_MODE_ADAM || mode == DTP_MODE_XGMI_ADAM) &&
         a.loss == DTP_LOSS_MSE;
}

// The step instance of a launch: its launcher (null: no instance serves the launch), lanes
// per sample (1: the one-lane kernel), waves per workgroup, workgroups per model (> 1: the
// split-batch step, grp_core.h) and variant.
struct StepPick {
  TrainLaunchFn fn = nullptr;
  int L = 1, NW = 4, GR = 1;
  StepVariant v = kPlain;
};

// threads of the workgroups the fused step instances launch (one-lane: kBlock; lanes:
// 64 NW, NW = 4 or 8)
constexpr int kStepThreads[] = {dtp::kBlock, 4 * 64, 8 * 64};

long long xgmi_bytes_for(int n_models, int world, int slot16) {
  return 2ll * n_models * world * slot16 * 16ll;
}
int xgmi_slot16_threads(int P, int nth) { return dtp::xgmi_slot16(P, (P + nth - 1) / nth); }
int xgmi_max_slot16(int P) {
  int m = 0;
  for (int nth : kStepThreads) m = max(m, xgmi_slot16_threads(P, nth));
  return m;
}

// does the launch clip its gradient in the kernel (clip_core.h)?
bool clip_set(const DtpTrainArgs& a) { return a.max_norm > 0.f || a.clip_value > 0.f; }

// does the launch ask for an accumulation twin (accum_core.h)?  Under DTP_ACCUM_TWIN=1 a launch
// without accumulation does too: one micro-batch per step
bool accum_set(const DtpTrainArgs& a) { return a.accum > 1 || step_env().accum_twin; }

// The variant of a launch, decided here only: an accumulating launch of an update mode runs
// the accumulation twin (which clips at run time), any other clipping launch the clip twin.
StepVariant step_variant(const DtpTrainArgs& a, int mode) {
  if (accum_set(a) && mode != DTP_MODE_GRAD) return kAccum;
  return clip_set(a) ? kClip : kPlain;
}

// Split-batch step (engine launches only: it owns the exchange buffer): a per-rank batch
// above 64 on one rank runs on ceil(batch / 64) workgroups per model, each the 4-lanes step
// on 64 samples, their gradients summed on chip.  DTP_GROUPS (StepEnv) overrides the caller's
// request; a forced lanes instance (DTP_LANES) runs as asked.
int pick_groups(const DtpTrainArgs& a, int in, int out, bool allow, bool forced_lanes) {
  // the caller's request (DtpTrainArgs.groups before the engine fills it in): 0 policy,
  // 1 on, -1 off; the environment wins (A/B runs)
  const int env = step_env().groups;
  const int want = env >= 0 ? env : (a.groups > 0 ? 1 : (a.groups < 0 ? 0 : -1));
  if (!allow || want == 0 || forced_lanes || a.n_models > 8) return 1;
  if (a.smp.n * (in + out) > dtp::kLaneData) return 1;
  // the split-batch step keeps its loss-log position as a 32-bit element offset
  if (a.loss_log && (long long)a.loss_log_cap * a.n_models > 0x7fff0000LL) return 1;
  const int b = min(a.smp.batch, a.smp.num_samples);
  if (b <= 64) return 1;
  const int gr = (b + 63) / 64;
  // several ranks: one flat exchange over world x groups virtual members (xgmi_core.h)
  const int cap = a.smp.world == 1 ? dtp::kGrpMax : dtp::kXgmiMaxWorld / a.smp.world;
  if (gr > cap) return 1;
  if (want == 1) return gr;
  // the policy (docs/perf_notes.md "Round 5: the split-batch step"): on for 4 members per
  // model (per-rank batch 256 -- one rank: 3.35-3.40 vs 4.11 us/step, two ranks: 5.6 vs 6.2-6.6 in
  // the rehearsal); 2 members (batch 128) measured no better than the 2-lanes step
  return gr >= 4 ? gr : 1;
}

// 4 lanes per sample for per-rank batches <= 64, 2 for <= 128, else the one-lane kernel
// (L = 1).  DTP_LANES=<L>[x<NW>] forces a choice (A/B runs; NW = 8 runs two waves per
// SIMD, 512 / L samples); a forced pick whose batch bound does not hold falls back to 1.
StepPick pick_lanes(const DtpTrainArgs& a, int in, int out, bool fast, bool forced_lanes) {
  const StepEnv& env = step_env();
  StepPick r;
  if (!fast || a.smp.n * (in + out) > dtp::kLaneData) return r;
  // the largest batch a step sees: a rank's share of the epoch can be smaller than the
  // configured batch (strong scaling: 512 samples over 8 ranks -> 64 of batch 256)
  const int b = min(a.smp.batch, a.smp.num_samples);
  r.L = b <= dtp::kBlock / 4 ? 4 : (b <= dtp::kBlock / 2 ? 2 : 1);
  if (forced_lanes && (env.L == 1 || env.L == 2 || env.L == 4) && (env.NW == 4 || env.NW == 8)) {
    r.L = env.L;
    r.NW = env.L == 1 ? 4 : env.NW;
  }
  if (b > 64 * r.NW / r.L) r = StepPick{};
  return r;
}

// The step a validated launch takes.  The candidates, in order: the split-batch step, the
// lanes step, the one-lane kernel; the first with an instance in the launch's variant wins.
// A pick without a twin (the 8-wave instances, FAST one-lane; for accumulation every one-lane
// instance) is a null entry of that variant's row: the next candidate is tried, and a launch
// left with none returns fn = null.
StepPick resolve_train(const DtpTrainArgs& a, int in, int h, int nl, int out, int mode, bool allow_groups = false) {
  const StepEnv& env = step_env();
  const StepVariant v = step_variant(a, mode);
  const bool base = fast_base_ok(a, in, out);
  const int x = dtp::mode_xgmi(mode);
  // the 8-wave instances have no twins: a clipping or accumulating launch resolves as if
  // DTP_LANES=..x8 had not been given
  const bool forced_lanes = env.lanes_set && !(v != kPlain && env.NW == 8);
  if (const LanesInst* li = base ? dtp::lanes_inst(in, h, nl, out, a.bf16, a.loss == DTP_LOSS_CE, mode) : nullptr) {
    const int gr = pick_groups(a, in, out, allow_groups, forced_lanes);
    // A/B only (DTP_GRP_NW=8): the split-batch step on members of 128 samples, each the
    // two-waves-per-SIMD 4-lanes step (8 waves), half the members of the default -- toy
    // fp32 Adam + MSE at one rank (docs/perf_notes.md "Round 6: two members")
    if (env.grp_nw8 && v == kPlain && gr > 1 && mode == DTP_MODE_ADAM && li->grp8) {
      const int gr8 = (min(a.smp.batch, a.smp.num_samples) + 127) / 128;
      if (gr8 > 1 && a.smp.n * (in + out) <= dtp::kLaneData) return StepPick{li->grp8, 4, 8, gr8, v};
    }
    if (gr > 1)
      if (TrainLaunchFn f = li->grp[v][x ? 2 : (gr == 4 ? 1 : 0)]) return StepPick{f, 4, 4, gr, v};
    const StepPick lp = pick_lanes(a, in, out, base, forced_lanes);
    if (lp.L > 1)
      if (TrainLaunchFn f = li->lanes[v][lp.NW == 8][lp.L == 4][x]) return StepPick{f, lp.L, lp.NW, 1, v};
  }
  StepPick one;
  one.v = v;
  if (const dtp::OneInst* oi = dtp::one_lane_inst(in, h, nl, out, a.bf16))
    one.fn = v == kPlain && fast_path_ok(a, in, out, mode) && oi->fast[mode] ? oi->fast[mode] : oi->fn[v][mode];
  return one;
}

// What stands between a pick and its launch, as the error it leaves (0: none).  No instance:
// -6 for an accumulating launch (its pick has no accumulation twin), else -2.  And the xGMI
// receive buffer must cover the picked instance's granule layout (peers' stores through a
// buffer resource are not bounds-checked: an undersized buffer is corrupted).
int pick_err(const DtpTrainArgs& a, int in, int h, int nl, int out, int mode, const StepPick& p) {
  char m[288];
  if (!p.fn && p.v == kAccum) {
    snprintf(m, sizeof m, "gradient accumulation (accum = %d): this launch picks a step instance without an "
             "accumulation twin (the one-lane kernel: a per-rank batch above 128 without the split-batch step, "
             "groups off, or a shape / data path the several-lanes step does not serve)", a.accum);
    return set_err(-6, m);
  }
  if (!p.fn) return set_err(-2, "mlp shape / mode not instantiated for the fused train kernel");
  if (!dtp::mode_xgmi(mode) || a.xbuf_bytes <= 0) return 0;
  const int P = dtp_mlp_param_count(in, h, nl, out);
  const int nth = p.L > 1 ? 64 * p.NW : dtp::kBlock;
  const long long need = xgmi_bytes_for(a.n_models, a.smp.world * p.GR, xgmi_slot16_threads(P, nth));
  if (need > a.xbuf_bytes) {
    snprintf(m, sizeof m, "xGMI receive buffer too small: %lld bytes needed, %d allocated", need, a.xbuf_bytes);
    return set_err(-5, m);
  }
  return 0;
}

int validate_train(const DtpTrainArgs* a, int mode) {
  if (!a) return set_err(-1, "null args");
  if (mode < DTP_MODE_GRAD || mode > DTP_MODE_XGMI_SGD) return set_err(-1, "mode is not a DtpMode");
  if (a->n_models <= 0 || a->n_steps <= 0) return set_err(-1, "n_models and n_steps must be positive");
  if (a->smp.batch <= 0 || a->smp.n <= 0) return set_err(-1, "empty dataset or batch");
  if (a->smp.mode != dtp::SAMPLER_EXPLICIT && (a->smp.steps_per_epoch <= 0 || a->smp.num_samples <= 0))
    return set_err(-1, "bad sampler geometry");
  if (a->smp.mode == dtp::SAMPLER_EXPLICIT && !a->idx) return set_err(-1, "explicit sampler without indices");
  if (a->smp.mode == dtp::SAMPLER_TABLE &&
      (!a->smp.perm || a->smp.perm_epochs <= 0 || (a->smp.perm_epochs & (a->smp.perm_epochs - 1))))
    return set_err(-1, "table sampler needs a power-of-two permutation ring");
  if (a->loss_log && a->loss_log_cap <= 0) return set_err(-1, "loss_log_cap must be positive");
  if (!a->params || !a->X || !a->Y || !a->step) return set_err(-1, "params, X, Y and step are required");
  // the fused step reads a schedule's rates from the host-formed table (its rows carry them)
  if (mode != DTP_MODE_GRAD && a->hp.lr_tab && (!a->adam_tab || a->adam_tab_len <= 0 || a->hp.lr_tab_len <= 0))
    return set_err(-1, "a learning-rate schedule needs the host-formed per-step table (adam_tab)");
  if (mode == DTP_MODE_GRAD && !a->grad_out) return set_err(-1, "MODE_GRAD needs grad_out");
  if (mode != DTP_MODE_GRAD && !a->opt_m) return set_err(-1, "optimizer modes need opt_m");
  if ((mode == DTP_MODE_ADAM || mode == DTP_MODE_XGMI_ADAM) && !a->opt_v) return set_err(-1, "Adam needs opt_v");
  if (a->hp.decoupled_wd && dtp::mode_sgd(mode))
    return set_err(-1, "decoupled weight decay (AdamW) is Adam's: SGD has no decoupled form");
  if (a->max_norm < 0.f || a->clip_value < 0.f || a->max_norm != a->max_norm || a->clip_value != a->clip_value)
    return set_err(-4, "clipping: max_norm and clip_value must not be negative");
  if (a->max_norm > 0.f && a->clip_value > 0.f) return set_err(-4, "clipping: max_norm and clip_value are exclusive");
  if (a->max_norm > 0.f && !a->norm_out) return set_err(-5, "clipping by norm needs norm_out");
  if (mode == DTP_MODE_GRAD && clip_set(*a))
    return set_err(-4, "MODE_GRAD writes the raw gradient: clipping is for the update modes");
  if (a->accum < 0) return set_err(-4, "accumulation: accum must not be negative");
  if (a->accum > 1) {
    if (mode == DTP_MODE_GRAD)
      return set_err(-4, "MODE_GRAD writes one batch's gradient: accumulation is for the update modes");
    // the data position is t0 * accum micro-steps, a 32-bit count in the kernel
    const long long t0 = a->host_t0 >= 0 ? a->host_t0 : 0;
    if (t0 * a->accum > 0x7fffffffLL || (t0 + a->n_steps) * (long long)a->accum > 0x7fffffffLL ||
        (long long)a->n_steps * a->accum > 0x7fffffffLL)
      return set_err(-4, "accumulation: t0 * accum and n_steps * accum must stay below 2^31");
  }
  if (dtp::mode_xgmi(mode)) {
    if (!a->peers || !a->epoch) return set_err(-1, "xGMI modes need the peer table and epoch counters");
    if (a->smp.world < 1 || a->smp.world > dtp::kXgmiMaxWorld || a->smp.rank < 0 || a->smp.rank >= a->smp.world)
      return set_err(-1, "xGMI modes serve 1..8 ranks");
  }
  return 0;
}

// Native step executor: the argument block and the kernel instance are fixed at
// creation, so a call costs one kernel launch (no per-call marshalling or
// dispatch on the host; the Python side calls it with (handle, n_steps, stream)).
struct TrainEngine {
  DtpTrainArgs a;
  int mode;
  StepPick pick;  // the instance it launches
  void* grp_mem = nullptr;  // split-batch step: [status 16 ints | epochs | granule buffer]
  ~TrainEngine() {
    if (grp_mem) (void)hipFree(grp_mem);
  }
};

// the split-batch step's device state, zeroed: 64 B of timeout words, the per-model epoch
// counters (64 B aligned), then the [2][n_models][GR][slot16] granule buffer
int grp_alloc(TrainEngine* e, int P) {
  const int nth = 64 * e->pick.NW;
  const long long slot = dtp::grp_slot16(P, (P + nth - 1) / nth);
  const long long gbytes = 2ll * e->a.n_models * e->pick.GR * slot * 16;
  const long long ebytes = ((long long)e->a.n_models * 4 + 63) & ~63ll;
  const long long total = 64 + ebytes + gbytes;
  if (hipMalloc(&e->grp_mem, total) != hipSuccess) {
    e->grp_mem = nullptr;
    return set_err(-3, "hipMalloc of the split-batch exchange buffer failed");
  }
  if (hipMemset(e->grp_mem, 0, total) != hipSuccess) return set_err(-3, "hipMemset of the exchange buffer failed");
  char* b = static_cast<char*>(e->grp_mem);
  e->a.grp_status = reinterpret_cast<int*>(b);
  e->a.grp_epoch = reinterpret_cast<unsigned*>(b + 64);
  e->a.grp_buf = b + 64 + ebytes;
  e->a.groups = e->pick.GR;
  return 0;
}

}  // namespace

extern "C" {

int dtp_mlp_train_bf16_supported(int in, int h, int nl, int out) {
  return dtp::one_lane_inst(in, h, nl, out, true) != nullptr;
}

int dtp_mlp_workspace_floats(int in, int h, int nl, int out) {
  const dtp::OneInst* oi = dtp::one_lane_inst(in, h, nl, out, false);
  return oi ? oi->ws : 0;
}

// bytes of one rank's receive buffer of the fused step's xGMI exchange
// ([parity 2][model][src rank][slot] of 16-byte granules, xgmi_core.h)
long long dtp_xgmi_fused_buffer_bytes(int P, int n_models, int world) {
  // sized for the instance with the most granules: xgmi_slot16 is not monotone in the
  // parameters per thread, so take the max over every instantiated thread count; and for
  // the split-batch step's virtual members (world x groups <= kXgmiMaxWorld slots)
  const int slots = world <= dtp::kXgmiMaxWorld ? dtp::kXgmiMaxWorld : world;
  return xgmi_bytes_for(n_models, slots, xgmi_max_slot16(P));
}

int dtp_mlp_param_count(int in, int h, int nl, int out) {
  int p = 0;
  for (int l = 0; l < nl; ++l) {
    const int di = l == 0 ? in : h, dq = l == nl - 1 ? out : h;
    p += dq * (di + 1);
  }
  return p;
}

// The Adam instances read the host-formed table only with the host's step number (they are
// the unscheduled kernels to the byte), so a scheduled Adam launch that would read its step
// number on the device -- an eager launch without host_t0, a captured graph -- is refused
// on every launch path instead of training at hp.lr.
static int check_sched_t0(const DtpTrainArgs& a, int mode, int t0) {
  if ((mode == DTP_MODE_ADAM || mode == DTP_MODE_XGMI_ADAM) && a.hp.lr_tab && t0 < 0)
    return set_err(-1, "Adam under a learning-rate schedule reads the host-formed table: give the step number "
                       "(host_t0 / t0 >= 0); it cannot be captured in a graph");
  return 0;
}

int dtp_mlp_train(const DtpTrainArgs* a, int in, int h, int nl, int out, int mode, void* stream) {
  if (int rc = validate_train(a, mode)) return rc;
  if (mode == DTP_MODE_GRAD && a->n_steps != 1) return set_err(-4, "MODE_GRAD requires n_steps == 1");
  if (int rc = check_sched_t0(*a, mode, a->host_t0)) return rc;
  const StepPick p = resolve_train(*a, in, h, nl, out, mode);
  if (int rc = pick_err(*a, in, h, nl, out, mode, p)) return rc;
  p.fn(*a, (hipStream_t)stream);
  return check_launch("mlp_train_kernel");
}

void* dtp_train_engine_create(const DtpTrainArgs* a, int in, int h, int nl, int out, int mode) {
  if (validate_train(a, mode)) return nullptr;
  const StepPick p = resolve_train(*a, in, h, nl, out, mode, true);
  if (pick_err(*a, in, h, nl, out, mode, p)) return nullptr;
  auto* e = new TrainEngine();
  e->a = *a;
  e->mode = mode;
  e->pick = p;
  if (p.GR > 1 && grp_alloc(e, dtp_mlp_param_count(in, h, nl, out))) {
    delete e;
    return nullptr;
  }
  return e;
}

// the family that carries the PROF instances: toy shape, fp32, Adam + MSE
static const LanesInst* toy_lanes() { return dtp::lanes_inst(2, 10, 5, 1, false, false, DTP_MODE_ADAM); }

// diagnostic: the engine's split-batch step (fp32 toy shape) as its PROF instance, phase
// stamps into prof (u64[8 * groups blocks][8][32], block b = model b % 8, member b / 8)
int dtp_train_engine_profile(void* h, int n_steps, int t0, void* prof, void* stream) {
  auto* e = static_cast<TrainEngine*>(h);
  if (!e || !prof || n_steps <= 0) return set_err(-1, "bad engine profile args");
  if (e->pick.GR <= 1 || e->a.bf16 || e->mode != DTP_MODE_ADAM)
    return set_err(-2, "the engine profile instance is the fp32 split-batch step");
  if (clip_set(e->a)) return set_err(-2, "the engine profile instance has no clipping twin");
  if (e->a.accum > 1) return set_err(-4, "the profile instances have no accumulation twin");
  DtpTrainArgs a = e->a;
  a.n_steps = n_steps;
  a.host_t0 = t0;
  a.status = static_cast<int*>(prof);
  // the instance the engine runs: 4 members as a constant, else the run-time count
  toy_lanes()->grp_prof[e->pick.GR == 4 && e->pick.NW == 4](a, (hipStream_t)stream);
  return check_launch("mlp_train_lanes_kernel<grp, prof>");
}

// the split-batch exchange's sticky timeout words {flag, epoch} (synchronous copy; 0/0
// when the engine has no split-batch step)
int dtp_train_engine_status(void* h, int* out2) {
  auto* e = static_cast<TrainEngine*>(h);
  if (!e || !out2) return set_err(-1, "null engine");
  out2[0] = out2[1] = 0;
  if (!e->a.grp_status) return 0;
  if (hipMemcpy(out2, e->a.grp_status, 2 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return set_err(-3, "status copy failed");
  return 0;
}

// test hook: mark the split-batch exchange as timed out at `epoch` (sticky, as a real
// timeout would), so the next launch runs dead -- and must leave the state untouched
int dtp_train_engine_poison(void* h, int epoch) {
  auto* e = static_cast<TrainEngine*>(h);
  if (!e || !e->a.grp_status) return set_err(-1, "no split-batch exchange");
  const int w[2] = {1, epoch};
  if (hipMemcpy(e->a.grp_status, w, sizeof w, hipMemcpyHostToDevice) != hipSuccess)
    return set_err(-3, "status write failed");
  return 0;
}

// the step the engine runs
int dtp_train_engine_pick(void* h, DtpStepPick* out) {
  auto* e = static_cast<TrainEngine*>(h);
  if (!e || !out) return set_err(-1, "null engine");
  *out = DtpStepPick{e->pick.L, e->pick.NW, e->pick.GR, e->pick.v};
  return 0;
}

// the step a train engine would run for these arguments: validation and the engine's pick.
// 0, or the error dtp_train_engine_create would leave, with *out zeroed
int dtp_mlp_train_pick(const DtpTrainArgs* a, int in, int h, int nl, int out, int mode, DtpStepPick* pick) {
  if (!pick) return set_err(-1, "null pick record");
  *pick = DtpStepPick{};
  if (int rc = validate_train(a, mode)) return rc;
  const StepPick p = resolve_train(*a, in, h, nl, out, mode, true);
  if (int rc = pick_err(*a, in, h, nl, out, mode, p)) return rc;
  *pick = DtpStepPick{p.L, p.NW, p.GR, p.v};
  return 0;
}

// n_steps iterations in ONE persistent launch on `stream`, starting at step t0 (the
// host's mirror of the device step counters; -1: read them on the device)
int dtp_train_engine_run(void* h, int n_steps, int t0, void* stream) {
  auto* e = static_cast<TrainEngine*>(h);
  if (!e) return set_err(-1, "null engine");
  if (n_steps <= 0) return set_err(-1, "n_steps must be positive");
  if (e->mode == DTP_MODE_GRAD && n_steps != 1) return set_err(-4, "MODE_GRAD requires n_steps == 1");
  if (int rc = check_sched_t0(e->a, e->mode, t0)) return rc;  // (dtp_graph_capture_engine runs with t0 = -1)
  if (e->a.accum > 1 && ((long long)(t0 > 0 ? t0 : 0) + n_steps) * e->a.accum > 0x7fffffffLL)
    return set_err(-4, "accumulation: t0 * accum and n_steps * accum must stay below 2^31");
  e->a.n_steps = n_steps;
  e->a.host_t0 = t0;
  e->pick.fn(e->a, (hipStream_t)stream);
  return check_launch("mlp_train_kernel");
}

void dtp_train_engine_destroy(void* h) { delete static_cast<TrainEngine*>(h); }

// diagnostic: toy shape, Adam, phase stamps into a->status (as u64[n_models][8][16])
int dtp_mlp_train_profile(const DtpTrainArgs* a, void* stream) {
  if (a && a->accum > 1) return set_err(-4, "the profile instances have no accumulation twin");
  if (!fast_path_ok(*a, 2, 1, DTP_MODE_ADAM))
    return set_err(-2, "the profile instance is the FAST one: cached dataset, SAMPLER_TABLE sampler");
  dtp::one_lane_inst(2, 10, 5, 1, false)->prof(*a, (hipStream_t)stream);
  return check_launch("mlp_train_kernel<prof>");
}

// same for the lanes step (toy shape), L = 2 or 4
int dtp_mlp_train_profile_lanes(const DtpTrainArgs* a, int lanes, void* stream) {
  const int L = lanes & 0xff, NW = lanes >> 8 ? lanes >> 8 : 4;
  if ((L != 2 && L != 4) || (NW != 4 && NW != 8))
    return set_err(-1, "lanes must be 2 or 4 (| waves << 8, waves 4 or 8)");
  if (a && a->accum > 1) return set_err(-4, "the profile instances have no accumulation twin");
  if (!fast_path_ok(*a, 2, 1, DTP_MODE_ADAM) || min(a->smp.batch, a->smp.num_samples) > 64 * NW / L ||
      a->smp.n * (2 + 1) > dtp::kLaneData)
    return set_err(-2, "the lanes profile instance needs the FAST configuration and batch <= 64 NW / L");
  toy_lanes()->prof[NW == 8][L == 4](*a, (hipStream_t)stream);
  return check_launch("mlp_train_lanes_kernel<prof>");
}

int dtp_sampler_indices(const dtp::SamplerCfg* s, long long t0, int n_steps, int* out, void* stream) {
  if (!s || !out || s->batch <= 0 || n_steps <= 0) return set_err(-1, "bad sampler probe args");
  dim3 grid((s->batch + 255) / 256, n_steps), block(256);
  hipLaunchKernelGGL(dtp::sampler_probe_kernel, grid, block, 0, (hipStream_t)stream, *s, t0, n_steps, out);
  return check_launch("sampler_probe_kernel");
}

}  // extern "C"

// C ABI of libdtp.so (consumed from Python through ctypes; every struct here
// has a mirror in distributed_training_pytorch_amd/_native.py — keep in sync).
#pragma once
#include <stdint.h>
#include "sampler.h"

extern "C" {

// ---- fused train step (fwd + loss + bwd [+ optimizer]) for n_models MLPs ----
enum DtpTrainMode : int {
  DTP_MODE_GRAD = 0,       // write local mean-loss gradients (+ loss) into grad_out; no update
  DTP_MODE_ADAM = 1,       // fused Adam update (single rank, or grads already global)
  DTP_MODE_SGD = 2,        // fused SGD(+momentum) update
  DTP_MODE_XGMI_ADAM = 3,  // in-kernel xGMI all-reduce across ranks, then Adam
  DTP_MODE_XGMI_SGD = 4,   // in-kernel xGMI all-reduce across ranks, then SGD
};

enum DtpLoss : int { DTP_LOSS_MSE = 0, DTP_LOSS_CE = 1 };

struct DtpHyper {
  double lr, beta1, beta2, eps, weight_decay, momentum;
  float slope;        // LeakyReLU negative slope
  float grad_scale;   // applied to the summed gradient before the update (1/world for DDP averaging)
  // learning-rate schedule: the step that follows t taken steps (the device step counter
  // before it) uses lr_tab[min(t, lr_tab_len - 1)] in place of lr.  Device memory, float64
  // (torch's param-group lr); null: lr.  The owner keeps it alive while launches or
  // captured graphs can run.
  const double* lr_tab;
  int lr_tab_len;
  // 1: AdamW, torch.optim.Adam(decoupled_weight_decay=True): the step after t taken steps first
  // scales p by d_t = (float)(1.0 - lr_t * weight_decay) (f64 product and difference, one fp32
  // multiply), then runs Adam's update on the gradient as it arrived -- weight_decay enters
  // neither g nor m / v.  Adam modes only; 0: weight_decay * p is added to the gradient.
  // (It takes the place of a padding int: the block's size and every offset are unchanged.)
  int decoupled_wd;
};

struct DtpTrainArgs {
  const float* X;       // [n][IN] dataset inputs (device resident)
  const float* Y;       // [n][OUT] targets (MSE) or [n] class ids stored as float (CE)
  const int* idx;       // SAMPLER_EXPLICIT: [n_steps][batch] dataset indices
  float* params;        // [n_models][P]
  float* opt_m;         // [n_models][P] Adam exp_avg / SGD momentum buffer
  float* opt_v;         // [n_models][P] Adam exp_avg_sq
  int* step;            // [n_models] optimizer step counters (device side)
  float* grad_out;      // MODE_GRAD: [n_models][P] gradients then [n_models] mean losses
  float* loss_log;      // [loss_log_cap][n_models] mean loss per step (nullable)
  int* status;          // [16] error / timeout words (xGMI mode), nullable
  float* const* peers;  // MODE_XGMI_*: [world] device pointers of every rank's receive buffer
  unsigned* epoch;      // MODE_XGMI_*: [n_models] exchange epoch counters (device)
  float* wsp;           // [n_models][dtp_mlp_workspace_floats] scalar-weight workspace (scratch)
  int loss_log_cap;
  int n_models;
  int n_steps;
  int loss;             // DtpLoss
  int cache_data;       // stage the dataset in LDS (persistent multi-step runs)
  int timeout_us;       // bound on every cross-GPU spin (xGMI)
  int bf16;             // bf16 compute instance (fp32 master weights / Adam), toy shapes
  int host_t0;          // >= 0: the step number of the first step (= the device counters), else read them
  dtp::SamplerCfg smp;
  DtpHyper hp;
  // Adam bias-correction scalars {lr / (1 - b1^t), sqrt(1 - b2^t)} of step t at [t], formed on
  // the host in f64 (torch's math); [len - 1] holds the saturated values (every later t).
  // Nullable: the kernel forms them itself.  Used with host_t0 >= 0 (the persistent engine).
  // With a learning-rate schedule (hp.lr_tab) the table is required; its rows carry the step's
  // rate: Adam {lr_t / (1 - b1^t), ...} (host_t0 >= 0 required), SGD {lr_t, 1} (either source
  // of t0), with lr_t the rate after t - 1 taken steps.
  const float* adam_tab;  // [adam_tab_len][2]
  int adam_tab_len;
  int xbuf_bytes;  // MODE_XGMI_*: bytes of each rank's receive buffer (0: unchecked)
  // split-batch step (grp_core.h): the engine's own exchange buffer, epoch counters and
  // timeout words; groups = workgroups per model.  Filled by dtp_train_engine_create; on
  // input groups is the caller's request: 0 the measured policy, 1 on, -1 off.
  void* grp_buf;
  unsigned* grp_epoch;
  int* grp_status;
  int groups;
  // gradient accumulation inside the step (accum_core.h), the update modes of the several-lanes
  // / split-batch kernel: one optimizer step consumes the `accum` consecutive batches
  // t accum .. t accum + accum - 1 of the sampler order; 0 or 1 = off.  n_steps, host_t0 and the
  // device counters stay optimizer steps; the caller folds 1 / accum into hp.grad_scale.
  // (It takes the place of a padding int: the block's size and every other offset are unchanged,
  // and with them the kernel arguments of every existing instance.)
  int accum;
  // gradient clipping inside the step (clip_core.h), per model, the update modes only; all
  // zeros = off.  At most one of max_norm / clip_value may be set; the meaning of DtpOptArgs's.
  float max_norm;    // > 0: scale model i's gradient by clamp(max_norm / (norm_i + 1e-6), max=1)
  float clip_value;  // > 0: clamp every element of the gradient * hp.grad_scale to [-clip_value, clip_value]
  float* norm_out;   // max_norm > 0: [n_models] L2 norm before clipping, of the last step a launch ran
};

int dtp_version(void);
const char* dtp_last_error(void);
int dtp_mlp_supported(int in, int h, int nl, int out, int final_act);
int dtp_mlp_supported_bf16(int in, int h, int nl, int out, int final_act);
int dtp_mlp_param_count(int in, int h, int nl, int out);
int dtp_mlp_workspace_floats(int in, int h, int nl, int out);
int dtp_mlp_train_bf16_supported(int in, int h, int nl, int out);
int dtp_mlp_train(const DtpTrainArgs* a, int in, int h, int nl, int out, int mode, void* stream);
int dtp_mlp_train_profile(const DtpTrainArgs* a, void* stream);
int dtp_mlp_train_profile_lanes(const DtpTrainArgs* a, int lanes, void* stream);
// Which step a launch or an engine runs: lanes per sample (1: the one-lane kernel, 2 / 4: the
// several-lanes step, mlp_lanes.h), waves per workgroup, workgroups per model (> 1: the
// split-batch step, grp_core.h) and variant (0 plain, 1 the clip twin, clip_core.h, 2 the
// accumulation twin, accum_core.h).
struct DtpStepPick {
  int lanes, waves, groups, variant;
};
// the step a train engine would run for these arguments: 0, or the error code that
// dtp_train_engine_create would leave, with *out zeroed
int dtp_mlp_train_pick(const DtpTrainArgs* a, int in, int h, int nl, int out, int mode, DtpStepPick* out_pick);
int dtp_train_engine_pick(void* engine, DtpStepPick* out_pick);
long long dtp_xgmi_fused_buffer_bytes(int P, int n_models, int world);

// ---- stage forward / backward (autograd path, layer-split pipeline) ----
struct DtpStageArgs {
  const float* x;         // [B][IN]
  const float* params;    // [P]
  float* out;             // [B][OUT]  (forward output; read by backward when FINAL_ACT)
  float* saved;           // [B][(NL-1)*H] hidden activations
  const float* grad_out;  // [B][OUT]  (backward)
  float* grad_in;         // [B][IN]   (backward, nullable)
  float* grad_params;     // [P]       (backward; must be zeroed when the grid has >1 block and !accumulate)
  float* out_peer;        // [B][OUT]  forward: second copy of the output stored straight into
                          //           the next stage's GPU (peer-mapped over xGMI), nullable
  int batch;
  float slope;
  int accumulate;  // backward: add into grad_params (a persistent .grad view) instead of overwriting it
  int bf16;        // bf16 compute (Stage<..., BF>: bf16 operands, fp32 accumulation and weight gradients)
};

int dtp_mlp_stage_fwd(const DtpStageArgs* a, int in, int h, int nl, int out, int final_act, void* stream);
// up to DTP_STAGE_MULTI_MAX models of one shape forward in ONE launch
#define DTP_STAGE_MULTI_MAX 4
struct DtpStageMulti {
  DtpStageArgs stage[DTP_STAGE_MULTI_MAX];
  int n;
  int pad_;
};
int dtp_mlp_stage_fwd_multi(const DtpStageMulti* m, int in, int h, int nl, int out, int final_act, void* stream);
int dtp_mlp_stage_bwd(const DtpStageArgs* a, int in, int h, int nl, int out, int final_act, void* stream);

// ---- held-out evaluation (eval.hip): forward + loss + reduction, all models in one launch ----
struct DtpEvalArgs {
  const float* X;        // [rows][IN]
  const float* Y;        // [rows][OUT] (MSE) or [rows] class ids as float (CE), as DtpTrainArgs
  const float* params;   // [n_models][P], torch order (the engines' flat rows)
  double* out;           // [n_models][2] = {sum of per-sample losses, correct (CE; 0 for MSE)}
  double* ws;            // dtp_mlp_eval_ws_bytes(n, n_models) bytes of scratch, may be null when that is 0
  long long row0, row_stride, n;  // sample k reads row row0 + k * row_stride  (a rank's shard: rank, world)
  int n_models;
  int loss;              // DtpLoss
  int bf16;              // bf16 compute instance (Stage<..., BF>), fp32 loss
  float slope;
};
// out is a pure function of the arguments (fixed reduction order, no atomics): bitwise equal
// run to run and under graph replay.  n == 0 writes zeros.
int dtp_mlp_eval(const DtpEvalArgs* a, int in, int h, int nl, int out, void* stream);
long long dtp_mlp_eval_ws_bytes(long long n, int n_models);
long long dtp_mlp_eval_one_launch_rows(void);  // n up to here: one launch, no workspace

// ---- persistent layer-split pipeline stage (split_train.hip) ----
// One stage of a model split by layers over several GPUs, resident for n_steps
// iterations: the stage's activation goes to the next stage and the input gradient
// back to the previous one as epoch-tagged granules stored straight into the
// neighbour GPU's receive buffer (peer-mapped over xGMI); the stage's weight
// gradient is (optionally) all-reduced over the data-parallel ranks in-kernel and
// the optimizer is fused.
struct DtpSplitStageArgs {
  const float* X;         // [n][IN of the model]  dataset inputs (first stage)
  const float* Y;         // [n][OUT of the model] targets (last stage)
  float* params;          // [P] this stage's parameters (torch order)
  float* opt_m;           // [P] Adam exp_avg / SGD momentum
  float* opt_v;           // [P] Adam exp_avg_sq
  int* step;              // [1] optimizer step counter (device)
  float* loss_log;        // [loss_log_cap] global mean loss per step (last stage), nullable
  int* status;            // [16]: [0,1] stage-link timeout flag / epoch, [2,3] data-parallel exchange
  void* act_in;           // receive buffer of the incoming activation (not the first stage), local
  void* act_out;          // the next stage's act_in, peer-mapped (not the last stage)
  void* grad_in;          // receive buffer of the incoming output gradient (not the last stage), local
  void* grad_out;         // the previous stage's grad_in, peer-mapped (not the first stage)
  float* const* dp_peers; // [dp_world] this stage's exchange buffers on every DP rank (dp_world > 1)
  int loss_log_cap;
  int n_steps;
  int timeout_us;
  int cache_data;
  int dp_world;
  int dp_rank;
  int optim;              // DTP_MODE_ADAM or DTP_MODE_SGD
  int link_local;         // bit 0: the previous stage, bit 1: the next stage is on this GPU;
                          // bit 2: every neighbour stage runs in this launch (split_lanes.hip plain links)
                          // (device-scope link: plain device memory, sc1); else system scope
  dtp::SamplerCfg smp;
  DtpHyper hp;            // grad_scale = 1 / dp_world
  // split-batch stages (split_lanes.hip, members > 1 on one rank): the stage's on-chip
  // member exchange buffer ([2][members][slot16] granules, zeroed), nullable
  void* grp_buf;
};

#define DTP_SPLIT_MAX_LOCAL 8
// the stages placed on one GPU, launched together (one workgroup each)
struct DtpSplitLaunch {
  DtpSplitStageArgs stage[DTP_SPLIT_MAX_LOCAL];
  int shape_id[DTP_SPLIT_MAX_LOCAL];  // dtp_split_shape_id of each stage
  int n;
  int members;  // split_lanes.hip: workgroups per stage (the stage's batch in member slices); else unused
};

int dtp_split_launch(const DtpSplitLaunch* L, void* stream);
int dtp_split_shape_id(int in, int h, int nl, int out, int final_act, int first);
long long dtp_split_link_bytes(int width, int batch);
int dtp_split_stage_supported(int in, int h, int nl, int out, int final_act, int first);
// split-batch stages: every stage's batch over L->members workgroups of the 4-lanes schedule
int dtp_split_lanes_launch(const DtpSplitLaunch* L, void* stream);
long long dtp_split_lanes_grp_bytes(int P, int members);

// ---- flat optimizers over [n_models][P] (after an external all-reduce) ----
struct DtpOptArgs {
  float* params;
  float* opt_m;
  float* opt_v;
  int* step;          // [n_models]
  const float* grad;  // [n_models][P] (+ [n_models] losses when loss_log != null)
  float* loss_log;
  int loss_log_cap;
  int n_models;
  int P;
  int kind;           // DTP_MODE_ADAM or DTP_MODE_SGD
  float loss_scale;   // applied to the all-reduced losses (1/world)
  int flags;          // DTP_OPT_ZERO_GRAD: write 0 over every gradient element once read
  DtpHyper hp;
  void* shadow;       // [n_models][shadow_ld] bf16 copy of the updated params, or null
  long long shadow_ld;  // row stride of shadow in elements (>= P)
  // gradient clipping, per row (one model = one optimizer); all zeros = off.  At most one of
  // max_norm / clip_value may be set.
  float max_norm;     // > 0: scale row i's gradient by clamp(max_norm / (norm_i + 1e-6), max=1)
  float clip_value;   // > 0: clamp every element of grad * hp.grad_scale to [-clip_value, clip_value]
  double* norm_ws;    // max_norm > 0 and P > 4096: dtp_grad_norm_ws_bytes(P) * n_models bytes of scratch
  float* norm_out;    // max_norm > 0: [n_models] L2 norm of grad * hp.grad_scale before clipping
};

#define DTP_OPT_ZERO_GRAD 1
int dtp_flat_optimizer(const DtpOptArgs* a, void* stream);
// out[i] = || grad[i, :] * scale ||_2 (fp64 accumulation in a fixed order: bitwise reproducible);
// ws: dtp_grad_norm_ws_bytes(P) * n_models bytes (may be null when that is 0)
int dtp_grad_norm(const float* grad, int n_models, int P, float scale, double* ws, float* out, void* stream);
long long dtp_grad_norm_ws_bytes(int P);
// the same norm, then grad[i, :] *= clamp(max_norm / (out[i] + 1e-6), max=1) in place: two launches
int dtp_clip_grad_norm(float* grad, int n_models, int P, float max_norm, double* ws, float* out, void* stream);

// ---- MFMA GEMM with fused Linear epilogues (gemm.hip) ----
#define DTP_DT_F32 0
#define DTP_DT_BF16 1
struct DtpGemmArgs {
  const void* A;      // A(m,k) = A[m*lda+k] (trans_a=0) or A[k*lda+m] (trans_a=1)
  const void* B;      // B(n,k) = B[n*ldb+k] (trans_b=0) or B[k*ldb+n] (trans_b=1)
  void* C;            // [M][ldc], out_dtype
  const float* bias;  // [N] or null
  const void* aux;    // [M][ldaux] (dtype): multiply by LeakyReLU'(aux) (backward through the previous layer)
  long long lda, ldb, ldc, ldaux;
  int M, N, K;
  int dtype;       // DTP_DT_* of A, B, aux
  int out_dtype;   // DTP_DT_* of C
  int trans_a, trans_b;
  int act;         // 1: LeakyReLU(slope) on the result
  int accumulate;  // 1: C += result
  int splitk;      // >1: K split over blocks, f32 atomics into C
  float alpha, slope;
  int vec_a, vec_b;  // set by dtp_gemm (16-byte loads allowed)
  int force_big;     // tests: take the 256x256 bf16 kernel for any layout it supports
  int fast;          // LDS-DMA 256x256 bf16 kernel: 0 auto, 1 whenever its preconditions hold, -1 never
  int pad_;
  void* work;              // split-K partial sums of the 8-phase kernel (splitk = 0: dtp_gemm picks)
  long long work_bytes;
};

int dtp_gemm(const DtpGemmArgs* a, void* stream);
// bytes of DtpGemmArgs::work the call would use with splitk = 0 (0: no split-K plan)
long long dtp_gemm_workspace(const DtpGemmArgs* a);
// out[n] (+)= sum_m X[m*ld+n]  (bias gradients)
int dtp_colsum(const void* X, long long ld, int M, int N, int dtype, float* out, int accumulate, void* stream);

// ---- FP8 (OCP e4m3 / e5m2) quantiser and GEMM (fp8_quant.hip, gemm_fp8.hip) ----
#define DTP_FP8_E4M3 0
#define DTP_FP8_E5M2 1
#define DTP_FP8_WS_FLOATS 1026  // workspace of dtp_fp8_quantize: scale, 1 / scale, 1024 amax partials
// Per-tensor scaled cast: ws[0] = fmax(fmt) / amax|x| (1 for an all-zero x), ws[1] = 1 / ws[0],
// q[m*ldq+k] = cvt(x[m*ldx+k] * ws[0]) and, with qT, qT[k*ldt+m] likewise.  x is f32 or bf16
// (DTP_DT_*), K % 16 == 0, ldq % 16 == 0, ldt % 16 == 0 and ldt >= M rounded up to 16 (the
// columns of qT past M are written as zeros).  Two launches, no host read.
int dtp_fp8_quantize(const void* x, long long ldx, int M, int K, int dtype, int fmt, void* q, long long ldq,
                     void* qT, long long ldt, float* ws, void* stream);

// -- delayed scaling: the scale comes from the amaxes of earlier steps, so it is known before the tensor is --
// One record per quantised tensor.  `partials`: word 0 the count n of partials its last producer wrote
// (0: nothing since the last update), words 1 .. n the maxima of |x| as f32 bit patterns; every producer
// (dtp_fp8_amax, dtp_fp8_quantize_scaled, dtp_gemm_fp8 with q) overwrites all of its n words and the count.
struct DtpFp8ScaleRec {
  unsigned* partials;  // [1 + cap]
  float* history;      // [H] ring of amaxes, zeros while empty
  float* scale;        // [2]: scale, 1 / scale
  int* pos;            // next ring slot
  int cap, H;          // H <= 1024
  float fmax;          // 448 (e4m3) or 57344 (e5m2)
  int pad_;
};
// For each record: n > 0: push max(partials) into the ring and set the count to 0; then
// scale = min(fmax / max(history), 2^126), 1 if that maximum is 0, and 1 / scale.  One launch, no host read.
int dtp_fp8_scale_update(DtpFp8ScaleRec* recs, int n_recs, void* stream);
// amax partials of x (as dtp_fp8_quantize's first launch) into the record layout: part[0] = n, part[1 .. n]
int dtp_fp8_amax(const void* x, long long ldx, int M, int K, int dtype, unsigned* part, int cap, void* stream);
// dtp_fp8_quantize with a given scale: q = cvt_rne(clamp(x * *scale, -fmax, fmax)); one launch reads x once,
// writes q, qT (may be null) and the amax partials of x (one per 64 x 64 tile; cap >= tiles).
int dtp_fp8_quantize_scaled(const void* x, long long ldx, int M, int K, int dtype, int fmt, void* q, long long ldq,
                            void* qT, long long ldt, const float* scale, unsigned* part, int cap, void* stream);

struct DtpGemmFp8Args {
  const void* A;        // [M][lda] fp8 (fmt_a), K-contiguous
  const void* B;        // [N][ldb] fp8 (fmt_b), K-contiguous
  void* C;              // [M][ldc], out_dtype
  const float* bias;    // [N] or null
  const void* aux;      // [M][ldaux] bf16 or null: multiply by LeakyReLU'(aux)
  const float* sa_inv;  // device scalars: the operands' inverse scales
  const float* sb_inv;
  long long lda, ldb, ldc, ldaux;
  int M, N, K;          // K % 16 == 0; bytes of a row past K up to the next multiple of 16 are never read
  int fmt_a, fmt_b;     // DTP_FP8_*: e4m3 x e4m3 or e5m2 x e4m3
  int out_dtype;        // DTP_DT_* of C
  int act;              // 1: LeakyReLU(slope) on the result
  int accumulate;       // 1: C += result
  float slope;
  int mfma;             // matrix instruction: 0 the 16x16x128 f8f6f4 MFMA, 1 the 16x16x32 fp8 / bf8 MFMAs
  int splitk;           // K-slices per output tile: 0 the library plans, 1 unsplit, S > 1 forced (tests, probes)
  void* work;           // split-K partial sums, 4 S M N bytes (uninitialised is fine); unused when unsplit
  long long work_bytes;
};
// C[M,N] (+)= epilogue(sa_inv * sb_inv * A(m,:) . B(n,:)), fp32 accumulation, the epilogues of dtp_gemm
int dtp_gemm_fp8(const DtpGemmFp8Args* a, void* stream);
// Quantised output for delayed scaling.  Needs a bf16 C without accumulate or split-K, and N % 16 == 0:
// q[m*ldq+n] = cvt_rne(clamp(C_bf16[m][n] * *scale, -fmax, fmax)) in format fmt, qT[n*ldqt+m] likewise
// (qT may be null; ldqt >= M rounded up to 16, columns [M, that) written as zeros), and part receives
// the |C_bf16| amax partials in the layout of DtpFp8ScaleRec::partials (cap >= 8 per 256 x 256 tile).
struct DtpFp8QuantOut {
  void* q;
  void* qT;
  const float* scale;  // device scalar
  unsigned* part;
  long long ldq, ldqt;
  int fmt;             // DTP_FP8_*
  int cap;
};
// dtp_gemm_fp8 that also emits C quantised: the pipelined kernel's epilogue writes q, qT and part itself;
// the short-K instance and an unaligned C / aux run the plain GEMM and then dtp_fp8_quantize_scaled on C:
// the same bits either way.  qo null: dtp_gemm_fp8.
int dtp_gemm_fp8_quant(const DtpGemmFp8Args* a, const DtpFp8QuantOut* qo, void* stream);
// bytes of DtpGemmFp8Args::work the call would use with splitk = 0 (0: no split-K plan); host only
long long dtp_gemm_fp8_workspace(const DtpGemmFp8Args* a);

// -- the flat optimizer that also emits the e4m3 weight operands of the delayed recipe (optim_fp8.hip) --
// One record per shadowed weight: a contiguous [out][in] matrix inside one row of the flat [n_models][P]
// buffers, both widths multiples of 16.  The launch that updates it writes q = cvt_rne(clamp(p_new * *scale,
// +-448)) row-major and transposed, the |p_new| amax of every 64 x 64 tile into `partials` (the layout of
// DtpFp8ScaleRec::partials: word 0 the tile count) and {scale[0], scale[1]} as it read them into `used`.
struct DtpFp8ShadowRec {
  const float* scale;   // [2] device: the slot's scale and 1 / scale
  unsigned* partials;   // [1 + cap]
  float* used;          // [2]
  void* q;              // [out][in] e4m3, 16-byte aligned
  void* qT;             // [in][out] e4m3, 16-byte aligned
  long long offset;     // of element (0, 0) in the flat buffers: model * P + column
  int out, in;
  int cap;
  int pad_;
};
// One workgroup's work.  rec >= 0: tile `a` (row-major over ceil(out / 64) x ceil(in / 64)) of that record.
// rec < 0: the element-wise update of columns [a, a + b) of row `model` (everything that is no shadowed weight).
struct DtpFp8WorkItem {
  int rec, a, b, model;
  int first;  // 1 on one item per model: it publishes the row's loss-log entry and norm
  int pad_[3];
};
struct DtpFp8ShadowWork {
  const DtpFp8ShadowRec* recs;  // the records again, on the device
  const DtpFp8WorkItem* items;  // device
  int n_items;
  int pad_;
};
// dtp_flat_optimizer (a->shadow must be null) as one launch over the work items, then the step counters.
// `recs` is the host copy, checked here; clipping by norm launches the norm first (its partials for rows of
// more than 4096 elements, else the finished norm into norm_out).
int dtp_flat_optimizer_fp8(const DtpOptArgs* a, const DtpFp8ShadowRec* recs, int n_recs, const DtpFp8ShadowWork* work,
                           void* stream);

// ---- MXFP8: FP8 with one E8M0 scale byte per 32 elements along K (mxfp8_quant.hip, gemm_mxfp8.hip) ----
// Block-scaled cast of x [M][ldx] (f32 or bf16, K % 32 == 0, finite).  For each block of 32 along K with
// a = max|x|: scale byte sb = a == 0 ? 127 : max(expfield(a) - emax, 0) (emax 8 e4m3 / 15 e5m2), elements
// cvt_rne(clamp(x * 2^(127 - sb), -fmax, fmax)).  q [M][ldq] (ldq % 16 == 0), s [M][lds] (lds % 4 == 0,
// lds >= 4 ceil(K / 128); bytes past K / 32 are written as 127).  With qT: the copy quantised along M,
// qT [K][ldt] (ldt % 16 == 0, ldt >= Mp = M rounded up to 32; bytes past M up to Mp are zeros) and
// sT [K][ldst] (as s, for Mp).  One launch, no workspace, no host read.
int dtp_mxfp8_quantize(const void* x, long long ldx, int M, int K, int dtype, int fmt, void* q, long long ldq, void* s,
                       long long lds, void* qT, long long ldt, void* sT, long long ldst, void* stream);

struct DtpGemmMxArgs {
  const void* A;             // [M][lda] fp8 (fmt_a), K-contiguous
  const void* B;             // [N][ldb] fp8 (fmt_b), K-contiguous
  void* C;                   // [M][ldc], out_dtype
  const float* bias;         // [N] or null
  const void* aux;           // [M][ldaux] bf16 or null: multiply by LeakyReLU'(aux)
  const unsigned char* sa;   // [M][ldsa] E8M0 bytes: byte kb scales A[m][32 kb .. +32)
  const unsigned char* sb;   // [N][ldsb]
  long long lda, ldb, ldc, ldaux, ldsa, ldsb;  // ldsa, ldsb >= 4 ceil(K / 128)
  int M, N, K;               // K % 32 == 0
  int fmt_a, fmt_b;          // DTP_FP8_*: e4m3 x e4m3 or e5m2 x e4m3
  int out_dtype;             // DTP_DT_* of C
  int act;                   // 1: LeakyReLU(slope) on the result
  int accumulate;            // 1: C += result
  float slope;
  int instance;              // 0: by K; 1: the pipelined block-scaled MFMA kernel; 2: the short-K one (probes)
  int splitk;                // as DtpGemmFp8Args: 0 planned, 1 unsplit, S > 1 forced (pipelined instance only)
  void* work;                // 4 S M N bytes
  long long work_bytes;
};
// C[M,N] (+)= epilogue(sum_k A(m,k) 2^(sa(m,k/32)-127) B(n,k) 2^(sb(n,k/32)-127)), fp32 accumulation
int dtp_gemm_mxfp8(const DtpGemmMxArgs* a, void* stream);
long long dtp_gemm_mxfp8_workspace(const DtpGemmMxArgs* a);  // as dtp_gemm_fp8_workspace

// sampler probe (tests): dataset indices of steps [t0, t0+n_steps), row-major [n_steps][batch], -1 padded
int dtp_sampler_indices(const dtp::SamplerCfg* s, long long t0, int n_steps, int* out, void* stream);

}  // extern "C"

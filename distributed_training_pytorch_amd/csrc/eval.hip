// Held-out evaluation: forward + per-sample loss + reduction for n_models MLPs of one
// shape in ONE launch (blockIdx.y = model).  One lane per sample as in the stage forward
// (mlp_stage.hip: stage_fwd_body); the workgroup stages its model's weights in LDS once and
// grid-strides over its rows.  Per-sample losses are fp32 (the train kernels' forms); from
// the lane's running sum on everything is fp64 in a fixed order: lane sum -> wave butterfly
// -> LDS -> one value per workgroup.  No atomics and no "last block" counter: up to
// kOneLaunchRows rows one workgroup per model finishes in the same launch, beyond that the
// workgroups write partials to ws and a one-workgroup launch adds them in index order.  The
// grid depends on (n, n_models) only, so out is a pure function of the arguments.
#include "dtp_api.h"
#include "mlp_core.h"
#include "mlp_shapes.h"

namespace dtp {

// Every toy set (512 validation rows by default, the 512-row training set, 4096 rows) takes
// the one-launch path: one workgroup per model walks up to 16 chunks of 256 rows, about
// 1.4 us each on the toy shape (25 us at 4096 rows, where the partial + finalize pair does
// 65536 rows in 15 us: profiles/eval/README.md).  4096 is the smallest limit that keeps
// those sets on one launch; a larger one would only lengthen the one-workgroup walk.
constexpr long long kOneLaunchRows = 4096;
constexpr int kEvalRowsPerBlock = 4 * kBlock;  // partial launch: rows per workgroup before the grid saturates
constexpr int kEvalMaxBlocks = 256;            // per model: one workgroup per CU; the finalize adds at most this many partials

DTP_HD int eval_blocks(long long n) {
  if (n <= kOneLaunchRows) return 1;
  const long long nb = (n + kEvalRowsPerBlock - 1) / kEvalRowsPerBlock;
  return nb < kEvalMaxBlocks ? (int)nb : kEvalMaxBlocks;
}

DTP_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// gridDim.x == 1: out[y] = {loss sum, correct}; else ws[y][blockIdx.x] = this workgroup's pair
template <class S>
__global__ __launch_bounds__(kBlock) void mlp_eval_kernel(DtpEvalArgs a) {
  __shared__ __align__(16) float sw[S::pad4(S::LP)];
  __shared__ double red[2][kBlock / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int y = blockIdx.y;
  const float* prm = a.params + (size_t)y * S::P;
  for (int p = tid; p < S::P; p += kBlock) lds_store_param<S>(sw, p, prm[p]);
  __syncthreads();
  const bool ce = a.loss == DTP_LOSS_CE;
  double lsum = 0.0;
  int hits = 0;
  for (long long k = (long long)blockIdx.x * kBlock + tid; k < a.n; k += (long long)gridDim.x * kBlock) {
    // the weights are loop invariant: left alone, the compiler hoists every layer's LDS reads
    // out of the row loop and holds all of them in registers (256 VGPRs, and 1.5-2 KB of
    // scratch per lane at hidden = 15); behind this barrier each row re-reads them as LDS
    // broadcasts, layer by layer, like the stage forward
    asm volatile("" ::: "memory");
    const long long row = a.row0 + k * a.row_stride;
    const float* x = a.X + (size_t)row * S::IN;
    float h[S::NL + 1][16];
    static_for<0, S::IN>([&](auto IC) { h[0][decltype(IC)::value] = S::rnd(x[decltype(IC)::value]); });
    mlp_forward<S>(sw, h, a.slope);
    float l;
    if (ce) {
      // max-subtracted log-sum-exp minus the target logit (the fused step's form; the precise
      // expf / logf: this value is reported, not only differentiated)
      const int cls = (int)a.Y[row];
      float mx = h[S::NL][0];
      int am = 0;
      static_for<1, S::OUT>([&](auto JC) {
        constexpr int j = decltype(JC)::value;
        const float o = h[S::NL][j];
        am = o > mx ? j : am;  // strict: the lowest index wins a tie
        mx = fmaxf(mx, o);
      });
      float se = 0.f, zc = 0.f;
      static_for<0, S::OUT>([&](auto JC) {
        constexpr int j = decltype(JC)::value;
        se += expf(h[S::NL][j] - mx);
        zc = (j == cls) ? h[S::NL][j] : zc;
      });
      l = (mx + logf(se)) - zc;
      hits += am == cls ? 1 : 0;
    } else {
      const float* t = a.Y + (size_t)row * S::OUT;
      l = 0.f;
      static_for<0, S::OUT>([&](auto JC) {
        constexpr int j = decltype(JC)::value;
        const float d = h[S::NL][j] - t[j];
        l = fmaf(d, d, l);
      });
    }
    lsum += (double)l;
  }
  const double ws0 = wave_sum_f64(lsum), ws1 = wave_sum_f64((double)hits);
  if (lane == 0) {
    red[0][wave] = ws0;
    red[1][wave] = ws1;
  }
  __syncthreads();
  if (tid < 2) {
    double s = red[tid][0];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) s += red[tid][w];
    double* dst = gridDim.x == 1 ? a.out + (size_t)y * 2 : a.ws + ((size_t)y * gridDim.x + blockIdx.x) * 2;
    dst[tid] = s;
  }
}

// one workgroup: thread t adds the nblk partials of out element t (= model t / 2, value t % 2)
// in index order
__global__ __launch_bounds__(kBlock) void mlp_eval_finalize_kernel(const double* __restrict__ ws, double* __restrict__ out,
                                                                   int n_models, int nblk) {
  for (int e = threadIdx.x; e < 2 * n_models; e += kBlock) {
    const double* p = ws + (size_t)(e >> 1) * nblk * 2 + (e & 1);
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += p[(size_t)b * 2];
    out[e] = s;
  }
}

}  // namespace dtp

namespace {
using dtp::check_launch;
using dtp::set_err;

template <class S>
int launch_eval(const DtpEvalArgs* a, hipStream_t st) {
  const int nblk = dtp::eval_blocks(a->n);
  hipLaunchKernelGGL((dtp::mlp_eval_kernel<S>), dim3(nblk, a->n_models), dim3(dtp::kBlock), 0, st, *a);
  if (nblk > 1)
    hipLaunchKernelGGL(dtp::mlp_eval_finalize_kernel, dim3(1), dim3(dtp::kBlock), 0, st, (const double*)a->ws, a->out,
                       a->n_models, nblk);
  return check_launch("mlp_eval_kernel");
}

// one row of the shared shape lists (mlp_shapes.h): the rows that end without an activation
// have an evaluation kernel, the others (layer-split stages inside the network) instantiate
// nothing
template <int I, int H, int N, int O, bool F, bool BF>
int launch_eval_shape(const DtpEvalArgs* a, hipStream_t st) {
  if constexpr (F) {
    return set_err(-2, "mlp eval shape not instantiated");
  } else {
    return launch_eval<dtp::Stage<I, H, N, O, false, BF>>(a, st);
  }
}
}  // namespace

extern "C" {

long long dtp_mlp_eval_one_launch_rows(void) { return dtp::kOneLaunchRows; }

long long dtp_mlp_eval_ws_bytes(long long n, int n_models) {
  if (n <= dtp::kOneLaunchRows || n_models <= 0) return 0;
  return (long long)dtp::eval_blocks(n) * n_models * 2 * (long long)sizeof(double);
}

int dtp_mlp_eval(const DtpEvalArgs* a, int in, int h, int nl, int out, void* stream) {
  if (!a) return set_err(-1, "mlp_eval: null arguments");
  if (!a->out || !a->params || a->n_models < 1 || a->n_models > 65535)
    return set_err(-1, "mlp_eval: params, out and 1..65535 models are required");
  if (a->n < 0 || a->row0 < 0 || a->row_stride < 1) return set_err(-1, "mlp_eval: n >= 0, row0 >= 0 and row_stride >= 1");
  if (a->loss != DTP_LOSS_MSE && a->loss != DTP_LOSS_CE) return set_err(-1, "mlp_eval: loss must be DTP_LOSS_MSE or DTP_LOSS_CE");
  hipStream_t st = (hipStream_t)stream;
  const bool known = dtp_mlp_supported(in, h, nl, out, 0) && (!a->bf16 || dtp_mlp_supported_bf16(in, h, nl, out, 0));
  if (!known) return set_err(-2, a->bf16 ? "no bf16 instance of this mlp eval shape" : "mlp eval shape not instantiated");
  if (a->n == 0) {  // nothing reads X: the sums are zero
    if (hipMemsetAsync(a->out, 0, (size_t)a->n_models * 2 * sizeof(double), st) != hipSuccess)
      return set_err(-3, "mlp_eval: hipMemsetAsync failed");
    return 0;
  }
  if (!a->X || !a->Y) return set_err(-1, "mlp_eval: X and Y are required when n > 0");
  if (dtp_mlp_eval_ws_bytes(a->n, a->n_models) > 0 && !a->ws)
    return set_err(-5, "mlp_eval: more rows than one launch takes need the workspace");
  if (a->bf16) {
#define X(I, H, N, O, F) \
  if (!F && in == I && h == H && nl == N && out == O) return launch_eval_shape<I, H, N, O, F, true>(a, st);
    DTP_STAGE_BF16_SHAPES(X)
#undef X
    return set_err(-2, "no bf16 instance of this mlp eval shape");
  }
#define X(I, H, N, O, F) \
  if (!F && in == I && h == H && nl == N && out == O) return launch_eval_shape<I, H, N, O, F, false>(a, st);
  DTP_STAGE_SHAPES(X)
#undef X
  return set_err(-2, "mlp eval shape not instantiated");
}

}  // extern "C"

// Optimizer math shared by the fused train-step kernel and the flat optimizer
// kernel.  Mirrors torch.optim.Adam / torch.optim.SGD (defaults used by the
// reference: Adam(lr=1e-3), demo.py:80-81) element for element:
//   Adam:  m.lerp_(g, 1-b1); v.mul_(b2).addcmul_(g, g, 1-b2);
//          denom = sqrt(v)/sqrt(1-b2^t) + eps; p.addcdiv_(m, denom, -lr/(1-b1^t))
//   AdamW (hp.decoupled_wd): p.mul_(1 - lr * wd) ahead of Adam's update, wd not in g
//   SGD :  buf = g (first step) | buf*mom + g;  p.add_(buf, -lr)
// with the scalar bias corrections formed in double, as torch does on the host.
#pragma once
#include "dtp_api.h"
#include "dtp_common.h"

namespace dtp {

struct AdamScalars {
  float step_size, bc2_sqrt, one_m_b1, b2, one_m_b2, eps, wd;
  // AdamW (hp.decoupled_wd with a weight_decay != 0): decoupled = 1, wd = 0 -- the decay does not
  // enter the gradient -- and decay = d_t = (float)(1.0 - lr_t * weight_decay), the factor of p
  // ahead of the update.  Else decoupled = 0, decay = 1 and wd as it always was.
  float decay;
  int decoupled;
};

// the learning rate of the step taken after t steps (t = the step counter before the step,
// 0-based): the schedule's table entry, its last one for ever past its end; no table: hp.lr
DTP_DEV double lr_of(const DtpHyper& hp, long long t) {
  if (!hp.lr_tab || hp.lr_tab_len <= 0) return hp.lr;  // (an empty table is never read)
  return hp.lr_tab[t < hp.lr_tab_len ? t : hp.lr_tab_len - 1];
}

// AdamW's factor of p for a step at rate lr: 1 - lr * weight_decay in f64 as torch forms it on the
// host -- a product, then a difference, whatever -ffp-contract the including source builds with --
// rounded to fp32 once.
DTP_DEV float decoupled_decay(const DtpHyper& hp, double lr) {
#pragma clang fp contract(off)
  const double prod = lr * hp.weight_decay;
  return (float)(1.0 - prod);
}

// is this launch AdamW's?  weight_decay == 0 with the flag is plain Adam, to the instruction
DTP_DEV bool decoupled_on(const DtpHyper& hp) { return hp.decoupled_wd != 0 && hp.weight_decay != 0.0; }

// wd / decay / decoupled of the scalars for a step at rate lr
DTP_DEV void adam_decay_fields(AdamScalars& s, const DtpHyper& hp, double lr) {
  s.decoupled = decoupled_on(hp) ? 1 : 0;
  s.wd = s.decoupled ? 0.f : (float)hp.weight_decay;
  s.decay = s.decoupled ? decoupled_decay(hp, lr) : 1.f;
}

DTP_DEV AdamScalars adam_scalars(const DtpHyper& hp, long long t1) {
  AdamScalars s;
  const double bc1 = 1.0 - pow_int(hp.beta1, (uint64_t)t1);
  const double bc2 = 1.0 - pow_int(hp.beta2, (uint64_t)t1);
  const double lr = lr_of(hp, t1 - 1);
  s.step_size = (float)(lr / bc1);
  s.bc2_sqrt = (float)sqrt(bc2);
  s.one_m_b1 = (float)(1.0 - hp.beta1);
  s.b2 = (float)hp.beta2;
  s.one_m_b2 = (float)(1.0 - hp.beta2);
  s.eps = (float)hp.eps;
  adam_decay_fields(s, hp, lr);
  return s;
}

// same, from carried powers b1t = beta1^t, b2t = beta2^t (t = the new step number)
DTP_DEV AdamScalars adam_scalars_from_pow(const DtpHyper& hp, double b1t, double b2t) {
  AdamScalars s;
  const double bc1 = 1.0 - b1t, bc2 = 1.0 - b2t;
  s.step_size = (float)(hp.lr / bc1);
  s.bc2_sqrt = (float)sqrt(bc2);
  s.one_m_b1 = (float)(1.0 - hp.beta1);
  s.b2 = (float)hp.beta2;
  s.one_m_b2 = (float)(1.0 - hp.beta2);
  s.eps = (float)hp.eps;
  s.wd = (float)hp.weight_decay;
  return s;
}

// the step-independent part of the scalars (step_size / bc2_sqrt filled by the caller; decay is
// that of hp.lr: the kernels that use these decay through decoupled_decay_step below)
DTP_DEV AdamScalars adam_consts(const DtpHyper& hp) {
  AdamScalars s;
  s.step_size = 0.f;
  s.bc2_sqrt = 1.f;
  s.one_m_b1 = (float)(1.0 - hp.beta1);
  s.b2 = (float)hp.beta2;
  s.one_m_b2 = (float)(1.0 - hp.beta2);
  s.eps = (float)hp.eps;
  adam_decay_fields(s, hp, hp.lr);
  return s;
}

// Every fused multiply-add is spelled out (fmaf) and the translation units that
// use these helpers build with -ffp-contract=off (build.py), so the rounding of
// each update is fixed by the source, not by how the compiler scheduled the
// surrounding kernel: every kernel instance (FAST or generic, fused step or flat
// optimizer) produces bitwise the same update.
// DTP_ADAM_FAST (default): sqrt(v) from the hardware square root, and each division as
// a reciprocal estimate, a product and one residual correction (fma) -- within an ulp or
// two of the correctly rounded results (the torch.optim.Adam comparisons of the GPU tests
// hold at their tolerances, down to rtol 1e-6 for the flat optimizer), and a short
// dependency chain: the precise forms (v_div_scale / fmas / fixup, the scaled sqrt
// refinement) were ~30 dependent VALU ops per parameter and 0.16 us of the 4.3 us fused
// step (profiles/r4_adam/).  -DDTP_ADAM_FAST=0 restores torch's exact division / sqrt.
#ifndef DTP_ADAM_FAST
#define DTP_ADAM_FAST 1
#endif

// a / b for a normal, positive b: reciprocal estimate, product, one residual correction
DTP_DEV float div_nr(float a, float b) {
  const float r = __builtin_amdgcn_rcpf(b);
  const float q = a * r;
  return fmaf(fmaf(-b, q, a), r, q);
}

DTP_DEV void adam_update(float& p, float& m, float& v, float g, const AdamScalars& s) {
  if (s.wd != 0.f) g = fmaf(s.wd, p, g);
  m = fmaf(s.one_m_b1, g - m, m);                  // m.lerp_(g, 1 - b1)
  v = fmaf(s.one_m_b2 * g, g, v * s.b2);           // v.mul_(b2).addcmul_(g, g, 1 - b2)
#if DTP_ADAM_FAST
  const float denom = div_nr(__builtin_amdgcn_sqrtf(v), s.bc2_sqrt) + s.eps;
  p = fmaf(-s.step_size, div_nr(m, denom), p);
#else
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = fmaf(-s.step_size, m / denom, p);            // p.addcdiv_(m, denom, -step_size)
#endif
}

// The flat optimizer and the stage backward fused with it run their Adam loops in two versions
// behind one block-uniform test (decoupled_on): DEC = false is the loop as it was before AdamW
// existed -- wd as always, no decay factor alive -- so a launch with weight_decay == 0 or the
// coupled decay executes what it did; DEC = true is AdamW: p *= d_t, then Adam's update on the
// decayed p with the gradient as it arrived (wd = 0).  d_t is the step's own
// (adam_scalars: lr_of by the device step counter) and block-uniform: kept in a scalar register.
template <bool DEC>
DTP_DEV AdamScalars adam_scalars_v(const DtpHyper& hp, long long t1) {
  AdamScalars s = adam_scalars(hp, t1);
  if constexpr (DEC) {
    s.wd = 0.f;
    s.decoupled = 1;
    s.decay = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, s.decay)));
  } else {
    s.wd = (float)hp.weight_decay;
    s.decoupled = 0;
    s.decay = 1.f;
  }
  return s;
}

template <bool DEC>
DTP_DEV void adamw_update_v(float& p, float& m, float& v, float g, const AdamScalars& s) {
  if constexpr (DEC) p *= s.decay;
  adam_update(p, m, v, g, s);
}

// AdamW in the kernels that keep a thread's parameters in registers over the steps of a launch
// (the fused step, the layer-split stages): the decay of the step taken after t steps on all of
// a thread's slots, ahead of the unrolled adam_update calls, behind ONE block-uniform branch per
// step and with no state carried from step to step -- nested inside adam_update, with the rate
// requested early in the step behind a branch of its own, it cost the default launch 0.085 us
// of its 2.59 us step (profiles/adamw).  The rate comes from lr_of (a per-step row
// {lr_t / (1 - b1^t), ...} does not give lr_t back): under a schedule one read of the device
// table, on the decoupled path only; without one, hp.lr.
template <int N>
DTP_DEV void decoupled_decay_step(const DtpHyper& hp, const AdamScalars& s, long long t, float (&p)[N]) {
  if (s.decoupled) {
    const float d = decoupled_decay(hp, lr_of(hp, t));
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] *= d;
  }
}

// torch.nn.utils.clip_grad_norm_'s coefficient from the fp32 total norm, operation for
// operation: clip_coef = max_norm / (total_norm + 1e-6) is Tensor.__rtruediv__, i.e.
// (total_norm + 1e-6).reciprocal() * max_norm, then clamp(max=1.0).  Correctly rounded
// division (not div_nr): the coefficient is bitwise torch's.  A NaN norm gives a NaN
// coefficient and an infinite one 0, as torch with error_if_nonfinite=False.
DTP_DEV float clip_coef(float norm, float max_norm) {
  const float r = 1.0f / (norm + 1e-6f);
  const float c = r * max_norm;
  return c > 1.0f ? 1.0f : c;
}

// torch.nn.utils.clip_grad_value_: g.clamp_(-c, c); NaN stays NaN
DTP_DEV float clamp_value(float g, float c) { return g < -c ? -c : (g > c ? c : g); }

DTP_DEV void sgd_update(float& p, float& buf, float g, float lr, float mom, float wd, bool first) {
  if (wd != 0.f) g = fmaf(wd, p, g);
  if (mom != 0.f) {
    buf = first ? g : fmaf(buf, mom, g);
    g = buf;
  }
  p = fmaf(-lr, g, p);
}

}  // namespace dtp

// Gradient accumulation inside the several-lanes / split-batch step (mlp_train_lanes.hip):
// the accumulation twins of the update instances.
//
// One optimizer step of an accumulating launch (DtpTrainArgs.accum = A > 1) consumes the A
// consecutive batches t A .. t A + A - 1 of the rank's sampler order.  The dW tiles of the step
// are MFMA accumulators and the weights sit in LDS unchanged until the update, so a micro-batch
// that is not the last of its window is the step's forward, loss and backward into the same
// accumulators and nothing else: no park, no barrier, no exchange, no update, no weight
// scatter.  The step's tail -- the waves' sums, the split-batch members' and the ranks'
// exchange, clipping, the update, the scatter, the loss log -- runs once per window.
//
//   gradient : sum_j grad(mean_loss_j) in the accumulators; the 1/A reaches it through
//              hp.grad_scale (the host folds it in: 1 / A locally, 1 / (world A) for xGMI)
//   loss     : every micro-batch stages lpart * inv_j (its own 1 / size: an epoch's ragged
//              batch is divided by its own count), so the loss cell holds sum_j mean_loss_j
//              and the logged value is that sum times hp.grad_scale
//   clipping : inside the twin behind a wave-uniform run-time branch (off / by norm / by value,
//              clip_core.h), so accumulation and clipping combine without further instances
//
// The twin is a bit on the kernel's MODE template argument (kModeAccum), next to kModeClip:
// the plain instances and the clip twins keep their names and their device code.
#pragma once
#include "clip_core.h"

namespace dtp {

// internal: MODE | kModeAccum instantiates the accumulation twin of an update mode
constexpr int kModeAccum = 16;
constexpr bool mode_accum(int mode) { return (mode & kModeAccum) != 0; }
static_assert(mode_base(DTP_MODE_XGMI_SGD | kModeAccum | kModeClip) == DTP_MODE_XGMI_SGD, "the twin bits sit above the modes");

}  // namespace dtp

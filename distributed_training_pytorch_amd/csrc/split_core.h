// Parts of one layer-split stage step that every stage body has: split_stage_body_v1 and
// split_stage_body_pipe (split_train.hip), split_lanes_body (split_lanes.hip).  Included by
// those two sources only; their kernels' code is what it was with the parts written out in
// each body (profiles/split_core/README.md).
#pragma once
#include "dtp_api.h"
#include "dtp_common.h"
#include "optim_core.h"

namespace dtp {

// cache policy of a link: sc1 = device scope (both stages on one GPU: the granules meet in
// the device's last-level cache, no round trip to HBM), sc0 | sc1 = system scope
// (kSysCoherent: neighbour on another GPU, uncached fine-grained buffer written over xGMI)
constexpr int kDevCoherent = 16;

// The per-step optimizer scalars of the next kSplitAdamTab steps, formed once per that many
// steps in f64 (torch's host math) -- not per step.  Row of step t0 + base + e + 1:
// {lr / (1 - b1^t), sqrt(1 - b2^t)} under Adam, {lr_t, 1} under SGD with a schedule.
constexpr int kSplitAdamTab = 1024;

// The optimizer step `it` of the launch on a thread's NPT parameter slots (registers), from
// the step's row of the table `tab`.  The statements keep the order and the places they had
// in the bodies: each branch forms the row's address itself (one address formed ahead of the
// branch moved split_train.hip's kernels), and the SGD branch reads the row itself.
// ROW_LATE: the Adam branch reads the row too (split_train.hip's bodies); else
// its scalars arrive in adam_sc, read before the gradient sums (split_lanes_body).  GUARD:
// only the slots with slot[k] >= 0 update (split_stage_body_v1, whose unowned slots have no
// sink to store to).  t: the step counter before this step (AdamW's rate: decoupled_decay_step).
template <bool ROW_LATE, bool GUARD, int NPT>
DTP_DEV void split_optim_step(const DtpHyper& hp, bool adam, float2 adam_sc, const float2 (&tab)[kSplitAdamTab], int it,
                              int t, bool first_step, float gs, const int (&slot)[NPT], float (&pw)[NPT], float (&mr)[NPT],
                              float (&vr)[NPT], const float (&g)[NPT]) {
  if (adam) {
    AdamScalars as = adam_consts(hp);
    if constexpr (ROW_LATE) {
      const float2 sc = tab[it % kSplitAdamTab];
      as.step_size = sc.x;
      as.bc2_sqrt = sc.y;
    } else {
      as.step_size = adam_sc.x;
      as.bc2_sqrt = adam_sc.y;
    }
    decoupled_decay_step(hp, as, t, pw);  // AdamW: p *= d_t (every slot: the unowned ones are never stored)
#pragma unroll
    for (int k = 0; k < NPT; ++k)
      if (!GUARD || slot[k] >= 0) adam_update(pw[k], mr[k], vr[k], g[k] * gs, as);
  } else {
    const float lr = hp.lr_tab ? tab[it % kSplitAdamTab].x : (float)hp.lr, mom = (float)hp.momentum, wd = (float)hp.weight_decay;
#pragma unroll
    for (int k = 0; k < NPT; ++k)
      if (!GUARD || slot[k] >= 0) sgd_update(pw[k], mr[k], g[k] * gs, lr, mom, wd, first_step);
  }
}

}  // namespace dtp

// The layer-split stage shapes and the launch check that both engines share: split_train.hip
// (one workgroup per stage) and split_lanes.hip (M member workgroups per stage).
#pragma once
#include <string>

#include "dtp_api.h"
#include "dtp_common.h"
#include "xgmi_core.h"

// (IN, H, NL, OUT, FINAL_ACT, FIRST): the contiguous layer ranges of the toy model as
// pipeline stages.  The first entry is the whole model as ONE stage: the split code's
// baseline with no links (scripts/split_cost.py).  First stages read the 2-feature input;
// stages that end inside the network carry the LeakyReLU of their last layer and are not
// last.  The shape id of a stage is its position in this list, in both engines.
#define DTP_SPLIT_SHAPES(X)   \
  X(2, 10, 5, 1, false, 1)    \
  X(2, 10, 1, 10, true, 1)    \
  X(2, 10, 2, 10, true, 1)    \
  X(2, 10, 3, 10, true, 1)    \
  X(2, 10, 4, 10, true, 1)    \
  X(10, 10, 1, 10, true, 0)   \
  X(10, 10, 2, 10, true, 0)   \
  X(10, 10, 3, 10, true, 0)   \
  X(10, 10, 1, 1, false, 0)   \
  X(10, 10, 2, 1, false, 0)   \
  X(10, 10, 3, 1, false, 0)   \
  X(10, 10, 4, 1, false, 0)

namespace dtp {

struct SplitShape {
  int in, h, nl, out;
  bool final_act, first;
  constexpr bool last() const { return !final_act; }
};

constexpr SplitShape kSplitShapes[] = {
#define X(I, H, N, O, F, FI) {I, H, N, O, F, (bool)FI},
    DTP_SPLIT_SHAPES(X)
#undef X
};
constexpr int kSplitNumShapes = sizeof(kSplitShapes) / sizeof(kSplitShapes[0]);

// What both launch checks ask of one stage; `who` is the engine's message prefix and
// `members` its workgroups per stage (1: one workgroup).  Each engine adds what is its own.
inline int split_check_stage(const DtpSplitStageArgs& a, const SplitShape& sh, const char* who, int members) {
  const auto refuse = [&](const char* what) { return set_err(-1, (std::string(who) + ": " + what).c_str()); };
  const bool first = sh.first, last = sh.last();
  if (!a.params || !a.opt_m || !a.step || !a.status) return refuse("missing buffers");
  if (a.n_steps <= 0) return refuse("n_steps must be positive");
  if (a.optim != DTP_MODE_ADAM && a.optim != DTP_MODE_SGD) return refuse("adam or sgd");
  if (a.optim == DTP_MODE_ADAM && !a.opt_v) return refuse("Adam needs opt_v");
  if (a.hp.decoupled_wd && a.optim != DTP_MODE_ADAM)
    return refuse("decoupled weight decay (AdamW) is Adam's: SGD has no decoupled form");
  if (first && !a.X) return refuse("the first stage needs the inputs");
  if (last && !a.Y) return refuse("the last stage needs the targets");
  if (!first && (!a.act_in || !a.grad_out)) return refuse("missing links to the previous stage");
  if (!last && (!a.act_out || !a.grad_in)) return refuse("missing links to the next stage");
  if (last && a.loss_log && a.loss_log_cap <= 0) return refuse("loss_log_cap");  // the kernels log at t % cap
  if (a.dp_world > 1 && (!a.dp_peers || a.dp_world * members > kXgmiMaxWorld || a.dp_rank < 0 || a.dp_rank >= a.dp_world))
    return refuse("the cross-rank exchange serves ranks x members <= 8 with a peer table");
  return 0;
}

}  // namespace dtp

// The fused train step with several lanes per sample (mlp_lanes.h), for gfx950 (MI355X): its
// plain instances and its instance table.
//
//   mlp_train_lanes_kernel : (mlp_train_lanes_kernel.h) the step for per-rank batches <= 256 / L
//                            (L = 2 or 4 lanes per sample, 4 or 8 waves), and the split-batch
//                            step: a larger batch over several such workgroups per model, their
//                            gradients summed on chip (grp_core.h) or across GPUs too
//                            (xgmi_core.h).  Instantiated here in its plain variant; the clip
//                            and accumulation twins of the instances are compiled in
//                            mlp_train_lanes_clip.hip and mlp_train_lanes_accum.hip.
//   lanes_inst()           : the lookup mlp_train.hip dispatches through, over the table of the
//                            (shape, precision, loss, optimizer) families (DTP_LANES_FAMILIES).
#include <array>

#include "mlp_train_lanes_kernel.h"

namespace dtp {

// a family's row: its plain variant, and the 8-wave, A/B and PROF instances, which have no twins
template <class S, bool CE, bool SGD, bool W8, bool GRP, bool EXTRA>
constexpr LanesInst lanes_row() {
  constexpr int M = SGD ? DTP_MODE_SGD : DTP_MODE_ADAM, XM = SGD ? DTP_MODE_XGMI_SGD : DTP_MODE_XGMI_ADAM;
  LanesInst r{S::IN, S::H, S::NL, S::OUT, S::BF, CE, SGD};
  lanes_fill<S, CE, SGD, GRP, kPlain>(r);
  if constexpr (W8) {
    r.lanes[kPlain][1][0][0] = &launch_lanes<S, 2, M, 8, CE>, r.lanes[kPlain][1][0][1] = &launch_lanes<S, 2, XM, 8, CE>;
    r.lanes[kPlain][1][1][0] = &launch_lanes<S, 4, M, 8, CE>, r.lanes[kPlain][1][1][1] = &launch_lanes<S, 4, XM, 8, CE>;
  }
  if constexpr (EXTRA) {
    r.grp8 = &launch_lanes<S, 4, M, 8, CE, false, true>;
    r.prof[0][0] = &launch_lanes<S, 2, M, 4, CE, true>, r.prof[0][1] = &launch_lanes<S, 4, M, 4, CE, true>;
    r.prof[1][0] = &launch_lanes<S, 2, M, 8, CE, true>, r.prof[1][1] = &launch_lanes<S, 4, M, 8, CE, true>;
    r.grp_prof[0] = &launch_lanes<S, 4, M, 4, CE, true, true>;
    r.grp_prof[1] = &launch_lanes<S, 4, M, 4, CE, true, true, 4>;
  }
  return r;
}

// the table, assembled at the first lookup: the rows above, then each twin source's variant of
// every row
const LanesInst* lanes_inst(int in, int h, int nl, int out, bool bf16, bool ce, int mode) {
#define X(I, H, N, O, B, CE, SGD, W8, GRP, EXTRA) lanes_row<Stage<I, H, N, O, false, B>, CE, SGD, W8, GRP, EXTRA>(),
  static const auto kLanes = [] {
    std::array rows{DTP_LANES_FAMILIES(X)};
    lanes_fill_clip(rows.data());
    lanes_fill_accum(rows.data());
    return rows;
  }();
#undef X
  if (mode < DTP_MODE_ADAM || mode > DTP_MODE_XGMI_SGD) return nullptr;
  for (const LanesInst& r : kLanes)
    if (r.in == in && r.h == h && r.nl == nl && r.out == out && r.bf16 == bf16 && r.ce == ce && r.sgd == mode_sgd(mode))
      return &r;
  return nullptr;
}

}  // namespace dtp

// The clip twins (clip_core.h) of the several-lanes / split-batch step's 4-wave instances:
// a source of their own, so that the three step variants compile side by side.
#include "mlp_train_lanes_kernel.h"

namespace dtp {

void lanes_fill_clip(LanesInst* rows) { lanes_fill_families<kClip>(rows); }

}  // namespace dtp

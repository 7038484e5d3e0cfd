// The MLP stage shapes the per-sample kernels are instantiated for: one list for the stage
// forward / backward (mlp_stage.hip), dtp_mlp_supported and the evaluation kernel (eval.hip,
// the rows without a final activation), so that what dtp_mlp_supported reports is what every
// one of them can launch.
#pragma once

// (IN, H, NL, OUT, FINAL_ACT): every contiguous layer range of the toy model
// (layer-split stages) plus the train shapes as whole-model stages
#define DTP_STAGE_SHAPES(X) \
  X(2, 10, 5, 1, false)     \
  X(2, 10, 4, 10, true)     \
  X(10, 10, 4, 1, false)    \
  X(2, 10, 3, 10, true)     \
  X(10, 10, 3, 10, true)    \
  X(10, 10, 3, 1, false)    \
  X(2, 10, 2, 10, true)     \
  X(10, 10, 2, 10, true)    \
  X(10, 10, 2, 1, false)    \
  X(2, 10, 1, 10, true)     \
  X(10, 10, 1, 10, true)    \
  X(10, 10, 1, 1, false)    \
  X(2, 10, 3, 1, false)     \
  X(2, 10, 5, 2, false)     \
  X(2, 10, 5, 4, false)     \
  X(2, 15, 5, 1, false)     \
  X(2, 15, 5, 4, false)     \
  X(4, 15, 5, 4, false)

// whole-model shapes that also have bf16-compute instances (autocast / precision='bf16')
#define DTP_STAGE_BF16_SHAPES(X) \
  X(2, 10, 5, 1, false)          \
  X(2, 10, 5, 4, false)

"""The layer-split engines' outputs as digests: ``FusedLayerSplit`` seeded as
``scripts/split_cost.py`` seeds it, K = 2 and K = 3 stages, ``members`` 0 (one workgroup per
stage) and ``"auto"`` (four members at batch 256), Adam and SGD, 40 steps in two launches of
20.  One line per run: the sha256 of the concatenated parameters, both moments and the 40
logged losses.  Run it once with ``DTP_LIB`` pointing at a build of the parent and once on the
tree: every line must be equal.
python profiles/split_core/bitwise_sweep.py"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from distributed_training_pytorch_amd.data.sampler import SamplerGeometry  # noqa: E402
from distributed_training_pytorch_amd.data.toy_data import ToyData  # noqa: E402
from distributed_training_pytorch_amd.ops.mlp import TOY_SPEC  # noqa: E402
from distributed_training_pytorch_amd.ops.optim import OptimConfig  # noqa: E402
from distributed_training_pytorch_amd.parallel.layer_split import FusedLayerSplit  # noqa: E402


def run(K, members, opt):
    dev = torch.device("cuda", 0)
    ds = ToyData(n=512, seed=2)
    init = torch.randn(TOY_SPEC.P, generator=torch.Generator().manual_seed(0)) * 0.4
    cfg = OptimConfig(lr=1e-3) if opt == "adam" else OptimConfig(name="sgd", lr=1e-2, momentum=0.9)
    eng = FusedLayerSplit(TOY_SPEC, [dev] * K, ds.X, ds.Y, SamplerGeometry(n=512, batch=256, seed=1), cfg, init,
                          members=members)
    try:
        eng.train(20)
        eng.train(20)
        eng.synchronize()
        sd = eng.state_dict()
        out = torch.cat([sd["params"], sd["m"], sd["v"], eng.losses(0, 40).reshape(-1)]).contiguous()
        return eng.members, hashlib.sha256(out.numpy().tobytes()).hexdigest(), float(eng.losses(39, 40).reshape(-1)[0])
    finally:
        eng.close()


if __name__ == "__main__":
    for K in (2, 3):
        for members in (0, "auto"):
            for opt in ("adam", "sgd"):
                m, h, last = run(K, members, opt)
                print(json.dumps({"K": K, "members": m, "opt": opt, "sha256": h, "loss39": last}), flush=True)

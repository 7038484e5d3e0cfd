#!/usr/bin/env python3
"""One-off: (lanes, waves, groups) of every answer of the fused step's dispatcher over a grid of
calls, as one sha256 and a count, for the library of the tree it runs in (or the one DTP_LIB
names).  It calls dtp_mlp_train_pick where the library has it, else dtp_mlp_train_lanes, and
prints no variant, so a tree before and after "twins as one table dimension" compare
(profiles/step_variants).  Run once per library and per forcing variable and compare the lines.

The grid also runs over five argument sets: none, max_norm = 0.5, clip_value = 0.01, accum = 4,
accum = 4 with max_norm = 0.5.

Usage: [DTP_LIB=path/libdtp.so] [DTP_LANES=2x8 ...] python profiles/step_table/pick_sweep.py
(from the root of the tree whose library is meant)
"""
import ctypes
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.getcwd())
from distributed_training_pytorch_amd import _native as nat  # noqa: E402

FORCING = ("DTP_LANES", "DTP_FAST", "DTP_GRP_NW", "DTP_GROUPS", "DTP_ACCUM_TWIN")
SHAPES = [(2, 10, 5, 1), (2, 10, 3, 1), (2, 10, 5, 4), (2, 15, 5, 1), (2, 15, 5, 4), (2, 10, 4, 1)]  # last two: absent
BATCHES = (1, 50, 64, 65, 100, 128, 129, 130, 200, 256, 257, 300, 512)
ARGSETS = ((0.0, 0.0, 0), (0.5, 0.0, 0), (0.0, 0.01, 0), (0.0, 0.0, 4), (0.5, 0.0, 4))  # max_norm, clip_value, accum
DUMMY = 0x1000  # no pointer is dereferenced


lib = nat.load()
new_api = hasattr(nat, "StepPick")  # the tree has dtp_mlp_train_pick


def pick(shape, mode, batch, n, world, loss, bf16, groups, cache, max_norm, clip_value, accum):
    a = nat.TrainArgs()
    for f in ("X", "Y", "params", "opt_m", "opt_v", "step", "status", "peers", "epoch", "norm_out", "grad_out"):
        setattr(a, f, DUMMY)
    a.n_models, a.n_steps, a.host_t0 = 2, 1, 0
    a.loss, a.cache_data, a.bf16, a.groups = loss, cache, bf16, groups
    a.max_norm, a.clip_value, a.accum = max_norm, clip_value, accum
    a.hp.slope = 0.01
    s = a.smp
    s.mode, s.perm, s.perm_epochs = nat.SAMPLER_TABLE, DUMMY, 4
    s.n, s.world, s.rank, s.batch = n, world, 0, batch
    s.num_samples = -(-n // world)
    s.steps_per_epoch = -(-s.num_samples // batch)
    if new_api:
        rec = nat.StepPick()
        lib.dtp_mlp_train_pick(ctypes.byref(a), *shape, mode, ctypes.byref(rec))
        return (rec.lanes, rec.waves, rec.groups)
    r = lib.dtp_mlp_train_lanes(ctypes.byref(a), *shape, mode)
    return (r & 255, (r >> 8) & 255, r >> 16)


h, n, hist = hashlib.sha256(), 0, {}
for (mn, cv, ac), shape, mode, loss, bf16, cache, groups, world, size, batch in itertools.product(
        ARGSETS, SHAPES, (1, 2, 3, 4), (0, 1), (0, 1), (0, 1), (-1, 0, 1), (1, 2, 3, 8), (512, 2048), BATCHES):
    r = pick(shape, mode, batch, size, world, loss, bf16, groups, cache, mn, cv, ac)
    h.update(repr(r).encode())
    hist[r] = hist.get(r, 0) + 1
    n += 1
env = " ".join(f"{k}={os.environ[k]}" for k in FORCING if k in os.environ) or "-"
print(f"{env:16s} points {n}  sha256 {h.hexdigest()[:16]}  "
      + "  ".join("%dx%dx%d:%d" % (*k, v) for k, v in sorted(hist.items())))

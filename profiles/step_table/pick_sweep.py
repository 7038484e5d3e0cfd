#!/usr/bin/env python3
"""One-off: every answer of dtp_mlp_train_lanes over a grid of calls, as one sha256 and a
count, for the library DTP_LIB names (default: the in-tree one).  Run once per library and
per forcing variable and compare the lines.

Usage: [DTP_LIB=path/libdtp.so] [DTP_LANES=2x8 ...] python profiles/step_table/pick_sweep.py
"""
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from distributed_training_pytorch_amd import _native as nat  # noqa: E402
from tests.test_step_pick_cpu import FORCING, pick, query  # noqa: E402

SHAPES = [(2, 10, 5, 1), (2, 10, 3, 1), (2, 10, 5, 4), (2, 15, 5, 1), (2, 15, 5, 4), (2, 10, 4, 1)]  # last two: absent
BATCHES = (1, 50, 64, 65, 100, 128, 129, 130, 200, 256, 257, 300, 512)

lib = nat.load()
h, n, hist = hashlib.sha256(), 0, {}
for shape, mode, loss, bf16, cache, groups, world, size, batch in itertools.product(
        SHAPES, (1, 2, 3, 4), (0, 1), (0, 1), (0, 1), (-1, 0, 1), (1, 2, 3, 8), (512, 2048), BATCHES):
    r = tuple(pick(lib, nat, query(shape, mode, batch, size, world, loss, bf16, groups, cache)))
    h.update(repr(r).encode())
    hist[r] = hist.get(r, 0) + 1
    n += 1
env = " ".join(f"{k}={os.environ[k]}" for k in FORCING if k in os.environ) or "-"
print(f"{env:16s} points {n}  sha256 {h.hexdigest()[:16]}  "
      + "  ".join("%dx%dx%d:%d" % (*k, v) for k, v in sorted(hist.items())))

"""Every fused-step kernel instance by its gradient against fp64 (GPU only).

One test per cell of ``tests/step_cases.py``: the dispatcher's pick is asserted, then the
gradient the step formed is read out through the optimizer state at step 0, at the last step of
epoch 0 and at the first step of epoch 1 and held to the bounds of ``tests/step_cases.py``
(fp32: 4 x the error of fp32 torch autograd; CE: plus the intrinsics' margin; bf16: half the
distance between the rounding model and fp32 compute).  Every read-out prints one JSON line
with E, Y and E / Y per tensor; ``profiles/step_matrix/`` keeps the table of one run.

n = 512 (1024 for the batch of 513), two models, steps_per_launch = 3."""
import json
import os
import subprocess
import sys

import pytest
import torch

from . import step_cases as sc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(recs, fails):
    for r in recs:
        print("STEP_MATRIX " + json.dumps(r))
    assert not fails, "\n".join(fails)
    assert recs


@pytest.mark.parametrize("cell", sc.CELLS, ids=[c.id for c in sc.CELLS])
def test_step_gradient_matches_fp64(cell):
    _report(*sc.run_cell(cell, DEV))


_ENVS = sorted({c.env for c in sc.FORCED})


@pytest.mark.parametrize("env", _ENVS, ids=["-".join(f"{k}={v}" for k, v in e) for e in _ENVS])
def test_forced_instance_gradient_matches_fp64(env, tmp_path):
    """DTP_LANES / DTP_FAST / DTP_GRP_NW are read once per process: one fresh child per value
    runs that value's cells (``python -m tests.step_cases``) and writes its records as JSON."""
    out = str(tmp_path / "cells.json")
    ids = [c.id for c in sc.FORCED if c.env == env]
    base = {k: v for k, v in os.environ.items() if k not in ("DTP_LANES", "DTP_FAST", "DTP_GRP_NW", "DTP_GROUPS")}
    r = subprocess.run([sys.executable, "-m", "tests.step_cases", out, *ids], cwd=ROOT, env={**base, **dict(env)},
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as fh:
        res = json.load(fh)
    assert {x["cell"] for x in res["records"]} == set(ids) or res["failures"]
    _report(res["records"], res["failures"])

"""The xGMI exchanges at every world size and step instance (GPU only; all ranks share GPU 0).

Every cross-rank sum goes through ``xgmi_allreduce_kernel`` (``csrc/xgmi_allreduce.hip``),
``xgmi_allreduce_slots`` or ``xgmi_allreduce_g3`` (``csrc/xgmi_core.h``), written for 1..8 ranks.
Here:

* one test per cell of ``step_cases.XGMI_CELLS`` / ``XGMI_FORCED``: the fused step under
  ``DTP_MODE_XGMI_ADAM`` / ``_SGD`` at W = 2, 3, 5 and 8 ranks, its gradient read out through
  the optimizer state on every rank and held to the mean of fp64 autograd over the ranks'
  batches by the bounds of ``tests/step_cases.py`` (``evaluate_step``), with the dispatcher's
  pick, the exchange in use, the step counters and bitwise equality of the read-out, the logged
  loss and the parameters across all ranks;
* the stand-alone all-reduce at 3, 5 and 8 ranks against its exact CPU loop
  (``tests/xgmi_cases.py``), bit for bit;
* at 8 ranks, graph replay against persistent launches, bit for bit.

Starting W processes costs far more than a cell, so the ranks are spawned once per world size
(and once per forced environment) by a module-scoped fixture; the rank function
(``xgmi_cases.world_rank``) runs that world's items in order, stops at the first that raises and
retries nothing.  A cell the spawn did not reach fails as "not run".  Every read-out prints one
``STEP_MATRIX`` JSON line; ``profiles/xgmi_matrix/`` keeps the table of one run."""
import json

import pytest
import torch

from . import step_cases as sc
from . import xgmi_cases as xc
from .dist_utils import run_ranks

pytestmark = pytest.mark.gpu

WORLDS = sorted({c.world for c in sc.XGMI_CELLS})
_ENVS = sorted({c.env for c in sc.XGMI_FORCED})
_spawned: dict = {}


def _spawn(key):
    """{rank: world_rank's result} of the spawn ``key`` = (world, env), run once per module."""
    if key not in _spawned:
        world, env = key
        cells = [c.id for c in (sc.XGMI_FORCED if env else sc.XGMI_CELLS) if c.world == world and c.env == env]
        lost = [k for k, v in _spawned.items() if isinstance(v, BaseException)]
        if lost:  # ranks died or never answered: nothing more is started on that GPU
            _spawned[key] = RuntimeError(f"not started: the spawn of {lost[0]} failed")
        else:
            try:
                _spawned[key] = run_ranks(xc.world_rank, world, (cells, env, world in xc.AR_WORLDS and not env,
                                                                  world == 8 and not env), timeout=300)
            except BaseException as e:  # every test of the spawn reports it
                _spawned[key] = e
    if isinstance(_spawned[key], BaseException):
        raise AssertionError(f"the spawn of {key} failed") from _spawned[key]
    return _spawned[key]


@pytest.fixture(scope="module")
def spawned():
    yield _spawn
    _spawned.clear()


def _report(recs, fails):
    for r in recs:
        print("STEP_MATRIX " + json.dumps(r))
    assert not fails, "\n".join(fails)
    assert recs


@pytest.mark.parametrize("cell", sc.ALL_XGMI, ids=[c.id for c in sc.ALL_XGMI])
def test_xgmi_step_gradient_matches_fp64(cell, spawned):
    res = spawned((cell.world, cell.env))
    stopped = [res[r]["stopped"] for r in sorted(res) if res[r]["stopped"]]
    if any(cell.id not in res[r]["cells"] for r in res):
        pytest.fail(f"{cell.id}: not run; the spawn stopped at\n" + "\n".join(stopped[:1]))
    recs, fails = sc.evaluate_cell_world(cell, {r: res[r]["cells"][cell.id] for r in res})
    _report(recs, fails)


@pytest.mark.parametrize("world", xc.AR_WORLDS)
def test_xgmi_allreduce_standalone_exact(world, spawned):
    """Every call of AR_SIZES on one object, on every rank, equals the CPU loop bit for bit."""
    res = spawned((world, ()))
    outs = {r: res[r]["ar"] for r in res}
    assert all(o is not None for o in outs.values()), [res[r]["stopped"] for r in res]
    for c, n in enumerate(xc.AR_SIZES):
        xs = [xc.ar_payload(world, r, c) for r in range(world)]
        ref = xc.ar_reference(xs, xc.ar_scale(world, c))
        assert outs[0][c].shape == (n,)
        if c == xc.AR_SPECIAL_CALL:
            nan = torch.isnan(ref)
            assert nan.sum() == 4 and torch.isinf(ref).sum() == 3, "the planted values"
            assert torch.equal(torch.isnan(outs[0][c]), nan)
            assert ref[2] == 0 and not torch.signbit(ref[2]) and not torch.signbit(outs[0][c][2])
        else:
            assert torch.equal(outs[0][c], ref), f"call {c} ({n} floats, {xc.ar_kind(c)})"
        assert xc.same_bits(outs[0][c], ref), f"call {c} ({n} floats, {xc.ar_kind(c)})"
        if xc.ar_kind(c) == "int":
            exact = torch.stack([x.long() for x in xs]).sum(0).double() * xc.INT_SCALE
            assert torch.equal(outs[0][c].double(), exact)
        for r in range(1, world):
            assert xc.same_bits(outs[r][c], outs[0][c]), f"call {c}: rank {r} differs from rank 0"
            if c != xc.AR_SPECIAL_CALL:
                assert torch.equal(outs[r][c], outs[0][c])


def test_xgmi_graph_replay_equals_persistent_at_8_ranks(spawned):
    """Seven steps of the 4-lanes toy cell at W = 8 with launch="graph" (steps_per_launch = 4)
    leave the parameters and losses of launch="persistent", bit for bit, on every rank."""
    res = spawned((8, ()))
    assert all(res[r]["graph"] is not None for r in res), [res[r]["stopped"] for r in res][:1]
    cell = sc.XGMI_GRAPH_CELL
    for r in sorted(res):
        g = res[r]["graph"]
        for launch in ("graph", "persistent"):
            comm, why, pick = g[launch + "_comm"]
            assert comm == "xgmi" and why is None and tuple(pick) == cell.expect, (r, launch, comm, why, pick)
        assert torch.equal(g["graph"][0], g["persistent"][0]), f"rank {r}: parameters differ"
        assert torch.equal(g["graph"][1], g["persistent"][1]), f"rank {r}: losses differ"
        assert torch.equal(g["graph"][0], res[0]["graph"]["graph"][0]), f"rank {r}: replicas diverged"
    assert torch.isfinite(res[0]["graph"]["graph"][1]).all()

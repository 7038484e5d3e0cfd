"""Every layer-split stage instance by its gradient against fp64 autograd (GPU only; all stages,
members and ranks share GPU 0).

One test per cell of ``tests/split_cases.py``: a ``FusedLayerSplit`` engine on the one-workgroup
stages (``csrc/split_train.hip``) or the member stages (``csrc/split_lanes.hip``), its gradient
read out through the optimizer state at step 0, at the last step of epoch 0 and at the first of
epoch 1, held per parameter tensor to ``E <= max(4 Y, 8 * 2^-24)`` together with the logged loss,
the applied update, the stages' step counters and ``check_comm()``.  Before it trains a cell
asserts the member count, the link kind and every stage's shape id.  The cells of several ranks
are spawned once per world size; a cell the spawn did not reach fails as "not run".  Every
read-out prints one ``SPLIT_MATRIX`` JSON line; ``profiles/split_matrix/`` keeps the table of one
run."""
import pytest
import torch

from . import split_cases as sp
from .dist_utils import run_ranks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_spawned: dict = {}


def _report(recs, fails):
    sp.report(recs)
    assert not fails, "\n".join(fails)
    assert recs


@pytest.mark.parametrize("cell", sp.CELLS, ids=[c.id for c in sp.CELLS])
def test_split_step_gradient_matches_fp64(cell):
    if cell.launch == "per_stage":
        from distributed_training_pytorch_amd import _native as nat

        if len(nat.stream_priority_levels(DEV)) < 2:
            pytest.skip("one stream priority level")
    recs, fails = sp.run_cell(cell, DEV)
    _report(recs, fails)
    assert len(recs) == len(sp.readout_steps(cell))


def _spawn(world):
    """{rank: world_rank's result} of one world size, run once per module."""
    if world not in _spawned:
        lost = [k for k, v in _spawned.items() if isinstance(v, BaseException)]
        if lost:  # ranks died or never answered: nothing more is started on that GPU
            _spawned[world] = RuntimeError(f"not started: the spawn of W = {lost[0]} failed")
        else:
            try:
                _spawned[world] = run_ranks(sp.world_rank, world, ([c.id for c in sp.WORLD_CELLS if c.world == world],),
                                            timeout=300)
            except BaseException as e:  # every test of the spawn reports it
                _spawned[world] = e
    if isinstance(_spawned[world], BaseException):
        raise AssertionError(f"the spawn of W = {world} failed") from _spawned[world]
    return _spawned[world]


@pytest.fixture(scope="module")
def spawned():
    yield _spawn
    _spawned.clear()


@pytest.mark.parametrize("world", sp.WORLDS)
def test_split_step_gradient_matches_fp64_over_ranks(world, spawned):
    """Every cell of this world size: the read-out, the logged loss and the parameters
    ``torch.equal`` across the ranks, rank 0's read-out within the bounds against the mean of fp64
    autograd over the ranks' batches."""
    res = spawned(world)
    stopped = [res[r]["stopped"] for r in sorted(res) if res[r]["stopped"]]
    fails, n = [], 0
    for cell in (c for c in sp.WORLD_CELLS if c.world == world):
        if any(cell.id not in res[r]["cells"] for r in res):
            fails.append(f"{cell.id}: not run; the spawn stopped at " + "; ".join(stopped[:1]))
            continue
        recs, f = sp.evaluate_world(cell, {r: res[r]["cells"][cell.id] for r in res})
        sp.report(recs)
        n += len(recs)
        fails += f
    assert not fails, "\n".join(fails)
    assert n == 3 * sum(c.world == world for c in sp.WORLD_CELLS)

"""The CPU side of the layer-split matrix (``tests/split_cases.py``): the conditions every
cell's inputs must meet for its bound to mean something, the cell table against the list of
stage instances, and the evaluation against read-outs that are wrong in the ways a split engine
can be wrong."""
import functools

import pytest
import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream

from . import split_cases as sp
from . import step_cases as sc
from .ref_train import torch_train


@functools.lru_cache(maxsize=None)
def _trajectory(opt, batch, n, world):
    """(t, parameters [1, P]) before each read-out step of a configuration along the torch
    reference (``ref_train.torch_train``: autograd + torch.optim, one geometry per rank), shared
    by the cells that differ only in partition, engine, members, links or launch."""
    cell = sp.SplitCell(sp.REF, opt, batch, n=n, world=world)
    X, Y = sp.cell_data(cell)
    geoms = [EpochIndexStream(sp.cell_geom(cell, r)) for r in range(world)]
    out = []
    for t in sp.readout_steps(cell):
        p, _ = torch_train(cell.spec, sp.cell_init(cell)[:1], X, Y, geoms, t, sp.ADAM if opt == "adam" else sp.SGD)
        out.append((t, p))
    return out


_CONFIGS = sorted({(c.opt, c.batch, c.n, c.world) for c in sp.ALL_CELLS})


@pytest.mark.parametrize("opt,batch,n,world", _CONFIGS, ids=[f"{o}-b{b}-n{n}-w{w}" for o, b, n, w in _CONFIGS])
def test_split_cell_inputs_meet_the_conditions(opt, batch, n, world):
    """Every tensor's max|g64| >= 1e-4 of the gradient's and Y <= 2e-6 at the three read-out
    steps of every (optimizer, batch, n, W) the cells use, from the references alone."""
    cell = sp.SplitCell(sp.REF, opt, batch, n=n, world=world)
    recs = []
    for t, p in _trajectory(opt, batch, n, world):
        r, _ = sp.evaluate(cell, sc.StepGradient(t, p, None, None, None))
        recs += r
    assert len(recs) == len(sp.readout_steps(cell)) == 3
    fails = sp.check_conditions(cell, recs)
    assert not fails, "\n".join(fails)


def test_every_split_instance_has_a_cell():
    """Each of the 31 (engine, body, shape id) a default build can run is run by a cell, and no
    cell names an instance that does not exist."""
    assert len(sp.INSTANCES) == len(set(sp.INSTANCES)) == 31
    have = {i for c in sp.ALL_CELLS for i in c.instances}
    missing = [i for i in sp.INSTANCES if i not in have]
    assert not missing, missing
    unknown = sorted(have - set(sp.INSTANCES))
    assert not unknown, unknown
    # Adam runs all of them; SGD every instance of the cached bodies and one uncached split
    adam = {i for c in sp.ALL_CELLS if c.opt == "adam" for i in c.instances}
    assert adam == set(sp.INSTANCES)
    sgd = {i for c in sp.ALL_CELLS if c.opt == "sgd" for i in c.instances}
    assert sgd >= set(sp.INSTANCES[:24]) | {("one", "v1", 2), ("one", "v1", 10)}


def test_split_shape_table_is_the_x_macro_list():
    """SHAPES against the one list in ``csrc/split_shapes.h``, which both engines' sources expand
    and neither redefines, and the partitions against the shapes."""
    import os
    import re

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed_training_pytorch_amd",
                        "csrc")
    src = open(os.path.join(root, "split_shapes.h")).read()
    assert src.count("#define DTP_SPLIT_SHAPES(X)") == 1
    body = src[src.index("#define DTP_SPLIT_SHAPES(X)"):]
    body = body[:body.index("\n\n")]
    rows = [(int(a), int(b), int(c), int(d), e == "true", int(f))
            for a, b, c, d, e, f in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (true|false), (\d)\)", body)]
    assert rows == sp.SHAPES
    for name in ("split_train.hip", "split_lanes.hip"):
        src = open(os.path.join(root, name)).read()
        assert not re.search(r"#\s*define\s+DTP_SPLIT\w*SHAPES", src), name  # no list of its own
        assert not re.search(r"X\(\d+, \d+, \d+, \d+, (true|false), \d\)", src), name
        assert '#include "split_shapes.h"' in src and re.search(r"^\s*DTP_SPLIT_SHAPES\(X\)$", src, re.M), name
    parts = sp.all_partitions()
    assert len(parts) == len(set(parts)) == 16
    for p in parts:
        assert p[0][0] == 0 and p[-1][1] == 4 and all(a[1] + 1 == b[0] for a, b in zip(p, p[1:]))
        assert all(sp.stage_shape(a, b) in sp.SHAPES for a, b in p)
    assert {i for p in sp.COVER for i in sp.SplitCell(p, "sgd", 256).shape_ids} == set(range(12))


def test_split_cells_cover_what_the_matrix_is_for():
    """All 16 partitions in both engines, both link kinds, M = 1..8, W in {2, 3, 4, 8}, and the
    cache edges exactly."""
    for eng in ("one", "lanes"):
        assert {c.part for c in sp.CELLS if c.engine == eng and c.links == "auto"} == set(sp.all_partitions())
        assert {c.links for c in sp.ALL_CELLS if c.engine == eng} == {"auto", "remote"}
        assert {c.opt for c in sp.CELLS if c.engine == eng and c.links == "remote"} == {"adam", "sgd"}
        assert any(c.launch == "per_stage" and c.links == "remote" and c.part == sp.REF
                   for c in sp.CELLS if c.engine == eng)
        assert {c.world for c in sp.WORLD_CELLS if c.engine == eng} == {2, 3, 4, 8}
    assert {c.members for c in sp.CELLS} == set(range(9))
    assert {c.members for c in sp.CELLS if c.opt == "sgd"} >= {0, 1, 3, 5, 8}
    assert any(c.links == "remote" and c.members for c in sp.WORLD_CELLS)
    assert all(1 < c.world <= 8 and c.world * max(c.members, 1) <= 8 for c in sp.WORLD_CELLS)
    assert {c.world * c.members for c in sp.WORLD_CELLS if c.members} >= {4, 6, 8}
    # a remote cell has a link; SGD runs every shape in both engines
    assert all(len(c.part) > 1 for c in sp.ALL_CELLS if c.links == "remote")
    for eng in ("one", "lanes"):
        assert {i for c in sp.CELLS if c.engine == eng and c.opt == "sgd" for i in c.shape_ids} == set(range(12))
    # the cache edges: n (XW + YW) at, just under and just over the two constants
    one = {(c.part, c.n) for c in sp.CELLS if c.engine == "one"}
    assert {(sp.REF, 4096), (sp.REF, 4097), (sp.part("04"), 2730), (sp.part("04"), 2731)} <= one
    assert 4096 * 2 == sp.K_SPLIT_CACHE and 2730 * 3 <= sp.K_SPLIT_CACHE < 2731 * 3
    lanes = {(c.part, c.n) for c in sp.CELLS if c.engine == "lanes"}
    assert {(sp.REF, 2048), (sp.part("04"), 1365)} <= lanes
    assert 2048 * 2 == sp.K_SL_DATA and 1365 * 3 <= sp.K_SL_DATA < 1366 * 3
    # every cell reads out the epoch's last batch (short unless the batch divides the rank's
    # share) and crosses into epoch 1
    for c in sp.ALL_CELLS:
        g = sp.cell_geom(c)
        steps = sp.readout_steps(c)
        assert len(steps) == 3 and steps[0] == 0 and steps[-1] == g.steps_per_epoch
        assert g.batch_size_at(steps[1]) == g.num_samples - (g.steps_per_epoch - 1) * c.batch
        assert g.batch_size_at(steps[1]) < c.batch or g.num_samples % c.batch == 0
    assert sp.cell_geom(sp.BY_ID["one-adam-b256-01_24-n4097"]).batch_size_at(16) == 1
    assert sp.cell_geom(sp.BY_ID["one-adam-b256-01_24-n8200"]).batch_size_at(32) == 8


def test_split_cells_claimed_bodies_follow_the_cache_rule():
    """A cell's instances follow from its partition, engine and n by ``n (XW + YW) <= 8192``; a
    members cell's dataset slices fit kSLData (its launch refuses them otherwise)."""
    for c in sp.ALL_CELLS:
        for (a, b), (eng, body, sid) in zip(c.part, c.instances):
            first, last = a == 0, b == 4
            floats = c.n * ((2 if first else 0) + (1 if last else 0))
            assert sid == sp.SHAPES.index(sp.stage_shape(a, b)) and eng == c.engine
            if c.members:
                assert body == "lanes" and floats <= sp.K_SL_DATA, c.id
                assert 1 <= c.members <= sp.K_SL_MAX_M and -(-c.batch // c.members) <= 64, c.id
            elif b == a:
                assert body == "v1"
            else:
                assert body == ("pipe" if floats <= sp.K_SPLIT_CACHE else "v1"), c.id
    # n = 4097: first stage uncached, last cached; n = 8200: both uncached; 4096: both cached
    assert [i[1] for i in sp.BY_ID["one-adam-b256-01_24-n4097"].instances] == ["v1", "pipe"]
    assert [i[1] for i in sp.BY_ID["one-adam-b256-01_24-n8200"].instances] == ["v1", "v1"]
    assert [i[1] for i in sp.BY_ID["one-adam-b256-01_24-n4096"].instances] == ["pipe", "pipe"]
    assert [i[1] for i in sp.BY_ID["one-adam-b256-04-n2730"].instances] == ["pipe"]
    assert [i[1] for i in sp.BY_ID["one-adam-b256-04-n2731"].instances] == ["v1"]


def test_split_sum_chain_is_the_one_the_evaluation_uses():
    for c in sp.ALL_CELLS:
        assert sp.split_sum_chain(c) == sc.sum_chain(c, c.batch), c.id


# ---- the evaluation against synthetic read-outs


def _apply(cell, t, p0, g):
    """The parameters after the step that took gradient ``g`` from zeroed moments."""
    if cell.opt == "sgd":
        return (p0.double() - sp.SGD.lr * g.double()).float()
    lr, b2, eps = sp.ADAM.lr, sp.ADAM.betas[1], sp.ADAM.eps
    m = g.double()
    bc2 = 1.0 - b2 ** (t + 1)
    return (p0.double() - lr * m / ((1.0 - b2) ** 0.5 * m.abs() / bc2 ** 0.5 + eps)).float()


def _synthetic(cell, wrong=None):
    """The read-outs an engine would leave if its step were fp32 autograd per rank, summed in
    rank order and scaled by 1 / W.  ``wrong(t, r, idx, g, lo) -> (g, lo)`` replaces one rank's
    gradient of one step; ``after(t, g) -> g`` (its attribute) the finished read-out."""
    X, Y = sp.cell_data(cell)
    out = []
    for t, p in _trajectory(cell.opt, cell.batch, cell.n, cell.world):
        g, lo = torch.zeros_like(p[0]), torch.zeros(())
        for r, idx in enumerate(sp.cell_indices(cell, t)):
            ix = torch.tensor(idx, dtype=torch.long)
            gr, lr = sp.autograd_gradient(cell.spec, p[0], X[ix], Y[ix], "mse", torch.float32)
            if wrong is not None:
                gr, lr = wrong(t, r, idx, p[0], gr, lr)
            g, lo = g + gr, lo + lr
        if cell.world > 1:
            inv = torch.tensor(1.0 / cell.world)
            g, lo = g * inv, lo * inv
        out.append(sc.StepGradient(t, p.clone(), g[None], lo.view(1), _apply(cell, t, p[0], g)[None]))
    return out


def _evaluate_all(cell, sgs):
    recs, fails = [], []
    for sg in sgs:
        r, f = sp.evaluate(cell, sg)
        recs += r
        fails += f
    return recs, fails


_SYN = ["one-adam-b200-01_24", "m3a-sgd-b130-00_12_34", "w3-one-sgd-b100-01_24", "w2-m4a-adam-b200-01_24"]


@pytest.mark.parametrize("cid", _SYN)
def test_split_evaluation_passes_fp32_autograd(cid):
    cell = sp.BY_ID[cid]
    recs, fails = _evaluate_all(cell, _synthetic(cell))
    assert not fails, "\n".join(fails)
    assert len(recs) == 3 and all(r["E"] == r["Y"] and r["E_loss"] == r["Y_loss"] for r in recs)


def _stage_slice(cell, s):
    a, b = cell.part[s]
    lo, hi = cell.spec.param_range(a, b)
    return slice(lo, hi)


def test_split_evaluation_catches_a_scaled_stage():
    """One stage's slice scaled by 1 + 1e-4 (the update made with it, so only the metric sees it)."""
    cell = sp.BY_ID["m3a-sgd-b130-00_12_34"]
    for s in range(3):
        def wrong(t, r, idx, p, g, lo, s=s):
            g = g.clone()
            g[_stage_slice(cell, s)] *= 1 + 1e-4
            return g, lo
        _, fails = _evaluate_all(cell, _synthetic(cell, wrong))
        assert fails and all(": E " in f for f in fails), fails
        assert len(fails) >= 3  # at every read-out


@pytest.mark.parametrize("cid", ["one-adam-b200-01_24", "m3a-sgd-b130-00_12_34"])
def test_split_evaluation_catches_a_short_batch_divided_by_the_batch(cid):
    """The epoch's short batch divided by ``batch`` instead of its own size -- which Adam's update
    hides (lr m / (sqrt(v) + eps) does not move) and the read-out does not."""
    cell = sp.BY_ID[cid]

    def wrong(t, r, idx, p, g, lo):
        f = torch.tensor(len(idx) / cell.batch)
        return g * f, lo

    sgs = _synthetic(cell, wrong)
    _, fails = _evaluate_all(cell, sgs)
    short = sp.readout_steps(cell)[1]
    assert fails and all(f" t={short} " in f and ": E " in f for f in fails), fails
    if cell.opt == "adam":  # the parameters alone would not have shown it
        good = _synthetic(cell)
        dp = (good[1].params_after - good[1].params_before).abs().max()
        assert (sgs[1].params_after - good[1].params_after).abs().max() <= 1e-2 * dp  # a gradient off by 44 %


def test_split_evaluation_catches_a_member_left_out():
    """The samples of one member (slices of ceil(batch / M)) missing from the sum."""
    cell = sp.BY_ID["m4a-adam-b200-01_24"]
    X, Y = sp.cell_data(cell)
    spm = -(-cell.batch // cell.members)
    for k in range(cell.members):
        def wrong(t, r, idx, p, g, lo, k=k):
            keep = [i for j, i in enumerate(idx) if j // spm != k]
            if len(keep) == len(idx):
                return g, lo
            ix = torch.tensor(keep, dtype=torch.long)
            gk, _ = sp.autograd_gradient(cell.spec, p, X[ix], Y[ix], "mse", torch.float32)
            return gk * torch.tensor(len(keep) / len(idx)), lo
        _, fails = _evaluate_all(cell, _synthetic(cell, wrong))
        # member 3 has no sample on the 112-sample batch: the other read-outs show it
        assert len({f.split(" model ")[0] for f in fails}) == (2 if k == 3 else 3), (k, fails)


def test_split_evaluation_catches_a_lost_rank_slot():
    cell = sp.BY_ID["w3-one-sgd-b100-01_24"]
    for drop in range(3):
        def wrong(t, r, idx, p, g, lo, drop=drop):
            return (torch.zeros_like(g), lo) if r == drop else (g, lo)
        _, fails = _evaluate_all(cell, _synthetic(cell, wrong))
        assert len([f for f in fails if ": E " in f]) >= 3, fails


def test_split_evaluation_catches_swapped_stages():
    """Two stages' slices in each other's place (equal sizes: the three middle one-layer stages)."""
    cell = sp.BY_ID["one-adam-b200-00_11_22_33_44"]
    s1, s2 = _stage_slice(cell, 1), _stage_slice(cell, 2)
    assert s1.stop - s1.start == s2.stop - s2.start

    def wrong(t, r, idx, p, g, lo):
        g = g.clone()
        g[s1], g[s2] = g[s2].clone(), g[s1].clone()
        return g, lo

    _, fails = _evaluate_all(cell, _synthetic(cell, wrong))
    assert any(" W1: E " in f for f in fails) and any(" W2: E " in f for f in fails), fails


def test_split_world_evaluation_catches_a_diverged_replica_and_a_short_run():
    cell = sp.BY_ID["w3-one-sgd-b100-01_24"]
    sgs = _synthetic(cell)
    last = sp.readout_steps(cell)[-1] + 1

    def result():
        one = {"fails": [], "readouts": [tuple(s) for s in sgs], "steps": [last] * 2, "t": last, "done": True}
        return {r: dict(one) for r in range(3)}

    recs, fails = sp.evaluate_world(cell, result())
    assert not fails and len(recs) == 3, fails
    res = result()
    t, p0, g, lo, p1 = res[1]["readouts"][1]
    g = g.clone()
    g[0, 7] = torch.nextafter(g[0, 7], torch.tensor(float("inf")))
    res[1]["readouts"] = [res[1]["readouts"][0], (t, p0, g, lo, p1), res[1]["readouts"][2]]
    _, fails = sp.evaluate_world(cell, res)
    assert fails == [f"{cell.id} t={t}: grad of rank 1 differs from rank 0's"], fails
    for key, val in (("steps", [last, last - 1]), ("done", False), ("fails", ["rank 2: link timed out"])):
        res = result()
        res[2][key] = val
        assert sp.evaluate_world(cell, res)[1], key
    res = result()
    del res[2]
    assert sp.evaluate_world(cell, res)[1]


def test_links_argument_is_validated():
    """``links`` is checked before anything touches a device."""
    from distributed_training_pytorch_amd.parallel.layer_split import FusedLayerSplit

    cell = sp.BY_ID["one-adam-b200-01_24"]
    X, Y = sp.cell_data(cell)
    with pytest.raises(ValueError, match="links"):
        FusedLayerSplit(cell.spec, [torch.device("cpu")] * 2, X, Y, sp.cell_geom(cell), sp.ADAM, sp.cell_init(cell)[0],
                        links="local")

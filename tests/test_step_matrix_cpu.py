"""The CPU side of the step matrix (``tests/step_cases.py``): the conditions every cell's inputs
must meet for its bound to mean something, the read-out helper on the CPU engine, and the cell
table against the list of kernel instances."""
import functools

import pytest
import torch

from . import step_cases as sc

CPU = torch.device("cpu")


@functools.lru_cache(maxsize=None)
def _trajectory(shape, opt, loss, batch, n):
    """The CPU engine's read-outs of a configuration (fp32 reference step; shared by the cells
    that differ only in instance, cache, groups, precision or forced environment)."""
    cell = sc.Cell(shape, opt, loss, batch, (0, 0, 0), "cpu", n=n)
    tr = sc.make_trainer(cell, CPU)
    out = []
    for t in sc.readout_steps(cell):
        if tr.t < t:
            tr.train(t - tr.t)
        out.append((sc.step_gradient(tr), tr.step_indices(t)))
    tr.close()
    return out


@pytest.mark.parametrize("cell", sc.ALL_CELLS, ids=[c.id for c in sc.ALL_CELLS])
def test_cell_inputs_meet_the_conditions(cell):
    """Every tensor's max|g64| >= 1e-4 of the gradient's, Y <= 2e-6, and for bf16 cells
    max D >= 100 Y -- at the three read-out steps, from the references alone."""
    X, Y = sc.cell_data(cell)
    recs = []
    for sg, idx in _trajectory(cell.shape, cell.opt, cell.loss, cell.batch, cell.n):
        r, _ = sc.evaluate_step(cell, sg._replace(grad=None), idx, X, Y)
        recs += r
    assert len(recs) == sc.N_MODELS * len(sc.readout_steps(cell))
    fails = sc.check_conditions(cell, recs)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", ["T-adam-mse-fp32-b200-gon", "T-sgd-mse-fp32-b100-goff", "C4-adam-ce-fp32-b130-gon",
                                 "C4-sgd-ce-fp32-b64-goff", "C4-adam-mse-fp32-b50-goff"])
def test_readout_on_cpu_engine_is_autograd_gradient(cid):
    """The read-out through the optimizer state is the gradient bit for bit: the CPU engine's
    step is fp32 autograd of the same expression, for Adam (beta1 = 0) and SGD (momentum),
    on the first and on later steps, short batches included."""
    cell = sc.BY_ID[cid]
    X, Y = sc.cell_data(cell)
    for sg, idx in _trajectory(cell.shape, cell.opt, cell.loss, cell.batch, cell.n):
        ix = torch.tensor(idx, dtype=torch.long)
        assert len(idx) == sc.cell_geom(cell).batch_size_at(sg.t)
        for i in range(sc.N_MODELS):
            g, lo = sc.autograd_gradient(cell.spec, sg.params_before[i], X[ix], Y[ix], cell.loss, torch.float32)
            assert torch.equal(sg.grad[i], g)
            assert sg.loss[i].item() == lo.item()
            assert not sc.applied_is_stored(cell, sg, i)
        # and the whole evaluation passes on it (E = 0 against its own yardstick)
        recs, fails = sc.evaluate_step(cell, sg, idx, X, Y)
        assert not fails, "\n".join(fails)
        assert all(r["E"] == r["Y"] for r in recs)


def test_applied_is_stored_catches_another_gradient():
    """The applied-vs-stored check fails when the update used another gradient than the one left
    in the moment: SGD sees one element scaled by 1 + 1e-3; Adam's first step from v = 0 is
    lr m / (c |m| + eps), which no scale of m moves, so there it is the sign."""
    for cid, f in (("T-sgd-mse-fp32-b100-goff", 1 + 1e-3), ("T-adam-mse-fp32-b200-gon", -1.0)):
        cell = sc.BY_ID[cid]
        sg, _ = _trajectory(cell.shape, cell.opt, cell.loss, cell.batch, cell.n)[1]
        g = sg.grad.clone()
        k = int(g[0].abs().argmax())
        g[0, k] *= f
        assert sc.applied_is_stored(cell, sg._replace(grad=g), 0)
        assert not sc.applied_is_stored(cell, sg, 0)


def test_metric_sees_one_element_off_by_1e4():
    """A bias-gradient row scaled by 1 + 1e-4 is far outside the fp32 bound."""
    cell = sc.BY_ID["T-adam-mse-fp32-b256-goff"]
    X, Y = sc.cell_data(cell)
    sg, idx = _trajectory(cell.shape, cell.opt, cell.loss, cell.batch, cell.n)[0]
    g = sg.grad.clone()
    lo, hi = cell.spec.param_range(2, 2)
    b2 = slice(hi - cell.spec.hidden, hi)  # b2
    g[0, b2] *= 1 + 1e-4
    _, fails = sc.evaluate_step(cell, sg._replace(grad=g, params_after=sg.params_before), idx, X, Y)
    assert any(" b2: E " in f and "model 0" in f for f in fails), fails


def test_bf16_rounding_model_keeps_parameter_gradients_in_fp32():
    """The kernels round what feeds a matmul (weights, activations, the gradients of matmul
    outputs and activations) and hand the optimizer the fp32 dW / db sums: so does the model."""
    from distributed_training_pytorch_amd.ops.mlp import bf16_round, mlp_forward_ref_bf16

    cell = sc.BY_ID["T-adam-mse-bf16-b100-goff"]
    X, Y = sc.cell_data(cell)
    p = sc.cell_init(cell)[0].double().requires_grad_(True)
    x = X[:100].double().requires_grad_(True)
    out = mlp_forward_ref_bf16(p, cell.spec, x)
    gp, gx = torch.autograd.grad(((out - Y[:100].double()) ** 2).mean(), [p, x])
    assert torch.equal(bf16_round(out.detach()), out.detach())
    assert torch.equal(bf16_round(gx), gx)
    off = (bf16_round(gp) - gp).abs() / gp.abs().clamp_min(1e-300)
    assert (off > 2.0 ** -12).sum() > 0.8 * gp.numel()  # not bf16 values: sums of products of bf16 values


def test_every_instance_has_a_cell():
    """Each (shape, lanes, waves, loss, optimizer, precision, kind) that the tables of
    csrc/mlp_train_one.hip and csrc/mlp_train_lanes.hip instantiate for the local optimizer
    modes is run by a cell;
    the split-batch families by a 4-member cell (the constant-count template) and another."""
    have = {c.instance for c in sc.ALL_CELLS}
    missing = [i for i in sc.INSTANCES if i not in have]
    assert not missing, missing
    unknown = sorted(have - set(sc.INSTANCES))
    assert not unknown, unknown
    for shape, loss, opt, prec in sc.GRP_CONST_FAMILIES:
        counts = {c.expect[2] for c in sc.CELLS
                  if c.kind == "grp" and (c.shape, c.loss, c.opt, c.prec) == (shape, loss, opt, prec)}
        assert 4 in counts and counts - {4}, (shape, loss, opt, prec, counts)


# ---- the cells of several ranks (the xGMI modes)


@functools.lru_cache(maxsize=None)
def _world_trajectory(shape, opt, loss, batch, n, world):
    """Parameters before each read-out step of a W-rank configuration along the fp32-model torch
    reference (``ref_train.torch_train``: autograd + torch.optim, one geometry per rank, the
    mean of the ranks' gradients), shared by the cells that differ only in instance or precision."""
    from distributed_training_pytorch_amd.data.sampler import EpochIndexStream

    from .ref_train import torch_train

    cell = sc.Cell(shape, opt, loss, batch, (0, 0, 0), "cpu", n=n, world=world)
    X, Y = sc.cell_data(cell)
    geoms = [EpochIndexStream(sc.cell_geom(cell, r)) for r in range(world)]
    out = []
    for t in sc.readout_steps(cell):
        p, _ = torch_train(cell.spec, sc.cell_init(cell), X, Y, geoms, t, sc.ADAM if opt == "adam" else sc.SGD, loss)
        out.append((t, p))
    return out


@pytest.mark.parametrize("cell", sc.ALL_XGMI, ids=[c.id for c in sc.ALL_XGMI])
def test_xgmi_cell_inputs_meet_the_conditions(cell):
    """The conditions of ``check_conditions`` for the cells of several ranks, from the references
    alone: the reference gradient is the mean over the ranks, Y the fp32 rank-order mean."""
    X, Y = sc.cell_data(cell)
    recs = []
    for t, p in _world_trajectory(cell.shape, cell.opt, cell.loss, cell.batch, cell.n, cell.world):
        sg = sc.StepGradient(t, p, None, None, None)
        r, _ = sc.evaluate_step(cell, sg, sc.cell_indices(cell, t), X, Y)
        recs += r
    assert len(recs) == sc.N_MODELS * len(sc.readout_steps(cell))
    fails = sc.check_conditions(cell, recs)
    assert not fails, "\n".join(fails)


def test_every_xgmi_instance_has_a_cell():
    """Each instance of the one-lane and the lanes table for DTP_MODE_XGMI_ADAM / _SGD is run by
    a cell of several ranks, and no cell names an instance that does not exist."""
    have = {c.instance for c in sc.ALL_XGMI}
    missing = [i for i in sc.XGMI_INSTANCES if i not in have]
    assert not missing, missing
    unknown = sorted(have - set(sc.XGMI_INSTANCES))
    assert not unknown, unknown
    assert all(1 < c.world <= 8 and c.world * c.expect[2] <= 8 for c in sc.ALL_XGMI)


def _pi(cell):
    """The poll body of xgmi_allreduce_g3 at 256 threads: ceil((V - 1) NG / 256)."""
    ng = (cell.spec.P + 1 + 2) // 3
    return -(-(cell.world * cell.expect[2] - 1) * ng // 256)


def test_xgmi_cells_reach_the_exchange_paths():
    """The paths the cells were chosen for, from the cells' own shapes: every poll body of g3
    (PI = 1, 2, 4 and MAXI = 8), a wave with two publish destinations, a padded sampler list
    whose last ranks wrap, the slots exchange at 8 ranks and at 512 threads."""
    g3 = [c for c in sc.XGMI_CELLS if c.kind in ("lanes", "grp") and c.expect[1] == 4]
    pis = {(c.shape, _pi(c)) for c in g3}
    assert {("T", 1), ("T", 2), ("T", 3), ("T", 4), ("H15", 3), ("H15", 5), ("H15", 8), ("C4", 2)} <= pis, sorted(pis)
    # publish: D = W - 1 destinations (W with members) over 4 waves
    assert any(c.world - 1 + (c.expect[2] > 1) > 4 for c in g3)
    for w, padded in ((3, 513), (5, 515)):
        cells = [c for c in sc.XGMI_CELLS if c.world == w]
        assert cells and all(sc.cell_geom(c).num_samples * w == padded for c in cells)
        # the last rank's share ends in the wrap: list position padded - 1 repeats the
        # permutation's element padded - 513, which is where rank padded - 513 starts
        c = cells[0]
        assert sc.EpochIndexStream(sc.cell_geom(c, w - 1)).epoch_list(0)[-1] == sc.EpochIndexStream(
            sc.cell_geom(c, padded - 513)).epoch_list(0)[0]
    slots8 = [c for c in sc.XGMI_CELLS if c.world == 8 and c.expect[0] == 1]
    assert {c.shape for c in slots8} >= {"T", "H15"} and all(c.n * 3 > 4096 for c in slots8)
    assert {c.expect[:2] for c in sc.XGMI_FORCED} == {(4, 8), (2, 8)}
    # every cell has a short last batch or a one-batch epoch, and crosses into epoch 1
    for c in sc.ALL_XGMI:
        g = sc.cell_geom(c)
        steps = sc.readout_steps(c)
        assert steps[0] == 0 and steps[-1] == g.steps_per_epoch
        assert g.batch_size_at(steps[-1] - 1) == g.num_samples - (g.steps_per_epoch - 1) * c.batch


def test_world_evaluation_of_one_rank_is_the_one_rank_evaluation():
    """evaluate_step on a cell of several ranks reduces to the one-rank evaluation when every
    rank holds the same batch: the mean of W equal gradients (W a power of two: exact)."""
    cell = sc.BY_ID["C4-adam-ce-fp32-b200-goff"]
    X, Y = sc.cell_data(cell)
    sg, idx = _trajectory(cell.shape, cell.opt, cell.loss, cell.batch, cell.n)[0]
    one, _ = sc.evaluate_step(cell, sg, idx, X, Y)
    two, _ = sc.evaluate_step(sc.replace(cell, world=2), sg, [idx, idx], X, Y)
    for a, b in zip(one, two):
        assert a["E"] == b["E"] and a["Y"] == b["Y"] and a["bound"] == b["bound"]
        assert a["bound_loss"] == b["bound_loss"] and a["E_loss"] == b["E_loss"]


def _synthetic_world_result(cell, drop_rank=None):
    """What run_cell_rank would return on every rank if the step were fp32 autograd per rank,
    summed in rank order and scaled by 1 / W (SGD: p1 = p0 - lr m) -- optionally with one
    rank's slot left out of the sum, as a wrong slot offset or mask bit would leave it."""
    X, Y = sc.cell_data(cell)
    W, inv = cell.world, torch.tensor(1.0 / cell.world)
    readouts = []
    for t, p in _world_trajectory(cell.shape, cell.opt, cell.loss, cell.batch, cell.n, W):
        g, lo = torch.zeros_like(p), torch.zeros(sc.N_MODELS)
        for r, ix in enumerate(sc.cell_indices(cell, t)):
            ix = torch.tensor(ix, dtype=torch.long)
            for i in range(sc.N_MODELS):
                gr, lr = sc.autograd_gradient(cell.spec, p[i], X[ix], Y[ix], cell.loss, torch.float32)
                if r != drop_rank:
                    g[i] += gr
                lo[i] += lr
        g, lo = g * inv, lo * inv
        readouts.append((t, p.clone(), g, lo, p - sc.SGD.lr * g))
    last = sc.readout_steps(cell)[-1] + 1
    one = {"fails": [], "comm": "xgmi", "fallback": None, "comm_after": "xgmi", "fallback_after": None,
           "pick": list(cell.expect), "readouts": readouts, "step_ctr": [last] * sc.N_MODELS, "t": last}
    return {r: dict(one) for r in range(W)}


def test_world_evaluation_catches_a_lost_slot_and_a_diverged_replica():
    cell = sc.BY_ID["w3-T-sgd-mse-fp32-b100-goff"]
    recs, fails = sc.evaluate_cell_world(cell, _synthetic_world_result(cell))
    assert not fails and len(recs) == 6 and all(r["E"] == r["Y"] for r in recs), fails
    # the last rank's slot missing from the sum: a third of the gradient
    _, fails = sc.evaluate_cell_world(cell, _synthetic_world_result(cell, drop_rank=2))
    assert any(": E " in f for f in fails), fails
    # one rank one ulp away in one element of one read-out
    res = _synthetic_world_result(cell)
    t, p0, g, lo, p1 = res[1]["readouts"][1]
    g = g.clone()
    g[1, 7] = torch.nextafter(g[1, 7], torch.tensor(float("inf")))
    res[1]["readouts"] = [res[1]["readouts"][0], (t, p0, g, lo, p1), res[1]["readouts"][2]]
    _, fails = sc.evaluate_cell_world(cell, res)
    assert fails == [f"{cell.id} t={t}: grad of rank 1 differs from rank 0's"], fails
    # a rank that fell back to RCCL, a rank with another pick, a rank that did not answer
    for key, val in (("fallback", "timeout at epoch 1"), ("pick", [1, 4, 1]), ("comm", "rccl")):
        res = _synthetic_world_result(cell)
        res[2][key] = val
        assert sc.evaluate_cell_world(cell, res)[1]
    res = _synthetic_world_result(cell)
    del res[2]
    assert sc.evaluate_cell_world(cell, res)[1]


def test_cells_follow_the_issue_geometry():
    """n = 512 (one cell: 1024), read-outs at step 0, the epoch's last step and the next epoch's first."""
    for c in sc.ALL_CELLS:
        g = sc.cell_geom(c)
        steps = sc.readout_steps(c)
        assert steps[0] == 0 and steps[-1] == g.steps_per_epoch
        assert g.batch_size_at(steps[-1] - 1) == c.n - (g.steps_per_epoch - 1) * c.batch

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
    """Each (shape, lanes, waves, loss, optimizer, precision, kind) that train_fn, lanes_inst and
    grp_inst of csrc/mlp_train.hip instantiate for the local optimizer modes is run by a cell;
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


def test_cells_follow_the_issue_geometry():
    """n = 512 (one cell: 1024), read-outs at step 0, the epoch's last step and the next epoch's first."""
    for c in sc.ALL_CELLS:
        g = sc.cell_geom(c)
        steps = sc.readout_steps(c)
        assert steps[0] == 0 and steps[-1] == g.steps_per_epoch
        assert g.batch_size_at(steps[-1] - 1) == c.n - (g.steps_per_epoch - 1) * c.batch

"""The CPU side of clipping inside the fused step (``tests/clip_step_cases.py``): the twin table
against the cells, the cells' bounds against their conditions, the protocol's evaluation against
wrong answers, the CPU engine's clipped read-out against clipped fp64 autograd, and the runner's
fallback on a CPU device."""
import sys
from dataclasses import replace

import pytest
import torch

from . import clip_step_cases as cc
from . import step_cases as sc

CPU = torch.device("cpu")
ALL = cc.CLIP_CELLS + [c for cs in cc.WORLD_CELLS.values() for c in cs]


def test_every_twin_has_a_cell_and_every_cell_names_a_twin():
    have = {cc.twin_of(c) for c in cc.CLIP_CELLS}
    missing = [t for t in cc.TWINS if t not in have]
    assert not missing, missing
    assert len(cc.CLIP_CELLS) == len(cc.TWINS) == len(set(cc.TWINS)) == 42
    assert not sorted(have - set(cc.TWINS))
    # a twin's cell is the FIRST cell of step_cases.CELLS that runs its plain instance
    for c in cc.CLIP_CELLS:
        first = next(x for x in sc.CELLS if cc.twin_of(x) == cc.twin_of(c))
        assert first is c
    # no twin of the 8-wave instances, and none is reached through a forced environment
    assert all(t[2] == 4 for t in cc.TWINS) and all(not c.env for c in cc.CLIP_CELLS)
    ids = {c.id for c in cc.CLIP_CELLS}
    assert set(cc.SUBSET_IDS) <= ids
    kinds = {cc.twin_of(sc.BY_ID[i])[6] if sc.BY_ID[i].prec == "fp32" else "bf16" for i in cc.SUBSET_IDS}
    assert kinds == {"generic", "lanes", "grp", "grp4", "bf16"}
    assert {sc.BY_ID[i].expect[0] for i in cc.SUBSET_IDS} == {1, 2, 4}
    # the cells' parameter counts, and parameters per thread that do not divide them
    assert {c.spec.P for c in cc.CLIP_CELLS} == {151, 371, 404, 781}
    assert {-(-c.spec.P // 256) for c in cc.CLIP_CELLS} == {1, 2, 4}
    assert min(c.batch for c in cc.CLIP_CELLS) == 50 and max(c.batch for c in cc.CLIP_CELLS) == 300
    # a split-batch member without a sample in the epoch's last batch
    assert any(c.kind == "grp" and sc.cell_geom(c).batch_size_at(sc.cell_geom(c).steps_per_epoch - 1) <= 64 * (c.expect[2] - 1)
               for c in cc.CLIP_CELLS)
    # the cells of several ranks: the four xGMI twin kinds
    assert {(w, cc.twin_of(c)[1], cc.twin_of(c)[6]) for w, cs in cc.WORLD_CELLS.items() for c in cs} == {
        (2, 4, "grp4"), (2, 2, "lanes"), (3, 4, "lanes"), (3, 1, "generic")}
    assert all(c.world * c.expect[2] <= 8 for c in ALL)


@pytest.mark.parametrize("cell", ALL, ids=[c.id for c in ALL])
def test_bounds_meet_their_conditions(cell):
    """From the reference alone: C_bind binds at every read-out step of both models with room
    for the kernels' fp32 gradient (coef <= 0.5), C_free cannot bind (coef would be >= 2), and
    c_val clamps between 10 % and 90 % of the elements at every read-out step."""
    b = cc.bounds(cell)
    assert len(b.norms) == len(sc.readout_steps(cell)) and all(len(r) == sc.N_MODELS for r in b.norms)
    flat = [x for r in b.norms for x in r]
    assert min(flat) > 1e-3, flat
    assert all(b.c_bind / (n + 1e-6) <= 0.5 for n in flat)
    assert all(b.c_free / (n + 1e-6) >= 2.0 - 1e-3 for n in flat)
    assert b.c_val > 0 and all(0.1 <= s <= 0.9 for s in b.clamped), b.clamped
    assert abs(b.clamped[0] - 0.5) < 0.01  # the median


@pytest.fixture(scope="module")
def cpu_readouts():
    """The protocol on the CPU engine (its step is fp32 autograd and flat_optimizer_step's CPU
    branch, whose clipping is the protocol's own expressions) for two cells, all three kinds."""
    out = {}
    for cid in ("T-sgd-mse-fp32-b128-goff", "C4-adam-ce-fp32-b50-goff"):
        cell = sc.BY_ID[cid]
        ros, fails = cc.run_clip_cell(cell, CPU, subset=True, expect_native=False)
        assert not fails, "\n".join(fails)
        assert len(ros) == len(sc.readout_steps(cell))
        out[cid] = ros
    return out


def test_protocol_passes_on_the_cpu_engine_and_sets_grad_norm(cpu_readouts):
    for cid, ros in cpu_readouts.items():
        b = cc.bounds(sc.BY_ID[cid])
        for r in ros:
            n = r["bind"].norm
            assert n is not None and n.dtype == torch.float32 and n.shape == (sc.N_MODELS,)
            assert (n >= 2 * b.c_bind * (1 - 1e-3)).all()
            assert r["value"].norm is None  # grad_norm: None without max_grad_norm
            assert r["free"].norm is not None and torch.equal(r["free"].norm, n)


def test_evaluation_fails_on_wrong_answers(cpu_readouts):
    cid = "T-sgd-mse-fp32-b128-goff"
    cell, b = sc.BY_ID[cid], cc.bounds(sc.BY_ID[cid])
    ro = cpu_readouts[cid][1]["bind"]
    assert not cc.evaluate_readout(cell, ro, "bind", b.c_bind)
    inf = torch.tensor(float("inf"))
    # the gradient scaled by the wrong coefficient: the other model's
    coef = (b.c_bind / (ro.norm + 1e-6)).clamp(max=1.0)
    assert coef[0] != coef[1]
    m = ro.m.clone()
    m[0] = ro.g_plain[0] * coef[1]
    fails = cc.evaluate_readout(cell, ro._replace(m=m), "bind", b.c_bind)
    assert any("model 0: m != gA * coef" in f for f in fails) and not any("model 1: m !=" in f for f in fails), fails
    # ... and by one float32 of the coefficient
    m[0] = ro.g_plain[0] * torch.nextafter(coef[0], inf)
    assert any("model 0: m != gA * coef" in f for f in cc.evaluate_readout(cell, ro._replace(m=m), "bind", b.c_bind))
    # a norm two floats off (one float off is a double-rounding tie: accepted), with the
    # gradient scaled to match it
    for k, bad in ((1, False), (2, True)):
        n = ro.norm.clone()
        for _ in range(k):
            n[1] = torch.nextafter(n[1], inf)
        c2 = (b.c_bind / (n + 1e-6)).clamp(max=1.0)
        fails = cc.evaluate_readout(cell, ro._replace(norm=n, m=ro.g_plain * c2.unsqueeze(1)), "bind", b.c_bind)
        assert any("model 1: grad_norm" in f for f in fails) == bad, (k, fails)
    # an engine that did not clip at all; a loss that differs
    assert cc.evaluate_readout(cell, ro._replace(m=ro.g_plain), "bind", b.c_bind)
    lo = ro.loss.clone()
    lo[0] = torch.nextafter(lo[0], inf)
    assert any("loss" in f for f in cc.evaluate_readout(cell, ro._replace(loss=lo), "bind", b.c_bind))
    # a bound that does not bind fails the protocol's coef < 1
    assert any("does not bind" in f for f in cc.evaluate_readout(cell, cpu_readouts[cid][1]["free"], "bind", b.c_free))
    # the parameters moved by another gradient than the one left in m
    p = ro.params.clone()
    p[1] = ro.params_plain[1]
    assert any("SGD" in f for f in cc.evaluate_readout(cell, ro._replace(params=p), "bind", b.c_bind))
    # by value: a clamp applied to only one model; a bound that clamps nothing
    rv = cpu_readouts[cid][1]["value"]
    assert not cc.evaluate_readout(cell, rv, "value", b.c_val)
    m = rv.m.clone()
    m[1] = rv.g_plain[1]
    fails = cc.evaluate_readout(cell, rv._replace(m=m), "value", b.c_val)
    assert any("model 1: m != gA.clamp" in f for f in fails) and not any("model 0: m !=" in f for f in fails), fails
    big = 2 * rv.g_plain.abs().max().item()
    assert any("are clamped" in f for f in cc.evaluate_readout(cell, rv._replace(m=rv.g_plain), "value", big))
    # free: any difference from the plain engine
    rf = cpu_readouts[cid][1]["free"]
    assert not cc.evaluate_readout(cell, rf, "free", b.c_free)
    assert cc.evaluate_readout(cell, rf._replace(m=ro.m), "free", b.c_free)


@pytest.mark.parametrize("cid", ["T-sgd-mse-fp32-b128-goff", "C4-adam-ce-fp32-b50-goff"])
def test_cpu_engine_clipped_readout_is_clipped_fp64_autograd(cid, cpu_readouts):
    """FusedTrainer on the CPU with max_grad_norm: the gradient its optimizer took is fp64
    autograd's scaled by torch's coefficient on the fp64 norm, at step_cases' fp32 bound
    (max(4 Y, 8 * 2^-24) per tensor, plus the CE margin), and tr.grad_norm is that norm."""
    cell, b = sc.BY_ID[cid], cc.bounds(sc.BY_ID[cid])
    X, Y = sc.cell_data(cell)
    stream = sc.EpochIndexStream(sc.cell_geom(cell))
    for r in cpu_readouts[cid]:
        ro = r["bind"]
        ix = torch.tensor(stream.indices(ro.t), dtype=torch.long)
        for i in range(sc.N_MODELS):
            p = ro.params_before[i]
            g64, _ = sc.autograd_gradient(cell.spec, p, X[ix], Y[ix], cell.loss, torch.float64)
            g32, _ = sc.autograd_gradient(cell.spec, p, X[ix], Y[ix], cell.loss, torch.float32)
            n64 = g64.norm()
            ref = g64 * (b.c_bind / (n64 + 1e-6)).clamp(max=1.0)
            assert abs(ro.norm[i].item() - n64.item()) <= 4 * max(sc.metric(cell.spec, g32, g64).values()) * n64.item() + 2e-7 * n64.item()
            Yt = sc.metric(cell.spec, g32, g64)
            bound = {n: max(4 * v, 8 * sc.U) for n, v in Yt.items()}
            if cell.loss == "ce":
                mt, _ = sc.ce_margin(cell.spec, p, X[ix], Y[ix], g64)
                bound = {n: bound[n] + mt[n] for n in bound}
            E = sc.metric(cell.spec, ro.m[i], ref)
            assert all(E[n] <= bound[n] for n in E), (ro.t, i, E, bound)
            # and it is not the unclipped gradient
            assert max(sc.metric(cell.spec, ro.m[i], g64).values()) > 0.4


def test_cpu_trainer_fields_and_checkpoint():
    cell = sc.BY_ID["T-sgd-mse-fp32-b128-goff"]
    b = cc.bounds(cell)
    tr = cc.make_clip_trainer(cell, CPU, replace(sc.SGD, max_grad_norm=b.c_bind))
    assert tr.clip_in_kernel is False and tr.grad_norm is not None and tr.grad_norm.device.type == "cpu"
    tr.train(2)
    assert (tr.grad_norm > b.c_bind).all()
    sd = tr.state_dict()
    assert "grad_norm" not in sd and set(sd) == {"params", "m", "v", "step", "t", "spec", "optim"}
    plain = sc.make_trainer(cell, CPU)
    assert plain.grad_norm is None and plain.clip_in_kernel is False
    assert cc.make_clip_trainer(cell, CPU, replace(sc.SGD, clip_grad_value=b.c_val)).grad_norm is None
    with pytest.raises(RuntimeError, match="native"):
        tr.local_gradients()


def test_runner_keeps_the_cpu_fallback(capsys):
    """--engine fused with a clipping flag on a CPU device: the module engine and its note,
    word for word (tests/test_clip_cpu.py runs the demo itself on two gloo ranks)."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import argument_parser
    from distributed_training_pytorch_amd.engine import runner

    cfg = argument_parser.get_args(["--engine", "fused", "--device", "cpu", "--iters", "2", "--no_progress", "--dry_run",
                                    "--clip_grad_norm", "0.5"])
    s = runner.train(cfg, None, CPU, 0, 1)
    out = capsys.readouterr().out
    assert s["engine"] == "module" and len(s["grad_norm"]) == 2
    assert ("gradient clipping (--clip_grad_norm / --clip_grad_value) is not in the fused step kernel: "
            "using the module engine") in out
    # without a flag the fused engine's CPU reference path runs, and reports no norm
    cfg = argument_parser.get_args(["--engine", "fused", "--device", "cpu", "--iters", "2", "--no_progress", "--dry_run"])
    s = runner.train(cfg, None, CPU, 0, 1)
    assert s["engine"] == "fused" and "grad_norm" not in s

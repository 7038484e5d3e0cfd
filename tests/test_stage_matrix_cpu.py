"""The CPU side of the stage matrix (``tests/stage_cases.py``): the conditions every cell's
inputs must meet for its bound to mean something, the metric's own sensitivity, the rounding
model, and the cell table against the shape lists of ``csrc/mlp_shapes.h``."""
import os
import re

import pytest
import torch

from distributed_training_pytorch_amd.ops.mlp import mlp_forward_ref, mlp_forward_ref_bf16

from . import stage_cases as st

_CASES = sorted({(c.key, b, c.slope, i, c.prec == "bf16") for c in st.CELLS for i, b in st.models_of(c)})


def _case_id(k):
    return f"{'x'.join(map(str, k[0]))}-b{k[1]}-s{k[2]}-m{k[3]}{'-bf16' if k[4] else ''}"


@pytest.mark.parametrize("ck", _CASES, ids=[_case_id(k) for k in _CASES])
def test_cell_inputs_meet_the_conditions(ck):
    """Y <= 2e-6 for the parameter tensors and ``out``, <= 4e-6 for ``grad_in``, every tensor's
    max|g64| >= 1e-2 of the gradient's, and for bf16 D >= 100 Y -- from the references alone."""
    fails = st.check_conditions(st.get_case(*ck))
    assert not fails, "\n".join(fails)


def _cpu_result(case):
    r = st.reference(case.spec, case.p, case.x, case.go, torch.float32)
    return {k: r[k] for k in ("out", "saved", "grad_params", "grad_in")}


@pytest.mark.parametrize("cid", ["bwd_dx-2x10x5x1x0-b257-fp32", "bwd_dx-10x10x3x10x1-b3000-fp32",
                                 "bwd_nodx-4x15x5x4x0-b1025-fp32", "fwd-2x15x5x4x0-b63-fp32"])
def test_fp32_autograd_passes_its_own_evaluation(cid):
    """fp32 CPU autograd is the yardstick: evaluated as a result it has E = Y and passes."""
    cell = st.BY_ID[cid]
    (case,) = st.cases_of(cell)
    got = _cpu_result(case)
    if cell.family == "fwd":
        got = {k: got[k] for k in ("out", "saved")}
    rec, fails = st.evaluate(cell, case, got)
    assert not fails, "\n".join(fails)
    assert all(rec["E"][n] == case.Y[n] for n in rec["E"])
    assert ("margin" in rec) == cell.multi_block


def test_metric_sees_the_mistakes_a_kernel_can_make():
    """One bias-gradient row scaled by 1 + 1e-4, one ``grad_in`` row dropped, one ``saved``
    column shifted by one: each fails its quantity and nothing else."""
    cell = st.BY_ID["bwd_dx-2x15x5x4x0-b257-fp32"]
    (case,) = st.cases_of(cell)
    spec, good = case.spec, _cpu_result(case)
    assert not st.evaluate(cell, case, good)[1]
    g = good["grad_params"].clone()
    lo, hi = spec.param_range(2, 2)
    g[hi - spec.hidden + 3] *= 1 + 1e-4  # one element of b2
    fails = st.evaluate(cell, case, {**good, "grad_params": g})[1]
    assert len(fails) == 1 and " b2: E " in fails[0], fails
    gi = good["grad_in"].clone()
    gi[200] = 0.0
    fails = st.evaluate(cell, case, {**good, "grad_in": gi})[1]
    assert len(fails) == 1 and " grad_in: E " in fails[0], fails
    sv = good["saved"].clone()
    H = spec.hidden
    sv[:, H:2 * H] = torch.roll(sv[:, H:2 * H], 1, dims=1)  # layer 2's columns shifted by one
    fails = st.evaluate(cell, case, {**good, "saved": sv})[1]
    assert len(fails) == 1 and " saved2: E " in fails[0], fails
    # the multi-block margin does not hide the scaled element either
    cell = st.BY_ID["bwd_dx-4x15x5x4x0-b3000-fp32"]
    (case,) = st.cases_of(cell)
    good = _cpu_result(case)
    g = good["grad_params"].clone()
    lo, hi = case.spec.param_range(2, 2)
    g[hi - case.spec.hidden + 3] *= 1 + 1e-4
    assert st.evaluate(cell, case, {**good, "grad_params": g})[1]


def test_bf16_metric_sees_fp32_compute():
    """The fp32 model's own results are D from the rounding model: they miss E <= D / 2."""
    cell = st.BY_ID["bwd_dx-2x10x5x4x0-b257-bf16"]
    (case,) = st.cases_of(cell)
    got = {k: case.r64[k].float() for k in ("grad_params", "grad_in")}
    fails = st.evaluate(cell, case, got)[1]
    assert any("grad_params" in f for f in fails) and any("grad_in" in f for f in fails), fails
    ok = {k: case.rb[k].float() for k in ("grad_params", "grad_in")}
    assert not st.evaluate(cell, case, ok)[1]


@pytest.mark.parametrize("key", st.BF16_SHAPES + [(10, 10, 2, 10, 1)])
def test_forward_parts_is_the_reference_model(key):
    """``forward_parts`` is ``mlp_forward_ref`` / ``mlp_forward_ref_bf16`` bit for bit, outputs
    and gradients: the hidden activations it also returns are those models'."""
    spec, p, x, go = st.stage_inputs(key, 65)
    for bf, ref in ((False, mlp_forward_ref), (True, mlp_forward_ref_bf16)):
        q = p.double().requires_grad_(True)
        xx = x.double().requires_grad_(True)
        want = ref(q, spec, xx)
        gq, gx = torch.autograd.grad(want, [q, xx], grad_outputs=go.double())
        r = st.reference(spec, p, x, go, torch.float64, bf16=bf)
        assert torch.equal(r["out"], want.detach()) and torch.equal(r["grad_params"], gq)
        assert torch.equal(r["grad_in"], gx)


def test_slope_cells_cross_the_kink_in_every_output_column():
    """``leaky_grad_from_out(out)`` decides from the stage's own output: the FINAL_ACT slope
    cells have samples with a negative and with a positive output in every column, and the
    run-time slope changes the reference."""
    cells = [c for c in st.CELLS if c.slope != 0.01 and c.key[4]]
    assert {c.family for c in cells} == {"fwd", "bwd_dx", "bwd_nodx"} and {c.key for c in cells} == {(10, 10, 2, 10, 1)}
    assert {c.key for c in st.CELLS if c.slope != 0.01} == {st.TOY, (10, 10, 2, 10, 1)}
    for c in cells:
        (case,) = st.cases_of(c)
        out = case.r64["out"]
        assert (out > 0).any(0).all() and (out < 0).any(0).all(), c.id
    for key in (st.TOY, (10, 10, 2, 10, 1)):
        a, b = st.get_case(key, 257, 0.2).r64, st.get_case(key, 257, 0.01).r64
        assert (a["grad_params"] - b["grad_params"]).abs().max() > 1e-2 * b["grad_params"].abs().max()


def test_every_shape_has_its_cells():
    """Every DTP_STAGE_SHAPES row has fwd, bwd<true> and bwd<false> cells, every
    DTP_STAGE_BF16_SHAPES row all three in bf16, and no cell names a shape outside the lists."""
    fp32 = st.header_shapes("DTP_STAGE_SHAPES")
    bf16 = st.header_shapes("DTP_STAGE_BF16_SHAPES")
    assert len(fp32) == 18 == len(set(fp32)) and len(bf16) == 2
    assert sorted(fp32) == sorted(st.FP32_SHAPES) and sorted(bf16) == sorted(st.BF16_SHAPES)
    for prec, shapes in (("fp32", fp32), ("bf16", bf16)):
        for fam in ("fwd", "bwd_dx", "bwd_nodx"):
            have = {c.key for c in st.CELLS if c.family == fam and c.prec == prec}
            assert not [k for k in shapes if k not in have], (prec, fam)
    for c in st.CELLS:
        assert c.key in (bf16 if c.prec == "bf16" else fp32), c.id
    # the multi-model families are instantiated for every fp32 shape: each has a cell, the
    # issue's three shapes every model count
    for fam, counts, full in (("fwd_multi", {1, 2, 3, 4}, (st.TOY, st.H15, (10, 10, 2, 1, 0))),
                              ("bwd_opt", {1, 2, 4}, (st.TOY, st.H15, st.IN4))):
        assert {c.key for c in st.CELLS if c.family == fam} == set(fp32), fam
        for k in full:
            assert {c.n for c in st.CELLS if c.family == fam and c.key == k} == counts
    assert {c.opt for c in st.CELLS if c.family == "bwd_opt" and c.key not in (st.TOY, st.H15, st.IN4)} == {"adam", "sgd"}


def _read(*parts):
    with open(os.path.join(st.ROOT, "distributed_training_pytorch_amd", *parts)) as fh:
        return fh.read()


def test_block_count_of_the_wrapper_is_the_launcher_s():
    """``ops.mlp.stage_backward`` zeroes the gradient buffer when its block count
    ``(B + 1023) // 1024`` exceeds one; ``launch_stage_bwd`` takes atomics when its own does."""
    kblock = int(re.search(r"constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;", _read("csrc", "dtp_common.h")).group(1))
    assert kblock == st.K_BLOCK
    m = re.search(r"int nblk = \(a->batch \+ (\d+) \* dtp::kBlock - 1\) / \((\d+) \* dtp::kBlock\);\s*"
                  r"if \(nblk > (\d+)\) nblk = (\d+);", _read("csrc", "mlp_stage.hip"))
    assert m, "launch_stage_bwd's block count has changed its form"
    per, per2, cap, cap2 = map(int, m.groups())
    assert per == per2 and cap == cap2 == st.BLOCK_CAP
    w = re.search(r"nblk = \(B \+ (\d+)\) // (\d+)\n", _read("ops", "mlp.py"))
    assert w, "stage_backward's block count has changed its form"
    add, div = map(int, w.groups())
    for B in list(range(1, 4200)) + [st.LARGE - 1, st.LARGE, 10 ** 7]:
        native = min((B + per * kblock - 1) // (per * kblock), cap)
        assert ((B + add) // div > 1) == (native > 1), B
        assert st.n_blocks(B) == native
        if native < cap:
            assert (B + add) // div == native, B
    assert st.n_blocks(st.LARGE) == 256 and -(-st.LARGE // 1024) == 258
    assert st.chain_length(1024) == 64 * 4 + 4 + 1 + 2 and st.chain_length(st.LARGE) == 64 * 5 + 4 + 256 + 2


def test_cells_follow_the_issue():
    ids = set(st.BY_ID)
    for k in st.EDGE_SHAPES:
        s = "x".join(map(str, k))
        for b in st.EDGE_BATCHES:
            assert f"fwd-{s}-b{b}-fp32" in ids and f"bwd_dx-{s}-b{b}-fp32" in ids
        for b in (1, 257, 1024, 1025):
            assert f"bwd_nodx-{s}-b{b}-fp32" in ids
    assert f"bwd_dx-10x10x3x10x1-b{st.LARGE}-fp32" in ids and f"bwd_nodx-4x15x5x4x0-b{st.LARGE}-fp32" in ids
    assert st.LARGE == 263169 and not any(c.key == st.TOY and c.batch == st.LARGE for c in st.CELLS)
    assert st.spec_of(st.IN4).P == 859
    assert len({b for b in st.MULTI_BATCHES}) == 4 and max(st.MULTI_BATCHES) == st.MULTI_BATCHES[0]

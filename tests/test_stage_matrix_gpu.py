"""Every stage kernel instance of ``csrc/mlp_stage.hip`` against fp64 (GPU only).

One test per cell of ``tests/stage_cases.py``: forward, backward with and without the input
gradient, accumulation into a pre-filled gradient, several models in one launch, the fused
backward + optimizer -- each held to the bounds of ``tests/stage_cases.py`` (fp32: 4 x the error
of fp32 torch autograd, plus the reduction margin above 1024 samples; bf16: half the distance
between the rounding model and fp32 compute).  Then the bounds of the kernels' reads and writes
(canaries around every output, NaN around every input), run-to-run determinism of the
single-block backward, and what the entry points must refuse.  Every cell prints one
``STAGE_MATRIX`` JSON line with E, Y (or D), the bound and E / Y; ``profiles/stage_matrix/``
keeps the table of one run."""
import json

import pytest
import torch

from distributed_training_pytorch_amd.ops.mlp import stage_backward, stage_forward

from . import stage_cases as st
from .step_cases import U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CANARY = -7777.25
DTP_OPT_ZERO_GRAD = 1


def _cells(*families):
    cs = [c for c in st.CELLS if c.family in families]
    return pytest.mark.parametrize("cell", cs, ids=[c.id for c in cs])


def _report(recs, fails):
    for r in recs:
        print("STAGE_MATRIX " + json.dumps(r))
    assert not fails, "\n".join(fails)
    assert recs


def _dev(case):
    return case.x.to(DEV), case.p.to(DEV), case.go.to(DEV)


@_cells("fwd", "bwd_dx", "bwd_nodx")
def test_stage_matches_fp64(cell):
    _report(*st.run_cell(cell, DEV))


@_cells("acc")
def test_accumulate_into_prefilled_gradient(cell):
    """One block: bitwise ``prefill + g`` with g the same call's result without accumulate, and
    again on a second call.  More blocks: the atomics add into the pre-fill, within the bound
    of ``prefill + g64`` (then ``prefill + 2 g64``)."""
    (case,) = st.cases_of(cell)
    spec = case.spec
    x, p, go = _dev(case)
    out, saved = stage_forward(x, p, spec)
    _, g = stage_backward(x, p, spec, out, saved, go)
    pre = st.prefill_vector(spec.P).to(DEV)
    buf = pre.clone()
    _, gp = stage_backward(x, p, spec, out, saved, go, grad_params=buf)
    assert gp.data_ptr() == buf.data_ptr()
    v1 = buf.clone()
    stage_backward(x, p, spec, out, saved, go, need_grad_in=False, grad_params=buf)
    torch.cuda.synchronize()
    recs, fails = [], []
    r, f = st.evaluate(cell, case, {"grad_params": g.cpu()}, what="plain")
    recs.append(r)
    fails += f
    if not cell.multi_block:
        assert torch.equal(v1, pre + g)
        assert torch.equal(buf, v1 + g)
    else:
        for calls, v in ((1, v1), (2, buf)):
            r, f = st.evaluate(cell, case, {"grad_params": v.cpu()}, prefill=pre.cpu(), calls=calls, what=f"call {calls}")
            recs.append(r)
            fails += f
    _report(recs, fails)


@_cells("fwd_multi")
def test_forward_of_several_models_in_one_launch(cell):
    """Models of different batches in one launch (the grid sized by the largest): each model's
    ``out`` and ``saved`` bitwise those of its own ``dtp_mlp_stage_fwd``, rows past its batch
    untouched, and within the fp64 bound."""
    cases = st.cases_of(cell)
    spec = cell.spec
    bmax = max(c.batch for c in cases)
    ins, outs, saveds, stages = [], [], [], []
    for c in cases:
        x, p, _ = _dev(c)
        o = torch.full((bmax, spec.out_features), CANARY, device=DEV)
        s = torch.full((bmax, (spec.n_layers - 1) * spec.hidden), CANARY, device=DEV) if spec.n_layers > 1 else None
        ins.append((x, p))
        outs.append(o)
        saveds.append(s)
        stages.append(st.stage_args(spec, x, p, o, s))
    assert st.launch_fwd_multi(spec.key, stages) == 0
    torch.cuda.synchronize()
    recs, fails = [], []
    for i, c in enumerate(cases):
        o1, s1 = stage_forward(*ins[i], spec)
        B = c.batch
        assert torch.equal(outs[i][:B], o1) and (outs[i][B:] == CANARY).all()
        if s1 is not None:
            assert torch.equal(saveds[i][:B], s1) and (saveds[i][B:] == CANARY).all()
        r, f = st.evaluate(cell, c, {"out": outs[i][:B].cpu(), "saved": None if s1 is None else saveds[i][:B].cpu()},
                           model=i)
        recs.append(r)
        fails += f
    _report(recs, fails)


class _OptSetup:
    """n models of one shape ready for ``dtp_mlp_stage_bwd_opt``: their forwards done, the
    optimizer's rows exactly their parameters and gradients."""

    def __init__(self, key, n, B, buffers_for=None):
        self.cases = [st.get_case(key, buffers_for or B, 0.01, i) for i in range(n)]
        self.spec, self.n, self.B = self.cases[0].spec, n, B
        self.P = self.spec.P
        self.params0 = torch.stack([c.p for c in self.cases]).to(DEV)
        self.x = [c.x.to(DEV) for c in self.cases]
        self.go = [c.go.to(DEV) for c in self.cases]
        fw = [stage_forward(self.x[i], self.params0[i].contiguous(), self.spec) for i in range(n)]
        self.out, self.saved = [f[0] for f in fw], [f[1] for f in fw]
        self.steps0 = torch.tensor(st.OPT_STEPS[:n], dtype=torch.int32, device=DEV)

    def state(self, grad, m=None):
        """Fresh (params, m, v, step, grad) rows."""
        z = torch.zeros(self.n, self.P, device=DEV)
        return [self.params0.clone(), z.clone() if m is None else m.clone(), z.clone(), self.steps0.clone(), grad.clone()]

    def stages(self, params, grad, accumulate=False, batch=None, grad_in=None, bf16=False):
        return [st.stage_args(self.spec, self.x[i], params[i], self.out[i], self.saved[i], self.go[i], grad_in,
                              grad[i], accumulate, bf16, batch=self.B if batch is None else batch)
                for i in range(self.n)]


@_cells("bwd_opt")
def test_backward_fused_with_optimizer(cell):
    """The gradient read out of ``opt_m`` (zero moment, beta1 = 0) and of ``grad_params`` agree
    bit for bit and hold the fp64 bound; the parameter change is the step of that gradient with
    row y's own counter (the rows start at 0, 5, 2, 7: SGD's first-step branch on one row only);
    every counter advances by one.  Then with ``accumulate`` on a pre-filled gradient and
    ``DTP_OPT_ZERO_GRAD``: the read-out is bitwise ``prefill + g``, the gradient ends all zero.
    SGD also from a non-zero momentum buffer: ``buf = g`` on the row at step 0,
    ``fmaf(buf, mom, g)`` on the others."""
    su = _OptSetup(cell.key, cell.n, cell.batch)
    n, P, opt = su.n, su.P, cell.opt
    recs, fails = [], []
    # ---- plain: grad_params overwritten (it starts as canary), not zeroed
    pa, m, v, step, grad = su.state(torch.full((n, P), CANARY, device=DEV))
    assert st.launch_bwd_opt(cell.key, su.stages(pa, grad), pa, m, v, step, grad, opt) == 0
    torch.cuda.synchronize()
    assert torch.equal(m, grad)
    assert step.tolist() == [t + 1 for t in st.OPT_STEPS[:n]]
    g_plain = m.clone()
    for i, c in enumerate(su.cases):
        r, f = st.evaluate(cell, c, {"grad_params": m[i].cpu()}, model=i)
        recs.append(r)
        fails += f
        fails += [f"{cell.id} model {i}: {x}" for x in
                  st.applied_is_stored(opt, st.OPT_STEPS[i], su.params0[i].cpu(), m[i].cpu(), pa[i].cpu())]
    if opt == "sgd":
        assert not v.any()
    # ---- accumulate into a pre-filled gradient, zeroed once read
    pre = torch.stack([st.prefill_vector(P, i) for i in range(n)]).to(DEV)
    pb, m, v, step, grad = su.state(pre)
    assert st.launch_bwd_opt(cell.key, su.stages(pb, grad, accumulate=True), pb, m, v, step, grad, opt,
                             flags=DTP_OPT_ZERO_GRAD) == 0
    torch.cuda.synchronize()
    assert not grad.any()
    assert torch.equal(m, pre + g_plain)
    assert step.tolist() == [t + 1 for t in st.OPT_STEPS[:n]]
    for i, c in enumerate(su.cases):
        r, f = st.evaluate(cell, c, {"grad_params": m[i].cpu()}, model=i, prefill=pre[i].cpu(), what="accumulate")
        recs.append(r)
        fails += f
        fails += [f"{cell.id} accumulate model {i}: {x}" for x in
                  st.applied_is_stored(opt, st.OPT_STEPS[i], su.params0[i].cpu(), m[i].cpu(), pb[i].cpu())]
    # ---- SGD from a non-zero momentum buffer: row y takes step[y]'s branch
    if opt == "sgd":
        m0 = (0.05 * torch.sin(torch.arange(n * P, dtype=torch.float64))).float().view(n, P).to(DEV)
        pc, m, v, step, grad = su.state(torch.zeros(n, P, device=DEV), m=m0)
        assert st.launch_bwd_opt(cell.key, su.stages(pc, grad), pc, m, v, step, grad, opt) == 0
        torch.cuda.synchronize()
        assert torch.equal(grad, g_plain)
        cfg = st.opt_config("sgd")
        mom, lr = float(torch.tensor(cfg.momentum).float()), float(torch.tensor(cfg.lr).float())
        for i in range(n):
            g64, b64 = grad[i].double(), m0[i].double()
            want = g64 if st.OPT_STEPS[i] == 0 else b64 * mom + g64  # exact in fp64 but for its last bit
            slack = 4e-16 * ((b64 * mom).abs() + g64.abs())  # the fp64 evaluation's own rounding
            assert ((m[i].double() - want).abs() <= U * want.abs() + slack).all(), (i, "momentum buffer")
            if st.OPT_STEPS[i] == 0:
                assert torch.equal(m[i], grad[i])
            p1 = su.params0[i].double() - lr * m[i].double()
            slack = 4e-16 * (su.params0[i].double().abs() + (lr * m[i].double()).abs())
            assert ((pc[i].double() - p1).abs() <= U * p1.abs() + slack).all(), (i, "parameters")
    _report(recs, fails)


def test_backward_fused_with_optimizer_refuses_what_it_cannot_run():
    """batch 1025, ``grad_in`` set, ``bf16`` set, a row whose ``params`` / ``grad`` pointer is
    not row i, n = 5 and ``o.P != S::P``: a non-zero return and nothing written."""
    su = _OptSetup(st.TOY, 2, 256, buffers_for=1025)
    n, P = su.n, su.P
    gin = torch.full((1025, su.spec.in_features), CANARY, device=DEV)

    def attempt(mutate, **kw):
        bufs = su.state(torch.full((n, P), CANARY, device=DEV))
        keep = [b.clone() for b in bufs]
        pa, m, v, step, grad = bufs
        stages = su.stages(pa, grad, **{k: kw[k] for k in ("batch", "grad_in", "bf16") if k in kw})
        if mutate:
            mutate(stages)
        rc = st.launch_bwd_opt(st.TOY, stages, pa, m, v, step, grad, "adam", n=kw.get("n"), P=kw.get("P"))
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(bufs, keep)) and bool((gin == CANARY).all())
        return rc, same

    def swap(field):
        def f(stages):
            a, b = getattr(stages[0], field), getattr(stages[1], field)
            setattr(stages[0], field, b)
            setattr(stages[1], field, a)
        return f

    for name, mutate, kw in (("batch 1025", None, {"batch": 1025}), ("grad_in", None, {"grad_in": gin}),
                             ("bf16", None, {"bf16": True}), ("params rows swapped", swap("params"), {}),
                             ("grad rows swapped", swap("grad_params"), {}), ("n = 5", None, {"n": 5}),
                             ("P", None, {"P": P - 1})):
        rc, same = attempt(mutate, **kw)
        assert rc != 0, name
        assert same, name
    rc, same = attempt(None)  # the unmodified launch is accepted and writes
    assert rc == 0 and not same


def test_rejected_shapes_and_sizes():
    """A shape outside the list: -2, in fp32 and (outside the bf16 list) in bf16; batch 0:
    0 and nothing written."""
    case = st.get_case(st.TOY, 65)
    spec = case.spec
    x, p, go = _dev(case)
    out, saved = stage_forward(x, p, spec)
    bufs = [torch.full_like(out, CANARY), torch.full_like(saved, CANARY), torch.full_like(x, CANARY),
            torch.full((spec.P,), CANARY, device=DEV)]
    o, s, gi, gp = bufs
    for key, bf in (((3, 10, 5, 1, 0), False), ((2, 10, 5, 1, 1), False), ((2, 10, 3, 1, 0), True), ((2, 15, 5, 1, 0), True)):
        assert st.launch_fwd(spec, x, p, o, s, bf16=bf, key=key) == -2, (key, bf)
        assert st.launch_bwd(spec, x, p, out, saved, go, gi, gp, bf16=bf, key=key) == -2, (key, bf)
    for bf in (False, True):
        assert st.launch_fwd(spec, x, p, o, s, bf16=bf, batch=0) == 0
        assert st.launch_bwd(spec, x, p, out, saved, go, gi, gp, bf16=bf, batch=0) == 0
    torch.cuda.synchronize()
    assert all(bool((b == CANARY).all()) for b in bufs)


# ------------------------------------------------------------------------------ bounds
_EDGE = [(k, b) for k in st.EDGE_SHAPES for b in (1, 255, 257, 1025)]
_edge = pytest.mark.parametrize("key,B", _EDGE, ids=[f"{'x'.join(map(str, k))}-b{b}" for k, b in _EDGE])


def _direct(case, wrap_in, wrap_out, want_dx=True):
    """Forward (with a peer output) and backward on the caller's kind of buffers:
    ({name: view}, [(buffer, view)] of the outputs)."""
    spec, B = case.spec, case.batch
    x, p, go = _dev(case)
    hid = (spec.n_layers - 1) * spec.hidden
    _, xv = wrap_in(x)
    ob, ov = wrap_out((B, spec.out_features))
    pb, pv = wrap_out((B, spec.out_features))
    sb, sv = wrap_out((B, hid)) if hid else (None, None)
    assert st.launch_fwd(spec, xv, p, ov, sv, out_peer=pv) == 0
    _, oin = wrap_in(ov.clone())
    _, sin = wrap_in(sv.clone()) if hid else (None, None)
    _, gov = wrap_in(go)
    gib, giv = wrap_out((B, spec.in_features)) if want_dx else (None, None)
    gb, gv = wrap_out((spec.P,))
    if st.n_blocks(B) > 1:
        gv.zero_()
    assert st.launch_bwd(spec, xv, p, oin, sin, gov, giv, gv) == 0
    torch.cuda.synchronize()
    views = {"out": ov, "out_peer": pv, "saved": sv, "grad_in": giv, "grad_params": gv}
    return views, [(b, v) for b, v in ((ob, ov), (pb, pv), (sb, sv), (gib, giv), (gb, gv)) if b is not None]


def _plain_in(t):
    return None, t


def _plain_out(shape):
    return None, torch.full(shape, CANARY, device=DEV)


@_edge
def test_writes_stay_inside_their_buffers(key, B):
    """``out``, ``out_peer``, ``saved``, ``grad_in`` and ``grad_params`` as views into canary-filled
    buffers: every canary intact, the results those of plain buffers."""
    case = st.get_case(key, B)

    def wrap_out(shape):
        return st.guarded(torch.full(shape, CANARY, device=DEV), CANARY)

    for want_dx in (True, False):
        views, outs = _direct(case, _plain_in, wrap_out, want_dx)
        for buf, view in outs:
            assert st.canary_intact(buf, view, CANARY)
            assert torch.isfinite(view).all() and not (view == CANARY).any()
        plain, _ = _direct(case, _plain_in, _plain_out, want_dx)
        assert torch.equal(views["out"], views["out_peer"])
        for k in ("out", "saved", "grad_in") + (("grad_params",) if st.n_blocks(B) == 1 else ()):
            assert (views[k] is None and plain[k] is None) or torch.equal(views[k], plain[k]), k
    # and through the wrapper's own peer buffer
    x, p, _ = _dev(case)
    o, _, peer = stage_forward(x, p, case.spec, peer_device=DEV, force_peer=True)
    assert peer.data_ptr() != o.data_ptr() and torch.equal(o, peer) and torch.equal(o, views["out"])


@_edge
def test_lanes_past_the_batch_read_nothing(key, B):
    """``x``, ``saved``, ``out`` and ``grad_out`` as views whose surroundings are NaN: the results
    are finite and, in one block, bitwise those with zero surroundings and equal run to run; with
    atomics (B = 1025) within the fp64 bound."""
    case = st.get_case(key, B)
    cell = st.Cell("bwd_dx", key, B)
    nan, _ = _direct(case, lambda t: st.guarded(t, float("nan")), _plain_out)
    zero, _ = _direct(case, lambda t: st.guarded(t, 0.0), _plain_out)
    again, _ = _direct(case, lambda t: st.guarded(t, 0.0), _plain_out)
    for k, v in nan.items():
        if v is None:
            continue
        assert torch.isfinite(v).all(), k
        if k != "grad_params" or st.n_blocks(B) == 1:
            assert torch.equal(v, zero[k]), k
            assert torch.equal(zero[k], again[k]), k
    got = {k: nan[k].cpu() for k in ("grad_params", "grad_in")}
    rec, fails = st.evaluate(cell, case, got, what="NaN surroundings")
    _report([rec], fails)

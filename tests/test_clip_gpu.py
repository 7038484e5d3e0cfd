"""Gradient clipping in the flat optimizer path on the GPU (csrc/optim.hip): the per-row
fp64 norm, the clipped update against the unclipped kernel (bitwise) and against
torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim, hipGraph replay, and the
Trainer's gradient_clip_val.  n_models = 2 everywhere: with an odd P row 1 starts off a
16-byte boundary."""
import copy
import os
import sys

import pytest
import torch

from distributed_training_pytorch_amd import _native as nat
from distributed_training_pytorch_amd.ops import optim as O
from distributed_training_pytorch_amd.ops.optim import FlatOptimizer, OptimConfig, flat_optimizer_step

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# the norm kernel's grid (csrc/optim.hip): a block takes CHUNK elements per grid-stride
# iteration, at most NB blocks per row -> with 16-byte aligned rows the first block runs a
# second iteration once P / 4 > NB * CHUNK / 4
CHUNK, NB = 4096, 256
STRIDE_P = NB * CHUNK + 4
ONE_BLOCK_P = 4096  # rows up to here: norm and update in one launch
SIZES = [1, 3, 5, 371, ONE_BLOCK_P, ONE_BLOCK_P + 1, STRIDE_P, STRIDE_P + 1]
STEP_SIZES = [371, ONE_BLOCK_P, ONE_BLOCK_P + 1, STRIDE_P + 1]


def _randn(P, seed, n=2):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, P, device=DEV, generator=g)


def _norm_ref(g):
    return torch.sqrt((g.double() ** 2).sum(1)).float()


def _assert_neighbour(got, ref):
    """Every element equals the reference or one of its two float32 neighbours."""
    up = torch.nextafter(ref, torch.full_like(ref, float("inf")))
    dn = torch.nextafter(ref, torch.full_like(ref, float("-inf")))
    ok = (got == ref) | (got == up) | (got == dn)
    assert ok.all(), (got.tolist(), ref.tolist())


def test_norm_grid_constants_are_the_librarys():
    lib = nat.require(DEV)
    blocks = lambda P: int(lib.dtp_grad_norm_ws_bytes(P)) // 8  # noqa: E731
    assert blocks(ONE_BLOCK_P) == 0 and blocks(ONE_BLOCK_P + 1) == 2
    assert blocks(CHUNK * (NB - 1)) == NB - 1 and blocks(CHUNK * NB) == NB and blocks(STRIDE_P + 1) == NB
    assert blocks(2 ** 31 - 1) == NB


@pytest.mark.parametrize("P", SIZES)
def test_grad_norm_is_the_fp64_norm_rounded(P):
    g = _randn(P, 10 + P % 97)
    print("P", P, "norm", O.grad_norm(g).tolist(), "ref", _norm_ref(g).tolist())
    _assert_neighbour(O.grad_norm(g), _norm_ref(g))
    _assert_neighbour(O.grad_norm(g, scale=0.5), _norm_ref(g * 0.5))
    a, b = O.grad_norm(g), O.grad_norm(g)
    assert torch.equal(a, b)
    out = torch.full((2,), -1.0, device=DEV)
    assert O.grad_norm(g, out=out) is out and torch.equal(out, a)
    z = torch.zeros(2, P, device=DEV)
    assert torch.equal(O.grad_norm(z), torch.zeros(2, device=DEV))
    # one row ([P]) is row 0 of the two
    assert torch.equal(O.grad_norm(g[0].contiguous()), a[:1])


@pytest.mark.parametrize("P", [5, 371, ONE_BLOCK_P + 1, STRIDE_P + 1])
def test_clip_grad_norm_op_scales_rows_by_torchs_coefficient(P):
    g = _randn(P, 3)
    g[0] *= 4  # row 0 above max_norm = 1 at every P here
    g[1] *= 1e-3 / P ** 0.5  # row 1 below it: untouched
    want_norm = O.grad_norm(g)
    coef = (1.0 / (want_norm + 1e-6)).clamp(max=1.0)
    want = g * coef.unsqueeze(1)
    got = g.clone()
    norm = O.clip_grad_norm_(got, 1.0)
    assert torch.equal(norm, want_norm)
    assert coef[0] < 1 and coef[1] == 1
    assert torch.equal(got, want) and torch.equal(got[1], g[1])


def _state(P, seed=1):
    p = _randn(P, seed) * 0.3
    return [p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(2, dtype=torch.int32, device=DEV)]


def _cfgs(kind, **clip):
    if kind == "adam":
        return OptimConfig("adam", lr=1e-2, **clip)
    return OptimConfig("sgd", lr=1e-2, momentum=0.9, **clip)


def _grads(P, steps=2):
    gs = []
    for k in range(steps):
        g = _randn(P, 20 + k)
        g[1] *= 1e-3 / P ** 0.5  # ||row 1 * grad_scale|| ~ 5e-4 < max_norm = 1 < ||row 0 * grad_scale||
        gs.append(g)
    return gs


@pytest.mark.parametrize("P", STEP_SIZES)
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_clipped_step_is_bitwise_the_unclipped_step_on_the_scaled_gradient(kind, P):
    """The clipped step = the unclipped kernel on (g * grad_scale) * coef, coef formed with
    torch's own expression from the norm the clipped step reports: params, m, v and step
    bitwise.  Row 0 is clipped, row 1 is not (and equals the unclipped step on the raw
    gradient).  Also zero_grad=True (gradient zero afterwards, same results) and a bf16
    shadow of the updated parameters."""
    MAXN, GS = 1.0, 0.5
    clip, plain = _cfgs(kind, max_grad_norm=MAXN), _cfgs(kind)
    a, b, raw, zg = _state(P), _state(P), _state(P), _state(P)
    ld = (P + 255) // 256 * 256
    shadow = torch.zeros(2, ld, dtype=torch.bfloat16, device=DEV)
    norm = torch.full((2,), -1.0, device=DEV)
    for g in _grads(P):
        flat_optimizer_step(*a, g.reshape(-1).clone(), clip, grad_scale=GS, norm_out=norm, shadow=shadow)
        _assert_neighbour(norm, _norm_ref(g * GS))
        coef = (MAXN / (norm + 1e-6)).clamp(max=1.0)
        assert coef[0] < 1 and coef[1] == 1, coef
        scaled = (g * GS) * coef.unsqueeze(1)
        flat_optimizer_step(*b, scaled.reshape(-1), plain)
        flat_optimizer_step(*raw, g.reshape(-1).clone(), plain, grad_scale=GS)
        gz = g.reshape(-1).clone()
        nz = torch.full((2,), -1.0, device=DEV)
        flat_optimizer_step(*zg, gz, clip, grad_scale=GS, norm_out=nz, zero_grad=True)
        assert not gz.any() and torch.equal(nz, norm)
        for x, y, z, r in zip(a, b, zg, raw):
            assert torch.equal(x, y) and torch.equal(x, z)
            assert torch.equal(x[1], r[1])
        assert not torch.equal(a[0][0], raw[0][0])  # clipping row 0 changed its update
        assert torch.equal(shadow[:, :P], a[0].bfloat16())
    assert a[3].tolist() == [2, 2]


@pytest.mark.parametrize("P", STEP_SIZES)
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_value_clipped_step_is_bitwise_the_unclipped_step_on_the_clamped_gradient(kind, P):
    CV, GS = 0.25, 0.5
    clip, plain = _cfgs(kind, clip_grad_value=CV), _cfgs(kind)
    a, b, zg = _state(P), _state(P), _state(P)
    ld = (P + 255) // 256 * 256
    shadow = torch.zeros(2, ld, dtype=torch.bfloat16, device=DEV)
    for k in range(2):
        g = _randn(P, 40 + k)
        clamped = (g * GS).clamp(min=-CV, max=CV)
        assert ((g * GS).abs() > CV).any() and ((g * GS).abs() < CV).any()
        flat_optimizer_step(*a, g.reshape(-1).clone(), clip, grad_scale=GS, shadow=shadow)
        flat_optimizer_step(*b, clamped.reshape(-1), plain)
        gz = g.reshape(-1).clone()
        flat_optimizer_step(*zg, gz, clip, grad_scale=GS, zero_grad=True)
        assert not gz.any()
        for x, y, z in zip(a, b, zg):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert torch.equal(shadow[:, :P], a[0].bfloat16())


def test_norm_and_value_together_are_rejected():
    with pytest.raises(ValueError):
        OptimConfig(max_grad_norm=1.0, clip_grad_value=1.0)
    cfg = OptimConfig()
    cfg.max_grad_norm = cfg.clip_grad_value = 1.0
    with pytest.raises(ValueError):
        flat_optimizer_step(*_state(8), torch.zeros(16, device=DEV), cfg)
    # and by the native entry point itself
    lib = nat.require(DEV)
    p, m, v, st = _state(8)
    g, n = torch.zeros(16, device=DEV), torch.zeros(2, device=DEV)
    args = nat.OptArgs(nat.ptr(p), nat.ptr(m), nat.ptr(v), nat.ptr(st), nat.ptr(g), None, 0, 2, 8, nat.MODE_ADAM, 1.0, 0,
                       OptimConfig().hyper(), None, 0, 1.0, 1.0, None, nat.ptr(n))
    import ctypes

    assert lib.dtp_flat_optimizer(ctypes.byref(args), nat.stream_ptr()) != 0


@pytest.mark.parametrize("P", [371, ONE_BLOCK_P + 1])
@pytest.mark.parametrize("kind,algo", [("adam", "norm"), ("sgd", "norm"), ("adam", "value"), ("sgd", "value")])
def test_clipped_steps_match_torch_clipping_and_optimizer(kind, algo, P):
    """Five steps of torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim per
    row, at the tolerance tests/test_loss_optim_gpu.py holds this kernel to."""
    C = 2.0 if algo == "norm" else 0.5
    cfg = _cfgs(kind, **({"max_grad_norm": C} if algo == "norm" else {"clip_grad_value": C}))
    p, m, v, st = _state(P)
    ps = [torch.nn.Parameter(p[i].clone()) for i in range(2)]
    opts = [_cfgs(kind).torch_optimizer([q]) for q in ps]
    norm = torch.zeros(2, device=DEV)
    for k in range(5):
        g = _randn(P, 60 + k)
        for i in range(2):
            ps[i].grad = g[i].clone()
            if algo == "norm":
                tn = torch.nn.utils.clip_grad_norm_([ps[i]], C)
            else:
                torch.nn.utils.clip_grad_value_([ps[i]], C)
            opts[i].step()
        flat_optimizer_step(p, m, v, st, g.reshape(-1), cfg, norm_out=norm)
        if algo == "norm":
            torch.testing.assert_close(norm[1], tn, rtol=1e-6, atol=0)
    torch.testing.assert_close(p, torch.stack([q.detach() for q in ps]), rtol=1e-6, atol=1e-7)
    assert st.tolist() == [5, 5]


@pytest.mark.parametrize("P", [371, ONE_BLOCK_P + 1])
def test_zero_gradient_leaves_no_nan(P):
    for kind in ("adam", "sgd"):
        p, m, v, st = _state(P)
        p0 = p.clone()
        norm = torch.full((2,), -1.0, device=DEV)
        flat_optimizer_step(p, m, v, st, torch.zeros(2 * P, device=DEV), _cfgs(kind, max_grad_norm=1.0), norm_out=norm)
        assert torch.equal(norm, torch.zeros(2, device=DEV))
        assert torch.isfinite(p).all() and torch.equal(p, p0)  # coefficient 1, zero update


@pytest.mark.parametrize("P", [371, ONE_BLOCK_P + 1])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_norm_propagates_as_in_torch(bad, P):
    """clip_grad_norm_(error_if_nonfinite=False): an infinite norm gives coefficient 0 (and
    inf * 0 = NaN in the element that caused it), a NaN norm a NaN coefficient -- row 0;
    row 1 stays finite and is updated as usual."""
    g = _randn(P, 5)
    g[0, P // 2] = bad
    p, m, v, st = _state(P)
    ps = [torch.nn.Parameter(p[i].clone()) for i in range(2)]
    opts = [torch.optim.SGD([q], lr=1e-2) for q in ps]
    for i in range(2):
        ps[i].grad = g[i].clone()
        torch.nn.utils.clip_grad_norm_([ps[i]], 1.0)
        opts[i].step()
    norm = torch.zeros(2, device=DEV)
    flat_optimizer_step(p, m, v, st, g.reshape(-1), OptimConfig("sgd", lr=1e-2, max_grad_norm=1.0), norm_out=norm)
    want = torch.stack([q.detach() for q in ps])
    assert not torch.isfinite(norm[0]) and torch.isfinite(norm[1]) and torch.isfinite(p[1]).all()
    assert torch.equal(torch.isnan(p), torch.isnan(want)) and torch.isnan(p[0]).any()
    torch.testing.assert_close(p, want, rtol=1e-6, atol=1e-7, equal_nan=True)


@pytest.mark.parametrize("P", [371, ONE_BLOCK_P + 1])
def test_clipped_flat_optimizer_replays_in_a_graph(P):
    """A backward-free body (fill the gradient, clipped FlatOptimizer.step) replayed as a
    hipGraph is bitwise the eager run over 3 steps; nothing is allocated under capture."""
    from distributed_training_pytorch_amd.engine.graph_step import CapturedStep

    gs = [_randn(P, 80 + k) for k in range(3)]

    def run(enabled):
        params, grad, src = _randn(P, 7) * 0.3, torch.zeros(2, P, device=DEV), torch.zeros(2, P, device=DEV)
        opt = FlatOptimizer(params, grad, OptimConfig("adam", lr=1e-2, max_grad_norm=1.0))
        norms = []

        def body(_key):
            grad.copy_(src)
            opt.step(zero_grad=True)

        st = CapturedStep(body, DEV, warmup=1, enabled=enabled)
        for g in gs:
            src.copy_(g)
            st.run(0)
            norms.append(opt.grad_norm.clone())
        torch.cuda.synchronize()
        return [params, opt.m, opt.v, opt.step_ctr, grad, *norms], st

    eager, _ = run(False)
    graph, st = run(True)
    assert st.is_captured(0) and st.replays >= 2
    for a, b in zip(eager, graph):
        assert torch.equal(a, b)
    assert graph[3].tolist() == [3, 3] and not graph[4].any()
    for n, g in zip(graph[5:], gs):
        _assert_neighbour(n, _norm_ref(g))


def test_fused_stage_backward_refuses_clip_fields():
    """dtp_mlp_stage_bwd_opt cannot clip (the backward is still writing the gradient):
    error code, nothing launched; FlatOptimizer.step launches the backwards first."""
    import ctypes

    lib = nat.require(DEV)
    o = nat.OptArgs()
    o.max_norm = 1.0
    m = nat.StageMulti()
    assert lib.dtp_mlp_stage_bwd_opt(ctypes.byref(m), ctypes.byref(o), 2, 10, 5, 1, 0, nat.stream_ptr()) != 0
    assert b"clipping" in lib.dtp_last_error()


def test_clipped_flat_optimizer_launches_deferred_backwards_first():
    """ParamBackwardFusion + a clipping FlatOptimizer: same results as without the window."""
    import contextlib

    from distributed_training_pytorch_amd.models.toy import ToyModel
    from distributed_training_pytorch_amd.ops.loss import mse_loss
    from distributed_training_pytorch_amd.ops.mlp import ParamBackwardFusion
    from distributed_training_pytorch_amd.parallel.ddp import FlatDDP

    def train(fuse):
        torch.manual_seed(5)
        ddp = FlatDDP(ToyModel().cuda())
        opt = FlatOptimizer(ddp.flat_params, ddp.flat_grad, OptimConfig("sgd", lr=5e-2, momentum=0.9, max_grad_norm=0.05))
        gen = torch.Generator(device="cuda").manual_seed(1)
        norms = []
        for _ in range(3):
            x = torch.randn(200, 2, device="cuda", generator=gen)
            y = torch.randn(200, 1, device="cuda", generator=gen)
            ddp.zero_grad()
            with (ParamBackwardFusion() if fuse else contextlib.nullcontext()) as fus:
                mse_loss(ddp(x), y).backward()
                opt.step(zero_grad=True, fused=fus.take() if fus is not None else None)
            norms.append(opt.grad_norm.clone())
        return [ddp.flat_params.detach().clone(), opt.m.clone(), *norms]

    for a, b in zip(train(False), train(True)):
        assert torch.equal(a, b)
    assert all(n.item() > 0.05 for n in train(True)[2:])


# ----------------------------------------------------------------------------- Trainer
def _lit(opt_name):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from demo_pytorch_lightning import LitToyModel

    if opt_name == "adam":
        return LitToyModel()

    class LitSgd(LitToyModel):
        def configure_optimizers(self):
            return [torch.optim.SGD(self.model_X.parameters(), lr=5e-2, momentum=0.9),
                    torch.optim.SGD(self.model_Y.parameters(), lr=5e-2, momentum=0.9)]

    return LitSgd()


def _torch_loop(init_layers, make_opt, dl, clip, steps):
    """PL 1.5 per optimizer on fp64 twins: backward, clip_grad_norm_ over that optimizer's
    parameters, step.  The two models are independent.  Returns their flat parameters and
    the smallest norm seen before clipping."""
    out, low = [], float("inf")
    for layers in init_layers:
        twin = copy.deepcopy(layers).double().cpu()
        opt = make_opt(twin.parameters())
        for k, (x, y) in enumerate(dl):
            if k == steps:
                break
            opt.zero_grad()
            torch.nn.functional.mse_loss(twin(x.double()), y.double()).backward()
            if clip:
                low = min(low, float(torch.nn.utils.clip_grad_norm_(twin.parameters(), clip)))
            opt.step()
        out.append(torch.nn.utils.parameters_to_vector(twin.parameters()).detach())
    return out, low


# Adam's update is invariant to the gradient's scale but for eps: a clip value that brings
# the gradient to eps' order makes clipping visible there; SGD sees any binding value
@pytest.mark.parametrize("opt_name,clip", [("adam", 1e-7), ("sgd", 0.05)])
def test_trainer_gradient_clip_val_matches_torch_loop(tmp_path, opt_name, clip):
    """LitToyModel through the Trainer's module path, 4 batches that all clip, against
    clip_grad_norm_ + torch.optim per optimizer on fp64 twins -- at the tolerance
    tests/test_module_path_gpu.py holds the module path to against its fp64 loop
    (rtol 1e-4, atol 2e-5), which the unclipped loop must miss by far."""
    from distributed_training_pytorch_amd.data.toy_data import ToyData
    from distributed_training_pytorch_amd.trainer import Trainer

    nat.require(DEV)
    rtol, atol = 1e-4, 2e-5
    torch.manual_seed(0)
    dl = torch.utils.data.DataLoader(ToyData(seed=0), batch_size=128)
    model = _lit(opt_name)
    init = [copy.deepcopy(model.model_X.layers), copy.deepcopy(model.model_Y.layers)]
    if opt_name == "adam":
        make = lambda ps: torch.optim.Adam(ps, lr=1e-3)  # noqa: E731
    else:
        make = lambda ps: torch.optim.SGD(ps, lr=5e-2, momentum=0.9)  # noqa: E731
    want, low = _torch_loop(init, make, dl, clip, 4)
    plain, _ = _torch_loop(init, make, dl, 0.0, 4)
    assert low > clip  # every step clipped
    tr = Trainer(gpus=1, max_steps=4, accelerator="gpu", log_every_n_steps=1, default_root_dir=str(tmp_path),
                 enable_progress_bar=False, enable_checkpointing=False, engine="auto", gradient_clip_val=clip)
    tr.fit(model, dl)
    assert tr.engine_used == "module" and "clipping" in (tr.fused_refused or "")
    assert all(f is not None and f.flat.cfg.max_grad_norm == clip for f in tr._flat_opts)  # the flat kernel clipped
    for m, w, pl in zip((model.model_X, model.model_Y), want, plain):
        got = torch.nn.utils.parameters_to_vector(m.layers.parameters()).detach().cpu().double()
        far = (w - pl).abs() > 10 * (atol + rtol * pl.abs())
        assert far.double().mean() >= 0.25, far.double().mean()
        torch.testing.assert_close(got, w, rtol=rtol, atol=atol)


def test_trainer_fused_engine_with_clipping_raises(tmp_path):
    from distributed_training_pytorch_amd.data.toy_data import ToyData
    from distributed_training_pytorch_amd.trainer import Trainer

    dl = torch.utils.data.DataLoader(ToyData(seed=0), batch_size=128)
    tr = Trainer(gpus=1, max_steps=2, accelerator="gpu", default_root_dir=str(tmp_path), enable_progress_bar=False,
                 enable_checkpointing=False, engine="fused", gradient_clip_val=0.5)
    with pytest.raises(RuntimeError, match="clipping"):
        tr.fit(_lit("adam"), dl)

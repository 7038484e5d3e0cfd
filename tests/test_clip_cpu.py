"""Gradient clipping without a GPU: the CPU branch of flat_optimizer_step and the public
norm ops against torch, the Trainer's gradient_clip_val on accelerator="cpu", the CLI
flags, and demo.py --clip_grad_norm on two gloo ranks."""
import copy
import os
import sys

import pytest
import torch

from distributed_training_pytorch_amd.ops import optim as O
from distributed_training_pytorch_amd.ops.optim import FlatOptimizer, OptimConfig, flat_optimizer_step

from .test_launchers_cpu import COMMON, _run_torchrun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(kind, **clip):
    if kind == "adam":
        return OptimConfig("adam", lr=1e-2, **clip)
    return OptimConfig("sgd", lr=1e-2, momentum=0.9, **clip)


@pytest.mark.parametrize("kind,algo", [("adam", "norm"), ("sgd", "norm"), ("adam", "value"), ("sgd", "value")])
def test_cpu_branch_matches_torch_clipping_and_optimizer(kind, algo):
    P, C = 371, (2.0 if algo == "norm" else 0.5)
    torch.manual_seed(3)
    cfg = _cfg(kind, **({"max_grad_norm": C} if algo == "norm" else {"clip_grad_value": C}))
    p = torch.randn(2, P) * 0.3
    m, v, st = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(2, dtype=torch.int32)
    ps = [torch.nn.Parameter(p[i].clone()) for i in range(2)]
    opts = [_cfg(kind).torch_optimizer([q]) for q in ps]
    norm = torch.zeros(2)
    for _ in range(5):
        g = torch.randn(2, P)
        g[1] *= 1e-2  # row 1 never clips by norm
        tn = []
        for i in range(2):
            ps[i].grad = g[i].clone()
            if algo == "norm":
                tn.append(torch.nn.utils.clip_grad_norm_([ps[i]], C))
            else:
                torch.nn.utils.clip_grad_value_([ps[i]], C)
            opts[i].step()
        flat_optimizer_step(p, m, v, st, g.reshape(-1), cfg, norm_out=norm)
        if algo == "norm":
            torch.testing.assert_close(norm, torch.stack(tn), rtol=1e-6, atol=0)
            assert norm[0] > C > norm[1]
    torch.testing.assert_close(p, torch.stack([q.detach() for q in ps]), rtol=1e-6, atol=1e-7)
    assert st.tolist() == [5, 5]


def test_cpu_norm_ops_and_flat_optimizer_grad_norm():
    torch.manual_seed(0)
    g = torch.randn(2, 37)
    g[1] *= 1e-3
    ref = torch.sqrt((g.double() ** 2).sum(1)).float()
    assert torch.equal(O.grad_norm(g), ref)
    assert torch.equal(O.grad_norm(g, scale=0.5), torch.sqrt(((g * 0.5).double() ** 2).sum(1)).float())
    h = g.clone()
    n = O.clip_grad_norm_(h, 1.0)
    assert torch.equal(n, ref) and torch.equal(h[1], g[1])
    torch.testing.assert_close(h[0].norm(), torch.tensor(1.0), rtol=1e-5, atol=0)
    with pytest.raises(ValueError):
        O.clip_grad_norm_(h, 0.0)
    # all-zero gradient: coefficient 1, no NaN
    p = torch.randn(2, 37)
    p0 = p.clone()
    opt = FlatOptimizer(p, torch.zeros(2, 37), OptimConfig("adam", max_grad_norm=1.0))
    opt.step()
    assert torch.equal(opt.grad_norm, torch.zeros(2)) and torch.equal(p, p0)
    with pytest.raises(ValueError):
        OptimConfig(max_grad_norm=1.0, clip_grad_value=0.5)


def _lit(opt_name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from demo_pytorch_lightning import LitToyModel

    if opt_name == "adam":
        return LitToyModel()

    class LitSgd(LitToyModel):
        def configure_optimizers(self):
            return [torch.optim.SGD(self.model_X.parameters(), lr=5e-2, momentum=0.9),
                    torch.optim.SGD(self.model_Y.parameters(), lr=5e-2, momentum=0.9)]

    return LitSgd()


def _torch_loop(init_layers, make_opt, dl, clip, algo, steps):
    """PL 1.5 per optimizer on fp64 twins: backward, clip that optimizer's parameters, step."""
    out, bound = [], 0
    for layers in init_layers:
        twin = copy.deepcopy(layers).double()
        opt = make_opt(twin.parameters())
        for k, (x, y) in enumerate(dl):
            if k == steps:
                break
            opt.zero_grad()
            torch.nn.functional.mse_loss(twin(x.double()), y.double()).backward()
            if clip and algo == "norm":
                bound += float(torch.nn.utils.clip_grad_norm_(twin.parameters(), clip)) > clip
            elif clip:
                bound += any(float(q.grad.abs().max()) > clip for q in twin.parameters())
                torch.nn.utils.clip_grad_value_(twin.parameters(), clip)
            opt.step()
        out.append(torch.nn.utils.parameters_to_vector(twin.parameters()).detach())
    return out, bound


# Adam's update is invariant to the gradient's scale but for eps: the norm is clipped to
# eps' order there (norm 1e-7, elements 1e-8), so that clipping shows; SGD sees any bound
@pytest.mark.parametrize("opt_name,algo,clip", [("adam", "norm", 1e-7), ("sgd", "norm", 0.05),
                                                ("adam", "value", 1e-8), ("sgd", "value", 0.02)])
def test_trainer_gradient_clip_val_cpu_matches_torch_loop(tmp_path, opt_name, algo, clip):
    from distributed_training_pytorch_amd.data.toy_data import ToyData
    from distributed_training_pytorch_amd.trainer import Trainer

    rtol, atol = 1e-4, 2e-5
    torch.manual_seed(0)
    dl = torch.utils.data.DataLoader(ToyData(seed=0), batch_size=128)
    model = _lit(opt_name)
    init = [copy.deepcopy(model.model_X.layers), copy.deepcopy(model.model_Y.layers)]
    if opt_name == "adam":
        make = lambda ps: torch.optim.Adam(ps, lr=1e-3)  # noqa: E731
    else:
        make = lambda ps: torch.optim.SGD(ps, lr=5e-2, momentum=0.9)  # noqa: E731
    want, bound = _torch_loop(init, make, dl, clip, algo, 4)
    plain, _ = _torch_loop(init, make, dl, 0.0, algo, 4)
    assert bound == 8  # both optimizers clipped at every step
    tr = Trainer(max_steps=4, accelerator="cpu", log_every_n_steps=1, default_root_dir=str(tmp_path),
                 enable_progress_bar=False, enable_checkpointing=False, gradient_clip_val=clip,
                 gradient_clip_algorithm=algo)
    tr.fit(model, dl)
    assert tr.engine_used == "module" and "clipping" in (tr.fused_refused or "")
    for m, w, pl in zip((model.model_X, model.model_Y), want, plain):
        got = torch.nn.utils.parameters_to_vector(m.layers.parameters()).detach().double()
        far = (w - pl).abs() > 10 * (atol + rtol * pl.abs())
        assert far.double().mean() >= 0.1, far.double().mean()
        torch.testing.assert_close(got, w, rtol=rtol, atol=atol)


def test_trainer_rejects_a_bad_algorithm_and_fused_with_clipping(tmp_path):
    from distributed_training_pytorch_amd.data.toy_data import ToyData
    from distributed_training_pytorch_amd.trainer import Trainer

    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        Trainer(gradient_clip_val=0.5, gradient_clip_algorithm="nrom")
    assert Trainer().gradient_clip_val == 0 and Trainer(gradient_clip_val=None).gradient_clip_val == 0
    tr = Trainer(max_steps=1, accelerator="cpu", default_root_dir=str(tmp_path), enable_progress_bar=False,
                 enable_checkpointing=False, engine="fused", gradient_clip_val=0.5)
    with pytest.raises(RuntimeError, match="clipping"):
        tr.fit(_lit("adam"), torch.utils.data.DataLoader(ToyData(seed=0), batch_size=128))


def test_parsers_take_one_clipping_flag():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import argument_parser
    import demo_one_model_multi_gpu
    import demo_pytorch_lightning

    a = argument_parser.get_args([])
    assert a.clip_grad_norm == 0 and a.clip_grad_value == 0
    assert argument_parser.get_args(["--clip_grad_norm", "0.5"]).clip_grad_norm == 0.5
    assert argument_parser.get_args(["--clip_grad_value", "0.25"]).clip_grad_value == 0.25
    for get in (argument_parser.get_args, demo_pytorch_lightning.get_args):
        with pytest.raises(SystemExit):
            get(["--clip_grad_norm", "0.5", "--clip_grad_value", "0.25"])
    # the layer-split demo refuses them before it touches a device or a process group
    with pytest.raises(SystemExit, match="clip_grad"):
        demo_one_model_multi_gpu.main(["--clip_grad_norm", "0.5", "--device", "cpu", "--backend", "gloo"])


def test_runner_config_carries_the_flags():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import argument_parser
    from distributed_training_pytorch_amd.engine import runner

    cfg = runner._optim(argument_parser.get_args(["--clip_grad_norm", "0.5"]))
    assert cfg.max_grad_norm == 0.5 and cfg.clip_grad_value == 0 and cfg.clips
    cfg = runner._optim(argument_parser.get_args(["--clip_grad_value", "0.25"]))
    assert cfg.clip_grad_value == 0.25 and cfg.max_grad_norm == 0
    assert not runner._optim(argument_parser.get_args([])).clips


def test_stock_loop_clips_each_model_with_torchs_functions():
    """The stock baseline: clip_grad_norm_ / clip_grad_value_ per model between the
    backwards and the two Adam steps (bounds of eps' order, so Adam shows them)."""
    from distributed_training_pytorch_amd.baselines.stock import StockLoop
    from distributed_training_pytorch_amd.data.toy_data import ToyData

    def run(**clip):
        loop = StockLoop(ToyData(seed=0), torch.device("cpu"), batch=128, seed=3, ddp=False, **clip)
        seen = []
        real = loop.ox.step

        def spy(*a, **k):  # the gradients the first optimizer steps on
            seen.append(torch.cat([q.grad.reshape(-1) for q in loop.mx.parameters()]).clone())
            return real(*a, **k)

        loop.ox.step = spy
        loop.train(2)
        return torch.nn.utils.parameters_to_vector(loop.mx.parameters()).detach(), seen

    plain, g0 = run()
    by_norm, g1 = run(clip_grad_norm=1e-7)
    by_value, g2 = run(clip_grad_value=1e-8)
    assert g0[0].norm() > 1e-3
    torch.testing.assert_close(g1[0].norm(), torch.tensor(1e-7), rtol=1e-4, atol=0)
    torch.testing.assert_close(g1[0], g0[0] * (1e-7 / (g0[0].norm() + 1e-6)), rtol=1e-5, atol=0)
    assert torch.equal(g2[0], g0[0].clamp(-1e-8, 1e-8))
    assert not torch.equal(plain, by_norm) and not torch.equal(plain, by_value)


def _summary(out: str) -> dict:
    """Rank 0's run summary.  The two ranks share the pipe: the dict is one write, but the
    other rank's next line can land before its newline, so the dict is cut at its closing
    brace instead of at the end of the line."""
    start = out.rindex("summary: ") + len("summary: ")
    depth = 0
    for end in range(start, len(out)):
        depth += (out[end] in "{[(") - (out[end] in "}])")
        if depth == 0:
            return eval(out[start:end + 1], {"nan": float("nan"), "inf": float("inf")})
    raise AssertionError(f"no complete summary in:\n{out[-2000:]}")


def test_demo_two_gloo_ranks_clip_grad_norm():
    """demo.py --engine module --clip_grad_norm X on two gloo ranks: the replicas stay
    bitwise equal, and the losses are not the unclipped run's.  X comes from the run itself:
    one iteration with a bound that cannot bind reports the first step's norms (the run
    summary's grad_norm), and X is a tenth of the smaller one."""
    base = ["--nproc-per-node", "2", "demo.py", "--torchrun", *COMMON, "--engine", "module", "--optimizer", "sgd",
            "--lr", "0.05"]
    probe = _run_torchrun([*base, "--iters", "1", "--clip_grad_norm", "1e9"])
    assert probe.returncode == 0, probe.stderr[-3000:]
    first = _summary(probe.stdout)["grad_norm"]
    assert len(first) == 2 and all(0 < n < 1e9 for n in first), first
    x = 0.1 * min(first)
    plain = _run_torchrun(base)
    assert plain.returncode == 0, plain.stderr[-3000:]
    clipped = _run_torchrun([*base, "--clip_grad_norm", repr(x)])
    assert clipped.returncode == 0, clipped.stderr[-3000:]
    sp, sc = _summary(plain.stdout), _summary(clipped.stdout)
    assert sp["iters"] == sc["iters"] == 20 and "grad_norm" not in sp
    assert all(v == v for v in sc["final_loss"]) and sc["final_loss"] != sp["final_loss"], (sc, sp)
    # --engine fused with the flag falls to the module engine
    fell = _run_torchrun(["--nproc-per-node", "2", "demo.py", "--torchrun", *COMMON, "--engine", "fused", "--iters", "2",
                          "--clip_grad_norm", repr(x)])
    assert fell.returncode == 0, fell.stderr[-3000:]
    assert _summary(fell.stdout)["engine"] == "module" and "using the module engine" in fell.stdout, fell.stdout[-2000:]

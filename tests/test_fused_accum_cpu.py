"""Gradient accumulation in the fused engine, the parts that need no GPU: the twin table against
the cells of ``tests/accum_cases.py``, the cells' input conditions from the references alone, the
CPU engine's read-out and trajectory against the fp64 loop, the evaluation catching wrong
answers, and the checkpoint's ``accumulate``."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

from distributed_training_pytorch_amd.data.sampler import EpochIndexStream
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig
from distributed_training_pytorch_amd.ops.optim import OptimConfig
from distributed_training_pytorch_amd.ops.schedule import LrSchedule

from . import accum_cases as ac
from . import step_cases as sc
from .sched_cases import torch_train_sched

CPU = torch.device("cpu")


# ------------------------------------------------------------------------------ the table
def test_every_twin_has_a_cell_and_every_cell_names_a_twin():
    named = {c.twin for c in ac.CELLS}
    assert len(ac.TWINS) == len(set(ac.TWINS)) == 2 * 8 + 2 * 5
    missing = [t for t in ac.TWINS if t not in named]
    assert not missing, f"twins without a cell: {missing}"
    stray = [c.id for c in ac.CELLS if c.twin not in ac.TWINS]
    assert not stray, f"cells that name no twin: {stray}"
    # the cell with two empty members has 4 members: it names the constant-count twin
    assert ac.BY_ID["T-adam-mse-fp32-b200-gon-A3"].twin[-1] == "grp4"
    # the twins are those of the plain 4-wave lanes / split-batch instances of step_cases' table
    plain = {(s, L, w, lo, o, p, k) for s, L, w, lo, o, p, k in sc.INSTANCES if w == 4 and k in ("lanes", "grp")}
    assert {t[:6] + ("grp" if t[6] == "grp4" else t[6],) for t in ac.TWINS} == plain


def test_geometries_read_the_ragged_batch_and_cross_or_fill_an_epoch():
    for c in ac.CELLS:
        g = sc.cell_geom(c.cell)
        spe = g.steps_per_epoch
        micro = [u for t in ac.READOUT_STEPS for u in range(t * c.A, (t + 1) * c.A)]
        sizes = [len(EpochIndexStream(g).indices(u)) for u in micro]
        edge = any((t * c.A) // spe != ((t + 1) * c.A - 1) // spe for t in ac.READOUT_STEPS)
        # (batch 200 at A = 3 and batch 256 at A = 2: a window is a whole epoch)
        assert edge or c.A == spe, c.id
        if c.cell.n % c.cell.batch:
            assert min(sizes) < c.cell.batch, c.id  # the ragged batch is read


# ------------------------------------------------------------------------------ the CPU engine
@pytest.mark.parametrize("cell", ac.CELLS, ids=[c.id for c in ac.CELLS])
def test_cpu_engine_readout_and_input_conditions(cell):
    """The reference path of the engine (``_reference_step``) is held to the same read-out as the
    kernels, and the cell's inputs meet ``step_cases.check_conditions`` along its trajectory."""
    if cell.cell.prec == "bf16":
        # the CPU engine computes in fp32: the bf16 cell's conditions (Y, D) come from the references
        recs, fails = ac.run_accum_cell(dataclasses.replace(cell, cell=dataclasses.replace(cell.cell, prec="fp32")),
                                        CPU, expect_native=False)
        assert not fails, "\n".join(fails)
        X, Y = sc.cell_data(cell.cell)
        recs = []
        tr = ac.make_trainer(cell, CPU, precision="fp32")
        for t in ac.READOUT_STEPS:
            sg = sc.StepGradient(t, tr.params.detach().clone(), None, None, None)
            recs += ac.evaluate_window(cell, sg, ac.window_indices(cell, t), X, Y)[0]
            tr.train(1)
    else:
        recs, fails = ac.run_accum_cell(cell, CPU, expect_native=False)
        assert not fails, "\n".join(fails)
    assert len(recs) == len(ac.READOUT_STEPS) * sc.N_MODELS
    bad = sc.check_conditions(cell.cell, recs)
    assert not bad, "\n".join(bad)


def test_cpu_engine_trajectory_matches_the_fp64_loop():
    """12 optimizer steps at n = 300, batch 64, A = 3, Adam with weight decay under a cosine
    schedule with 2 warm-up steps, against the fp64 loop extended by accumulation."""
    cell = ac.LANES4
    ocfg = trajectory_optim()
    X, Y = sc.cell_data(cell.cell)
    ref_p, ref_l = torch_train_sched(cell.cell.spec, sc.cell_init(cell.cell), X, Y, ac.window_views(cell.cell, cell.A),
                                     12, ocfg)
    tr = ac.make_trainer(cell, CPU, ocfg)
    tr.train(12)
    assert tr.t == 12 and tr.step_ctr.tolist() == [12, 12]
    torch.testing.assert_close(tr.losses(0, 12), ref_l, rtol=2e-4, atol=1e-5)
    torch.testing.assert_close(tr.params, ref_p, rtol=1e-4, atol=0)
    # accumulation matters: the plain engine over the same 12 steps ends elsewhere
    pl = ac.make_trainer(cell, CPU, ocfg, A=1)
    pl.train(12)
    assert not torch.allclose(pl.params, ref_p, rtol=1e-3, atol=1e-4)


def trajectory_optim() -> OptimConfig:
    return OptimConfig(lr=1e-2, weight_decay=1e-2,
                       schedule=LrSchedule.make("cosine", 1e-2, warmup_iters=2, decay_iters=12, min_ratio=0.1))


# ------------------------------------------------------------------------------ wrong answers are caught
def _fp32_window(cell, p, idx, X, Y, scale=None, sizes=None):
    """fp32 autograd over the window's micro-batches as a (gradient [n, P], loss [n]) read-out;
    ``sizes``: divide micro-batch j's sums by sizes[j] instead of its own count."""
    gs, ls = [], []
    for i in range(sc.N_MODELS):
        g, lo = None, None
        for j, ix in enumerate(idx):
            ix_t = torch.tensor(ix, dtype=torch.long)
            gr, lr = sc.autograd_gradient(cell.cell.spec, p[i], X[ix_t], Y[ix_t], cell.cell.loss, torch.float32)
            if sizes is not None:
                gr, lr = gr * (len(ix) / sizes[j]), lr * (len(ix) / sizes[j])
            g, lo = (gr, lr) if g is None else (g + gr, lo + lr)
        s = torch.tensor(1.0 / len(idx) if scale is None else scale, dtype=torch.float32)
        gs.append(g * s)
        ls.append(lo * s)
    return torch.stack(gs), torch.stack(ls)


def test_evaluation_catches_wrong_answers():
    cell = ac.LANES4  # windows (0 1 2) (3 4 | 0): step 1 holds the ragged batch and the epoch edge
    X, Y = sc.cell_data(cell.cell)
    p = torch.stack(sc.cell_init(cell.cell))
    t = 1
    idx = ac.window_indices(cell, t)
    assert [len(ix) for ix in idx] == [64, 44, 64]

    def fails_of(g, lo):
        # (no parameters after the step here: the check of the applied step is not part of this)
        sg = sc.StepGradient(t, p, g, lo, p - sc.ADAM.lr * torch.sign(g))
        _, f = ac.evaluate_window(cell, sg, idx, X, Y)
        return [m for m in f if "Adam:" not in m]

    g, lo = _fp32_window(cell, p, idx, X, Y)
    assert not fails_of(g, lo)
    # a gradient not divided by A
    g_sum, _ = _fp32_window(cell, p, idx, X, Y, scale=1.0)
    assert any("loss" not in m for m in fails_of(g_sum, lo))
    # the last micro-batch alone: its gradient, its loss
    g_last, lo_last = _fp32_window(cell, p, idx[-1:], X, Y)
    assert any("loss" not in m for m in fails_of(g_last, lo))
    assert any("loss" in m for m in fails_of(g, lo_last))
    # the ragged micro-batch divided by the full batch size
    g_rag, lo_rag = _fp32_window(cell, p, idx, X, Y, sizes=[64, 64, 64])
    assert any("loss" not in m for m in fails_of(g_rag, lo)) and any("loss" in m for m in fails_of(g, lo_rag))
    # the window shifted by one batch
    shifted = [v.indices(t) for v in ac.window_views(cell.cell, cell.A, shift=1)]
    g_sh, lo_sh = _fp32_window(cell, p, shifted, X, Y)
    assert any("loss" not in m for m in fails_of(g_sh, lo)) and any("loss" in m for m in fails_of(g, lo_sh))


# ------------------------------------------------------------------------------ configuration, checkpoints
def test_accumulate_is_validated_and_kept_in_the_checkpoint():
    cell = ac.LANES4
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="accumulate"):
            ac.make_trainer(cell, CPU, A=bad)
    assert EngineConfig().accumulate == 1
    tr = ac.make_trainer(cell, CPU)
    assert list(tr.micro_batches(2)) == [6, 7, 8] and not tr.accum_in_kernel
    tr.train(4)
    sd = tr.state_dict()
    assert sd["accumulate"] == 3
    fresh = ac.make_trainer(cell, CPU)
    fresh.load_state_dict(sd)
    fresh.train(4)
    whole = ac.make_trainer(cell, CPU)
    whole.train(8)
    for a, b in zip((fresh.params, fresh.m, fresh.v, fresh.losses(4, 8)), (whole.params, whole.m, whole.v, whole.losses(4, 8))):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="accumulate"):
        ac.make_trainer(cell, CPU, A=2).load_state_dict(sd)
    plain = ac.make_trainer(cell, CPU, A=1)
    with pytest.raises(ValueError, match="accumulate"):
        plain.load_state_dict(sd)
    sd1 = plain.state_dict()
    assert "accumulate" not in sd1  # a state dict without the key (any earlier checkpoint) counts as 1
    plain.load_state_dict(sd1)
    with pytest.raises(ValueError, match="accumulate"):
        tr.load_state_dict(sd1)


# ------------------------------------------------------------------------------ the entry points
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _demo(args, timeout=200):
    env = dict(os.environ, WANDB_MODE="dryrun")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "demo.py", *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                       env=env)
    assert r.returncode == 0 and "Finished" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if "summary:" in l][-1]
    return eval(line.split("summary:", 1)[1], {"nan": float("nan"), "inf": float("inf")}), r.stdout  # our own dict


def test_parser_flag_and_the_two_demos_refusals():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import argument_parser
    import demo_one_model_multi_gpu
    import demo_pytorch_lightning

    assert argument_parser.get_args([]).accumulate_grad_batches == 1
    assert argument_parser.get_args(["--accumulate_grad_batches", "3"]).accumulate_grad_batches == 3
    assert demo_pytorch_lightning.get_args([]).accumulate_grad_batches == 1
    # both refuse a value above 1 before they touch a device or a process group
    with pytest.raises(SystemExit, match="accumulate_grad_batches"):
        demo_one_model_multi_gpu.main(["--accumulate_grad_batches", "2", "--device", "cpu", "--backend", "gloo"])
    with pytest.raises(SystemExit, match="accumulate_grad_batches"):
        demo_pytorch_lightning.main(["--accumulate_grad_batches", "2"])


def test_module_engine_on_the_cpu_matches_the_stock_engine(tmp_path):
    """demo.py --device cpu --accumulate_grad_batches 3: the module engine's window (each loss
    scaled by 1/A through the backward seed, one flat-optimizer step) against the torch loop
    (loss / A, step on the last), same seed and data; and accumulation changes the run."""
    base = ["--device", "cpu", "--backend", "gloo", "--iters", "12", "--batch_size", "64", "--seed", "11", "--dry_run",
            "--no_progress"]
    res = {}
    for engine, A in (("stock", 3), ("module", 3), ("module", 1)):
        res[engine, A], out = _demo([*base, "--engine", engine, "--accumulate_grad_batches", str(A),
                                     "--log_dir", str(tmp_path / f"{engine}{A}")])
        assert res[engine, A]["engine"] == engine and res[engine, A]["accumulate_grad_batches"] == A
        assert res[engine, A]["iters"] == 12
        if engine == "module" and A > 1:
            assert "accumulation window of 3 micro-batches: run eagerly" in out
    torch.testing.assert_close(torch.tensor(res["module", 3]["final_loss"]), torch.tensor(res["stock", 3]["final_loss"]),
                               rtol=1e-5, atol=1e-6)
    assert not torch.allclose(torch.tensor(res["module", 1]["final_loss"]), torch.tensor(res["module", 3]["final_loss"]),
                              rtol=1e-3)


# ------------------------------------------------------------------------------ FlatDDP.no_sync
def _no_sync_rank(rank, world):
    import contextlib
    import copy

    from distributed_training_pytorch_amd.parallel import comm_util
    from distributed_training_pytorch_amd.parallel.ddp import FlatDDP

    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Tanh(), torch.nn.Linear(5, 2))
    ref = torch.nn.parallel.DistributedDataParallel(copy.deepcopy(net))
    ddp = FlatDDP(net, comm="rccl", bucket_cap_mb=1e-6, first_bucket_mb=1e-6)  # one bucket per parameter
    n_buckets = len(ddp._buckets)
    calls = [0]
    orig = comm_util.all_reduce_

    def counting(t, *a, **k):
        calls[0] += 1
        return orig(t, *a, **k)

    comm_util.all_reduce_ = counting
    out = {"buckets": n_buckets, "windows": []}
    A = 3
    g = torch.Generator().manual_seed(100 + rank)
    try:
        for w in range(3):
            if w == 1:  # leaving the context without a backward breaks nothing
                with ddp.no_sync():
                    assert not ddp.graph_safe()
            xs = [torch.randn(4, 3, generator=g) for _ in range(A)]
            ys = [torch.randn(4, 2, generator=g) for _ in range(A)]
            ddp.flat_grad.zero_()
            ref.zero_grad(set_to_none=True)
            calls[0] = 0
            for j in range(A):
                hold = j < A - 1 and w != 2  # window 2: no no_sync, every backward reduces
                with (ddp.no_sync() if hold else contextlib.nullcontext()):
                    (torch.nn.functional.mse_loss(ddp(xs[j]), ys[j]) / A).backward()
                with (ref.no_sync() if j < A - 1 else contextlib.nullcontext()):
                    (torch.nn.functional.mse_loss(ref(xs[j]), ys[j]) / A).backward()
            want = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
            out["windows"].append({"calls": calls[0], "got": ddp.flat_grad.detach().clone(), "want": want.detach().clone()})
    finally:
        comm_util.all_reduce_ = orig
    return out


def test_flat_ddp_no_sync_two_gloo_ranks():
    from .dist_utils import run_ranks

    res = run_ranks(_no_sync_rank, 2, (), timeout=200)
    for r in (0, 1):
        nb = res[r]["buckets"]
        assert nb == 4
        w = res[r]["windows"]
        # one bucket reduction per window instead of A
        assert w[0]["calls"] == nb and w[1]["calls"] == nb and w[2]["calls"] == 3 * nb, [x["calls"] for x in w]
        for k in (0, 1):
            torch.testing.assert_close(w[k]["got"], w[k]["want"], rtol=1e-6, atol=1e-9)
        # (window 2 ran without no_sync: A times the reductions for the same mean, summed in
        # another order -- a few ulps of the largest term where an element's terms cancel)
        torch.testing.assert_close(w[2]["got"], w[2]["want"], rtol=1e-6, atol=8 * 2.0 ** -24 * w[2]["want"].abs().max().item())
    assert torch.equal(res[0]["windows"][0]["got"], res[1]["windows"][0]["got"])

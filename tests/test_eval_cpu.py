"""Held-out evaluation without a GPU: the CPU branch of ops.eval against fp64, ToyData's
held-out sets, the CLI flags, demo.py --eval_every on two gloo ranks, and the Trainer's
validation loop (size-weighted epoch means, uneven rank shards, unchanged rows without it)."""
import csv
import os
import sys

import pytest
import torch

from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.ops import eval as E
from distributed_training_pytorch_amd.ops.mlp import mlp_forward_ref_bf16
from distributed_training_pytorch_amd.runtime import checkpoint

from . import eval_cases as C
from .dist_utils import run_ranks
from .test_launchers_cpu import PY, _run, _run_torchrun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- ops.eval, CPU branch
@pytest.mark.parametrize("loss,spec", [("mse", C.MSE_SPEC), ("ce", C.CE_SPEC)])
@pytest.mark.parametrize("n", [1, 65, 513])
def test_cpu_branch_matches_fp64(loss, spec, n):
    P = C.params(spec)
    X, Y = C.inputs(spec, n, loss)
    got = E.evaluate(P, spec, X, Y, loss=loss)
    assert got.dtype == torch.float64 and got.shape == (3, 2)
    C.assert_matches_fp64(got, P, spec, X, Y, loss)
    res = E.EvalResult(E.evaluate(P[:2], spec, X, Y, loss=loss), n, spec.out_features, loss)
    assert res.count == n and res.mean_loss.dtype == torch.float32 and res.mean_loss.shape == (2,)
    torch.testing.assert_close(res.mean_loss.double(), C.mean_loss(got[:2], n, spec, loss), rtol=1e-6, atol=0)
    if loss == "ce":
        torch.testing.assert_close(res.accuracy.double(), got[:2, 1] / n, rtol=1e-6, atol=0)
    else:
        assert res.accuracy is None


@pytest.mark.parametrize("loss,spec", [("mse", C.MSE_SPEC), ("ce", C.CE_SPEC)])
def test_cpu_shards_add_up_and_empty_shards_are_zero(loss, spec):
    P = C.params(spec)
    for n in (513, 5):
        X, Y = C.inputs(spec, n, loss)
        whole = E.evaluate(P, spec, X, Y, loss=loss)
        for world in (2, 3, 8):
            parts = [E.evaluate(P, spec, X, Y, loss=loss, row0=r, row_stride=world) for r in range(world)]
            for r in range(n, world):
                assert torch.equal(parts[r], torch.zeros(3, 2, dtype=torch.float64))
            # torch's CPU GEMM rounds a row differently in another batch, so the shards' fp32
            # per-sample values are not the whole's bit for bit (the kernel's are: the GPU test
            # holds them to 1e-12): the fp32 loss tolerance here
            torch.testing.assert_close(torch.stack(parts).sum(0), whole, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    with pytest.raises(ValueError):
        E.evaluate(P, spec, X, Y, loss=loss, row0=1, row_stride=2, n=3)  # rows 1, 3 only


def test_cpu_bf16_branch_uses_the_bf16_reference():
    spec, n = C.MSE_SPEC, 257
    P = C.params(spec)
    X, Y = C.inputs(spec, n, "mse")
    got = E.evaluate(P, spec, X, Y, bf16=True)
    want = torch.stack([((mlp_forward_ref_bf16(P[i], spec, X) - Y) ** 2).sum(1).double().sum() for i in range(3)])
    torch.testing.assert_close(got[:, 0] / n, want / n, rtol=C.BF16_RTOL, atol=C.BF16_ATOL)
    assert not torch.equal(got, E.evaluate(P, spec, X, Y))


def test_fused_trainer_evaluate_on_the_cpu_changes_nothing():
    from distributed_training_pytorch_amd.data.sampler import SamplerGeometry
    from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer

    ds = ToyData(n=200, seed=4)
    tr = FusedTrainer(C.MSE_SPEC, 2, ds.X, ds.Y, SamplerGeometry(n=200, world=1, rank=0, batch=64, shuffle=False),
                      cfg=EngineConfig(log_cap=64))
    tr.train(3)
    before = [t.clone() for t in tr._state()] + [torch.tensor(tr.t)]
    res = tr.evaluate()
    after = [t.clone() for t in tr._state()] + [torch.tensor(tr.t)]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert res["count"] == 200 and res["accuracy"] is None and res["loss"].dtype == torch.float32
    want, _ = C.ref_sums(tr.params, C.MSE_SPEC, ds.X, ds.Y, "mse")
    torch.testing.assert_close(res["loss"].double(), want[:, 0] / 200, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    held = ds.held_out(77, 5)
    assert tr.evaluate(held.X, held.Y)["count"] == 77


# ----------------------------------------------------------------------------- ToyData
def _draw(n, seed, in_features=2):
    """ToyData's draw order, written out: n x randn, then one randn(1) per sample."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    y = torch.stack([torch.randn(1, generator=g) * 0.5 + v[i] ** 2 for i in range(n)]).reshape(n, 1)
    return v.unsqueeze(1).repeat(1, in_features), y


def test_toydata_draws_are_unchanged_and_held_out_uses_the_train_edges():
    X, Y = _draw(96, 7)
    ds = ToyData(n=96, seed=7)
    assert torch.equal(ds.X, X) and torch.equal(ds.Y, Y) and ds.edges is None
    dc = ToyData(n=96, seed=7, classes=4)
    edges = torch.quantile(Y.view(-1), torch.linspace(0, 1, 5)[1:-1])
    assert torch.equal(dc.edges, edges) and torch.equal(dc.X, X)
    assert torch.equal(dc.Y, torch.bucketize(Y.view(-1), edges).float().view(96, 1))
    # a new draw of the same distribution, labelled with the TRAIN set's edges
    hx, hy = _draw(50, 8)
    h = dc.held_out(50, 8)
    assert torch.equal(h.X, hx) and torch.equal(h.Y, torch.bucketize(hy.view(-1), edges).float().view(50, 1))
    assert torch.equal(h.edges, edges) and h.classes == 4 and len(h) == 50
    own = ToyData(n=50, seed=8, classes=4)
    assert not torch.equal(own.edges, edges) and not torch.equal(own.Y, h.Y)  # its own quantiles differ
    again = dc.held_out(50, 8)
    assert torch.equal(again.X, h.X) and torch.equal(again.Y, h.Y)
    hr = ds.held_out(50, 8)
    assert torch.equal(hr.Y, hy) and hr.edges is None


# ----------------------------------------------------------------------------- CLI
def test_parsers_default_to_no_evaluation():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import argument_parser
    import demo_one_model_multi_gpu
    import demo_pytorch_lightning

    a = argument_parser.get_args([])
    assert a.eval_every == 0 and a.val_samples == 512
    a = argument_parser.get_args(["--eval_every", "50", "--val_samples", "300"])
    assert a.eval_every == 50 and a.val_samples == 300
    b = demo_pytorch_lightning.get_args([])
    assert b.val_samples == 0 and b.check_val_every_n_epoch == 1
    # the layer-split demo refuses the flag before it touches a device or a process group
    with pytest.raises(SystemExit, match="eval_every"):
        demo_one_model_multi_gpu.main(["--eval_every", "5", "--device", "cpu", "--backend", "gloo"])


# ----------------------------------------------------------------------------- demo.py
DEMO = ["--backend", "gloo", "--device", "cpu", "--iters", "20", "--log_every", "5", "--no_progress", "--seed", "11",
        "--eval_every", "8", "--val_samples", "131"]


def _val_rows(log_dir):
    return [r for r in C.read_metrics(log_dir) if "val/lossX" in r]


def _loss_rows(log_dir):
    return [r for r in C.read_metrics(log_dir) if "loss/lossX" in r]


def test_demo_fused_two_gloo_ranks_log_the_full_sets_validation_loss(tmp_path):
    """Two ranks evaluate rows r::2 of the 131-row held-out set (66 + 65, no padding): the
    val/* rows sit after iterations 8, 16 and 20, the last one is the one-process fp64
    evaluation of the checkpointed weights on the whole regenerated set, and the loss/*
    rows are those of the run without --eval_every."""
    args = ["--nproc-per-node", "2", "demo.py", "--torchrun", *DEMO, "--engine", "fused", "--check_replicas"]
    r = _run_torchrun([*args, "--log_dir", str(tmp_path / "a"), "--checkpoint_dir", str(tmp_path / "ck")])
    assert r.returncode == 0, r.stderr[-3000:]
    rows = _val_rows(tmp_path / "a")
    assert [x["step"] for x in rows] == [8, 16, 20] and all("val/accX" not in x for x in rows)
    st = checkpoint.load(str(tmp_path / "ck"))
    _, held = C.held_out_sets(11, 512, 131, 0)
    want, _ = C.ref_sums(st["params"], C.MSE_SPEC, held.X, held.Y, "mse")
    got = torch.tensor([rows[-1]["val/lossX"], rows[-1]["val/lossY"]], dtype=torch.float64)
    torch.testing.assert_close(got, want[:, 0] / 131, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    assert f"'val_loss': [{rows[-1]['val/lossX']!r}, {rows[-1]['val/lossY']!r}]" in r.stdout
    off = _run_torchrun(["--nproc-per-node", "2", "demo.py", "--torchrun", *DEMO[:-4], "--engine", "fused",
                         "--log_dir", str(tmp_path / "b")])
    assert off.returncode == 0, off.stderr[-3000:]
    assert not _val_rows(tmp_path / "b") and "val_loss" not in off.stdout
    assert _loss_rows(tmp_path / "a") == _loss_rows(tmp_path / "b") and len(_loss_rows(tmp_path / "b")) == 20


def test_demo_stock_two_gloo_ranks_log_the_full_sets_validation_loss(tmp_path):
    """The stock engine on two ranks (rows r::2, 66 + 65): the last val/* row is the
    one-process fp64 evaluation of the weights it wrote to --checkpoint_dir on the whole
    regenerated set."""
    r = _run_torchrun(["--nproc-per-node", "2", "demo.py", "--torchrun", *DEMO, "--engine", "stock",
                       "--log_dir", str(tmp_path / "a"), "--checkpoint_dir", str(tmp_path / "ck")])
    assert r.returncode == 0, r.stderr[-3000:]
    rows = _val_rows(tmp_path / "a")
    assert [x["step"] for x in rows] == [8, 16, 20]
    st = checkpoint.load(str(tmp_path / "ck"))
    assert st["engine"] == "stock" and st["params"].shape == (2, C.MSE_SPEC.P)
    _, held = C.held_out_sets(11, 512, 131, 0)
    want, _ = C.ref_sums(st["params"], C.MSE_SPEC, held.X, held.Y, "mse")
    got = torch.tensor([rows[-1]["val/lossX"], rows[-1]["val/lossY"]], dtype=torch.float64)
    torch.testing.assert_close(got, want[:, 0] / 131, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    assert f"'val_loss': [{rows[-1]['val/lossX']!r}, {rows[-1]['val/lossY']!r}]" in r.stdout
    assert [x["step"] for x in _loss_rows(tmp_path / "a")] == list(range(20))


def _runner_validation_shards(rank, world):
    """The runner's torch path (stock engine, wide models): this rank's shard and the one
    all-reduce, against the whole set in one process."""
    import argparse

    from distributed_training_pytorch_amd.engine.runner import _Validation
    from distributed_training_pytorch_amd.utils.logging import MetricLogger

    out = {}
    for loss, spec in (("mse", C.MSE_SPEC), ("ce", C.CE_SPEC)):
        cfg = argparse.Namespace(eval_every=3, val_samples=131, iters=7, loss=loss, per_rank_data=True, n_samples=64,
                                 seed=5)
        train = ToyData(n=64, seed=5, rank=rank, per_rank=True, classes=4 if loss == "ce" else 0)
        val = _Validation(cfg, train, rank, world, torch.device("cpu"), MetricLogger(rank=1))
        P = C.params(spec)[:2]
        from distributed_training_pytorch_amd.ops.mlp import mlp_forward_ref

        sums, n = val.sums_torch(lambda x: [mlp_forward_ref(P[i], spec, x) for i in range(2)])
        res = val.reduce(sums, n, spec.out_features)
        out[loss] = (res["loss"], res["accuracy"], res["count"], n, val.X, val.Y,
                     [val.due(i) for i in range(8)], val.to_next(4))
    return out


def test_runner_validation_shards_reduce_to_the_whole_set():
    res = run_ranks(_runner_validation_shards, 2)
    for loss, spec in (("mse", C.MSE_SPEC), ("ce", C.CE_SPEC)):
        l0, a0, c0, n0, X0, Y0, due, nxt = res[0][loss]
        l1, a1, c1, n1, X1, Y1, _, _ = res[1][loss]
        assert (n0, n1, c0, c1) == (66, 65, 131, 131)
        # the same held-out rows and labels on both ranks although each drew its own training set
        assert torch.equal(X0, X1) and torch.equal(Y0, Y1) and torch.equal(l0, l1)
        _, held = C.held_out_sets(5, 64, 131, 4 if loss == "ce" else 0)
        assert torch.equal(X0, held.X) and torch.equal(Y0, held.Y)
        want, _ = C.ref_sums(C.params(spec)[:2], spec, held.X, held.Y, loss)
        torch.testing.assert_close(l0.double(), want[:, 0] / 131, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
        if loss == "ce":
            assert torch.equal(a0, a1)
            torch.testing.assert_close(a0.double(), want[:, 1] / 131, rtol=1e-6, atol=0)
        else:
            assert a0 is None
        assert due == [False, False, False, True, False, False, True, True] and nxt == 2


# ----------------------------------------------------------------------------- Trainer
def _lit():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from demo_pytorch_lightning import LitToyModel

    return LitToyModel()


def _csv_rows(tr):
    with open(tr._log_dir / "metrics.csv", newline="") as f:
        return list(csv.DictReader(f))


def _manual_val(model, X, Y):
    with torch.no_grad():
        return {"val_loss_X": float(((model.model_X(X) - Y).double() ** 2).mean()),
                "val_loss_Y": float(((model.model_Y(X) - Y).double() ** 2).mean())}


def test_trainer_validation_epoch_mean_is_weighted_by_batch_size(tmp_path):
    from distributed_training_pytorch_amd.trainer import Trainer

    torch.manual_seed(0)
    train = ToyData(seed=0)
    held = train.held_out(130, 1)  # batches of 64, 64 and 2
    dl = torch.utils.data.DataLoader(train, batch_size=128)
    vdl = torch.utils.data.DataLoader(held, batch_size=64)
    model = _lit()
    hooks = []
    model.on_validation_epoch_start = lambda: hooks.append(("start", model.training))
    model.on_validation_epoch_end = lambda: hooks.append(("end", model.training))
    tr = Trainer(max_epochs=2, accelerator="cpu", log_every_n_steps=1, default_root_dir=str(tmp_path),
                 enable_progress_bar=False, enable_checkpointing=False)
    tr.fit(model, dl, val_dataloaders=vdl)
    assert tr.global_step == 8 and model.training
    assert hooks == [("start", False), ("end", True)] * 2
    want = _manual_val(model, held.X, held.Y)
    for k, v in want.items():
        assert tr.callback_metrics[k] == pytest.approx(v, rel=1e-5, abs=1e-6)
    # not the mean of the three batch means: the 2-row batch would weigh a third
    with torch.no_grad():
        bm = [float(((model.model_X(held.X[a:b]) - held.Y[a:b]) ** 2).mean()) for a, b in ((0, 64), (64, 128), (128, 130))]
    assert abs(sum(bm) / 3 - want["val_loss_X"]) > 1e-3 * want["val_loss_X"]
    rows = _csv_rows(tr)
    vrows = [r for r in rows if r.get("val_loss_X")]
    assert [int(r["step"]) for r in vrows] == [4, 8]
    assert float(vrows[-1]["val_loss_X"]) == pytest.approx(want["val_loss_X"], rel=1e-5, abs=1e-6)
    assert "loss/lossX" in tr.callback_metrics and "val_loss_X" not in model._logged
    assert len([r for r in rows if r.get("loss/lossX")]) == 8
    got = tr.validate(model, vdl)
    assert isinstance(got, list) and len(got) == 1
    for k, v in want.items():
        assert got[0][k] == pytest.approx(v, rel=1e-5, abs=1e-6)
    # every 2 batches instead of at the epoch ends; every second epoch only
    tr2 = Trainer(max_epochs=2, accelerator="cpu", log_every_n_steps=1, default_root_dir=str(tmp_path / "b"),
                  enable_progress_bar=False, enable_checkpointing=False, val_check_interval=2,
                  check_val_every_n_epoch=2)
    tr2.fit(_lit(), dl, val_dataloaders=vdl)
    assert [int(r["step"]) for r in _csv_rows(tr2) if r.get("val_loss_X")] == [6, 8]
    with pytest.raises(TypeError):
        tr2.fit(_lit(), dl, None, None, vdl)  # keyword only


def test_trainer_without_validation_writes_the_same_rows(tmp_path):
    from distributed_training_pytorch_amd.trainer import LightningModule, Trainer

    def fit(root, **kw):
        torch.manual_seed(0)
        tr = Trainer(max_steps=6, accelerator="cpu", log_every_n_steps=1, default_root_dir=str(tmp_path / root),
                     enable_progress_bar=False, enable_checkpointing=False)
        tr.fit(_lit(), torch.utils.data.DataLoader(ToyData(seed=0), batch_size=128), **kw)
        with open(tr._log_dir / "metrics.csv", newline="") as f:
            return f.read(), tr

    plain, tr = fit("a")
    none, _ = fit("b", val_dataloaders=None)
    assert plain == none and "val_loss" not in plain and plain.count("\n") == 7
    assert all(not k.startswith("val") for k in tr.callback_metrics)
    with_val, _ = fit("c", val_dataloaders=torch.utils.data.DataLoader(ToyData(seed=0).held_out(130, 1), batch_size=64))
    trn = [[r[k] for k in ("step", "loss/lossX", "loss/lossY")] for r in csv.DictReader(with_val.splitlines())
           if r["loss/lossX"]]
    assert trn == [[r[k] for k in ("step", "loss/lossX", "loss/lossY")] for r in csv.DictReader(plain.splitlines())]
    # a module that does not override validation_step is never validated
    class NoVal(type(_lit())):
        validation_step = LightningModule.validation_step

    vdl = torch.utils.data.DataLoader(ToyData(seed=0).held_out(130, 1), batch_size=64)
    torch.manual_seed(0)
    tr = Trainer(max_steps=6, accelerator="cpu", log_every_n_steps=1, default_root_dir=str(tmp_path / "d"),
                 enable_progress_bar=False, enable_checkpointing=False)
    tr.fit(NoVal(), torch.utils.data.DataLoader(ToyData(seed=0), batch_size=128), val_dataloaders=vdl)
    with open(tr._log_dir / "metrics.csv", newline="") as f:
        assert f.read() == plain
    with pytest.raises(RuntimeError, match="validation_step"):
        tr.validate(NoVal(), vdl)


def _trainer_two_ranks(rank, world, root):
    from distributed_training_pytorch_amd.trainer import Trainer

    torch.manual_seed(0)
    train = ToyData(seed=0)
    held = train.held_out(131, 1)  # rows r::2: 66 and 65
    dl = torch.utils.data.DataLoader(train, batch_size=128)
    model = _lit()
    tr = Trainer(gpus=0, max_epochs=1, accelerator="cpu", log_every_n_steps=1, default_root_dir=root,
                 enable_progress_bar=False, enable_checkpointing=False, strategy="ddp")
    # a plain dataset: the strided Subset path; the ToyData itself: device slices
    plain = torch.utils.data.TensorDataset(held.X, held.Y)
    tr.fit(model, dl, val_dataloaders=torch.utils.data.DataLoader(plain, batch_size=64))
    a = dict(tr.callback_metrics)
    b = tr.validate(model, torch.utils.data.DataLoader(held, batch_size=64))[0]
    return a, b, _manual_val(model, held.X, held.Y)


def test_trainer_validation_two_gloo_ranks_uneven_shards(tmp_path):
    res = run_ranks(_trainer_two_ranks, 2, args=(str(tmp_path),))
    a0, b0, want0 = res[0]
    a1, b1, want1 = res[1]
    assert want0 == want1  # DDP: the replicas agree
    for k, v in want0.items():
        assert a0[k] == a1[k] and b0[k] == b1[k]
        assert a0[k] == pytest.approx(v, rel=1e-5, abs=1e-6)
        assert b0[k] == pytest.approx(v, rel=1e-5, abs=1e-6)


def test_demo_lightning_val_samples_flag(tmp_path):
    r = _run([PY, "demo_pytorch_lightning.py", "--accelerator", "cpu", "--steps", "8", "--no_progress",
              "--root_dir", str(tmp_path), "--val_samples", "130", "--batch_size", "128"], timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "'val_loss_X'" in r.stdout and "'val_loss_Y'" in r.stdout

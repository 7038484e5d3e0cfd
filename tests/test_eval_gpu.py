"""Held-out evaluation on the MI355X: the evaluation kernel (csrc/eval.hip) against fp64 at
every size where it changes path, its bounds, shards, bitwise reproducibility (eager and
hipGraph replay), FusedTrainer.evaluate, two ranks sharing the GPU, demo.py --eval_every on
the three engines and the Trainer's validation on the module and fused paths."""
import csv
import functools
import os
import sys

import pytest
import torch

from distributed_training_pytorch_amd import _native as nat
from distributed_training_pytorch_amd.data.sampler import SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops import eval as E
from distributed_training_pytorch_amd.ops.mlp import MlpSpec, mlp_forward_ref_bf16
from distributed_training_pytorch_amd.ops.optim import OptimConfig
from distributed_training_pytorch_amd.runtime import checkpoint

from . import eval_cases as C
from .dist_utils import run_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)


def _T() -> int:
    return int(nat.load().dtp_mlp_eval_one_launch_rows())


def _other_spec() -> MlpSpec:
    """Another width or depth the library has whole-model kernels for."""
    lib = nat.load()
    for key in ((2, 15, 5, 1), (2, 10, 3, 1)):
        if lib.dtp_mlp_supported(*key, 0):
            return MlpSpec(*key)
    raise AssertionError("dtp_mlp_supported knows no second whole-model shape")


@functools.lru_cache(maxsize=None)
def _case(which: str, n: int):
    """(spec, loss, P, X, Y) on the CPU, shared by the tests that use the same case."""
    spec, loss = {"mse": (C.MSE_SPEC, "mse"), "ce": (C.CE_SPEC, "ce")}.get(which) or (_other_spec(), "mse")
    X, Y = C.inputs(spec, n, loss)
    return spec, loss, C.params(spec), X, Y


def _gpu(*ts):
    return [t.to(DEV).contiguous() for t in ts]


# ----------------------------------------------------------------------------- 1. sizes
@pytest.mark.parametrize("n_models", [1, 2, 3])
@pytest.mark.parametrize("which", ["mse", "ce", "other"])
def test_sizes_against_fp64(which, n_models):
    T = _T()
    assert T >= 4096
    lib = nat.load()
    for n in (1, 63, 64, 65, 255, 256, 257, 511, 513, T - 1, T, T + 1, T + 257):
        spec, loss, P, X, Y = _case(which, n)
        P = P[:n_models]
        wsb = int(lib.dtp_mlp_eval_ws_bytes(n, n_models))
        assert (wsb == 0) if n <= T else (wsb > 0), (n, wsb)
        got = E.evaluate(*_gpu(P), spec, *_gpu(X, Y), loss=loss)
        assert got.shape == (n_models, 2) and got.dtype == torch.float64 and got.is_cuda
        C.assert_matches_fp64(got, P, spec, X, Y, loss)


def test_bf16_instances_use_the_bf16_forward():
    for which in ("mse", "ce"):
        spec, loss, P, X, Y = _case(which, 513)
        got = E.evaluate(*_gpu(P), spec, *_gpu(X, Y), loss=loss, bf16=True).cpu()
        fp32 = E.evaluate(*_gpu(P), spec, *_gpu(X, Y), loss=loss).cpu()
        assert not torch.equal(got[:, 0], fp32[:, 0])
        want = E.evaluate(P, spec, X, Y, loss=loss, bf16=True)  # the CPU branch: mlp_forward_ref_bf16
        torch.testing.assert_close(C.mean_loss(got, 513, spec, loss), C.mean_loss(want, 513, spec, loss),
                                   rtol=C.BF16_RTOL, atol=C.BF16_ATOL)
        o = mlp_forward_ref_bf16(P[0], spec, X)
        assert o.shape == (513, spec.out_features)
    with pytest.raises(NotImplementedError):
        spec = _other_spec()
        E.evaluate(torch.zeros(1, spec.P, device=DEV), spec, torch.zeros(4, 2, device=DEV), torch.zeros(4, 1, device=DEV),
                   bf16=True)


def test_bad_arguments_are_errors():
    spec, loss, P, X, Y = _case("mse", 65)
    Pg, Xg, Yg = _gpu(P, X, Y)
    with pytest.raises(ValueError):
        E.evaluate(Pg, spec, Xg, Yg, row0=-1)
    with pytest.raises(ValueError):
        E.evaluate(Pg, spec, Xg, Yg, n=66)
    with pytest.raises(ValueError):
        E.evaluate(Pg, spec, Xg, Yg[:64])
    with pytest.raises(NotImplementedError):
        wide = MlpSpec(2, 64, 5, 1)
        E.evaluate(torch.zeros(1, wide.P, device=DEV), wide, Xg, Yg)
    lib = nat.load()
    out = torch.zeros(3, 2, dtype=torch.float64, device=DEV)
    a = nat.EvalArgs(nat.ptr(Xg), nat.ptr(Yg), nat.ptr(Pg), nat.ptr(out), None, 0, 0, 65, 3, nat.LOSS_MSE, 0, 0.01)
    import ctypes

    assert lib.dtp_mlp_eval(ctypes.byref(a), *spec.key[:4], nat.stream_ptr()) == -1  # row_stride 0
    assert b"row_stride" in lib.dtp_last_error()
    a = nat.EvalArgs(nat.ptr(Xg), nat.ptr(Yg), nat.ptr(Pg), nat.ptr(out), None, 0, 1, _T() + 1, 3, nat.LOSS_MSE, 0, 0.01)
    assert lib.dtp_mlp_eval(ctypes.byref(a), *spec.key[:4], nat.stream_ptr()) != 0  # workspace missing: nothing launched


# ----------------------------------------------------------------------------- 2. bounds
@pytest.mark.parametrize("which", ["mse", "ce"])
def test_reads_and_writes_stay_inside_their_rows(which):
    T = _T()
    for n, row0, stride in ((1, 0, 1), (513, 0, 1), (513, 2, 3), (T + 257, 0, 1), (T + 257, 1, 2)):
        spec, loss, P, X, Y = _case(which, n)
        pad = 64
        xb = torch.full((pad + n + pad, spec.in_features), float("nan"))
        xb[pad:pad + n] = X
        yb = torch.full((pad + n + pad, Y.shape[1]), float("nan"))
        yb[pad:pad + n] = Y
        pb = torch.full((P.numel() + 2 * pad,), float("nan"))
        pb[pad:pad + P.numel()] = P.reshape(-1)
        xg, yg, pg = _gpu(xb, yb, pb)
        k = E.shard_rows(n, row0, stride)
        wsn = int(nat.load().dtp_mlp_eval_ws_bytes(k, 3)) // 8
        ob = torch.full((8 + 6 + 8,), -7.0, dtype=torch.float64, device=DEV)
        wb = torch.full((8 + wsn + 8,), -7.0, dtype=torch.float64, device=DEV)
        got = E.evaluate(pg[pad:pad + P.numel()].view(3, -1), spec, xg[pad:pad + n], yg[pad:pad + n], loss=loss,
                         row0=row0, row_stride=stride, out=ob[8:14].view(3, 2), ws=wb[8:8 + wsn] if wsn else None)
        assert got.data_ptr() == ob[8:].data_ptr()
        assert torch.isfinite(got).all(), (n, row0, stride, got)
        assert (ob[:8] == -7).all() and (ob[14:] == -7).all() and (wb[:8] == -7).all() and (wb[8 + wsn:] == -7).all()
        if wsn:
            assert torch.isfinite(wb[8:8 + wsn]).all() and (wb[8:8 + wsn] != -7).any()
        C.assert_matches_fp64(got, P, spec, X[row0::stride], Y[row0::stride], loss)


# ----------------------------------------------------------------------------- 3. shards
@pytest.mark.parametrize("which", ["mse", "ce"])
def test_shard_sums_add_to_the_whole(which):
    for n in (513, 5):
        spec, loss, P, X, Y = _case(which, n)
        Pg, Xg, Yg = _gpu(P, X, Y)
        whole = E.evaluate(Pg, spec, Xg, Yg, loss=loss).cpu()
        for world in (2, 3, 8):
            parts = [E.evaluate(Pg, spec, Xg, Yg, loss=loss, row0=r, row_stride=world).cpu() for r in range(world)]
            for r in range(n, world):  # a rank with no rows
                assert torch.equal(parts[r], torch.zeros(3, 2, dtype=torch.float64))
            torch.testing.assert_close(torch.stack(parts).sum(0), whole, rtol=C.SHARD_RTOL, atol=0)
            assert torch.equal(torch.stack(parts).sum(0)[:, 1], whole[:, 1])


# ----------------------------------------------------------------------------- 4. reproducibility
@pytest.mark.parametrize("which", ["mse", "ce"])
def test_bitwise_reproducible_eager_and_graph_replay(which):
    T = _T()
    for n in (513, T + 257):
        spec, loss, P, X, Y = _case(which, n)
        Pg, Xg, Yg = _gpu(P, X, Y)
        a = E.evaluate(Pg, spec, Xg, Yg, loss=loss).clone()
        b = E.evaluate(Pg, spec, Xg, Yg, loss=loss).clone()
        assert torch.equal(a, b)
        out = torch.zeros(3, 2, dtype=torch.float64, device=DEV)
        ws = E.eval_ws(n, 3, DEV)
        assert (ws is None) == (n <= T)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            E.evaluate(Pg, spec, Xg, Yg, loss=loss, out=out, ws=ws)
        for _ in range(2):
            out.fill_(-1.0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


# ----------------------------------------------------------------------------- 5. FusedTrainer.evaluate
def _trainer(loss, launch="persistent", seed=5, spl=5):
    ds = ToyData(n=200, seed=2, classes=4 if loss == "ce" else 0)
    X, Y = ds.device_tensors(DEV)
    spec = C.CE_SPEC if loss == "ce" else C.MSE_SPEC
    torch.manual_seed(seed)
    init = [torch.randn(spec.P) * 0.4 for _ in range(2)]
    geom = SamplerGeometry(n=200, world=1, rank=0, batch=64, shuffle=False)
    tr = FusedTrainer(spec, 2, X, Y, geom, OptimConfig(lr=1e-2),
                      EngineConfig(launch=launch, steps_per_launch=spl, loss=loss, log_cap=64), init_params=init)
    return tr, ds, spec


def _check_against_fp64(res, params, spec, X, Y, loss):
    n = X.shape[0]
    want, _ = C.ref_sums(params.cpu(), spec, X.cpu(), Y.cpu(), loss)
    assert res["count"] == n and res["loss"].dtype == torch.float32 and res["loss"].shape == (2,)
    torch.testing.assert_close(res["loss"].double(), C.mean_loss(want, n, spec, loss), rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    if loss == "ce":
        # trained weights: a row whose fp64 top-2 margin is below MIN_MARGIN may go either way in fp32
        from distributed_training_pytorch_amd.ops.mlp import mlp_forward_ref

        close = 0
        for i in range(2):
            top = mlp_forward_ref(params[i].cpu().double(), spec, X.cpu().double()).topk(2, dim=1).values
            close = max(close, int(((top[:, 0] - top[:, 1]) < C.MIN_MARGIN).sum()))
        assert close <= 2, f"{close} rows with a top-2 margin below {C.MIN_MARGIN}: the accuracy check would be vacuous"
        assert res["accuracy"].dtype == torch.float32
        assert ((res["accuracy"].double() * n - want[:, 1]).abs() <= close + 1e-3).all(), (res["accuracy"], want[:, 1], close)
    else:
        assert res["accuracy"] is None


@pytest.mark.parametrize("loss", ["mse", "ce"])
def test_fused_trainer_evaluate_reads_the_weights_and_changes_nothing(loss):
    tr, ds, spec = _trainer(loss)
    tr.train(7)
    state = [tr.params, tr.m, tr.v, tr.step_ctr, tr.loss_log, tr.comm_buf]
    if tr._ring is not None:
        state.append(tr._ring.table)
    before = [t.clone() for t in state]
    t_before = tr.t
    res = tr.evaluate()
    assert tr.t == t_before == 7 and all(torch.equal(a, b) for a, b in zip(before, state))
    _check_against_fp64(res, tr.params, spec, tr.X, tr.Y, loss)
    held = ds.held_out(77, 9)
    hx, hy = held.device_tensors(DEV)
    _check_against_fp64(tr.evaluate(hx, hy), tr.params, spec, hx, hy, loss)
    # step t's batch: the evaluation's mean loss is the train kernel's own loss of that batch
    idx = torch.as_tensor(tr.step_indices(tr.t), dtype=torch.long, device=DEV)
    _, step_loss = tr.local_gradients()
    got = tr.evaluate(tr.X[idx], tr.Y[idx])
    assert got["count"] == idx.numel()
    torch.testing.assert_close(got["loss"], step_loss.cpu(), rtol=1e-5, atol=0)
    tr.close()


@pytest.mark.parametrize("loss", ["mse", "ce"])
@pytest.mark.parametrize("launch", ["persistent", "eager", "graph"])
def test_evaluate_between_launches_leaves_training_bitwise(launch, loss):
    a, _, _ = _trainer(loss, launch)
    a.train(10)
    b, _, _ = _trainer(loss, launch)
    b.train(5)
    mid = b.evaluate()
    b.train(5)
    a.synchronize()
    b.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert torch.equal(a.losses(0, 10), b.losses(0, 10)) and a.t == b.t == 10
    assert torch.isfinite(mid["loss"]).all()
    a.close()
    b.close()


# ----------------------------------------------------------------------------- 6. two ranks, one GPU
def _two_rank_eval(rank, world, loss):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ds = ToyData(n=512, seed=1, classes=4 if loss == "ce" else 0)
    X, Y = ds.device_tensors(dev)
    spec = C.CE_SPEC if loss == "ce" else C.MSE_SPEC
    geom = SamplerGeometry(n=512, world=world, rank=rank, batch=128, seed=3)
    torch.manual_seed(100)
    init = [torch.randn(spec.P) * 0.4 for _ in range(2)]
    tr = FusedTrainer(spec, 2, X, Y, geom, OptimConfig(lr=1e-2), EngineConfig(steps_per_launch=4, loss=loss),
                      init_params=init)
    tr.train(4)
    held = ds.held_out(513, 2)
    hx, hy = held.device_tensors(dev)
    res = tr.evaluate(hx, hy)
    whole = E.evaluate(tr.params, spec, hx, hy, loss=loss).cpu()  # one process, every row
    mine = E.evaluate(tr.params, spec, hx, hy, loss=loss, row0=rank, row_stride=world).cpu()
    tr.synchronize()
    out = (res["loss"], res["accuracy"], res["count"], whole, mine, tr.params.cpu())
    tr.close()
    return out


@pytest.mark.parametrize("loss", ["mse", "ce"])
def test_two_ranks_return_the_same_dict_as_one_process(loss):
    res = run_ranks(_two_rank_eval, 2, (loss,), timeout=300)
    l0, a0, c0, whole0, mine0, p0 = res[0]
    l1, a1, c1, whole1, mine1, p1 = res[1]
    assert torch.equal(p0, p1), "replicas diverged"
    assert torch.equal(l0, l1) and c0 == c1 == 513 and torch.equal(whole0, whole1)
    spec = C.CE_SPEC if loss == "ce" else C.MSE_SPEC
    torch.testing.assert_close(mine0 + mine1, whole0, rtol=C.SHARD_RTOL, atol=0)
    want = E.EvalResult(mine0 + mine1, 513, spec.out_features, loss)
    assert torch.equal(l0, want.mean_loss)
    if loss == "ce":
        assert torch.equal(a0, a1) and torch.equal(a0, want.accuracy)
    else:
        assert a0 is None and a1 is None


# ----------------------------------------------------------------------------- 7. demo.py
def _demo(argv):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import demo

    saved = {k: os.environ.get(k) for k in ("WANDB_MODE", "MASTER_ADDR", "MASTER_PORT")}
    os.environ["WANDB_MODE"] = "disabled"
    try:
        return demo.main(["--no_progress", "--seed", "3", *argv])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_demo_case(tmp_path, engine, loss):
    """demo.py --iters 120 --eval_every 50 --val_samples 300 against the same run without
    --eval_every."""
    base = ["--iters", "120", "--engine", engine, "--loss", loss]
    s = _demo([*base, "--eval_every", "50", "--val_samples", "300", "--log_dir", str(tmp_path / "a"),
               "--checkpoint_dir", str(tmp_path / "ck")])
    rows = C.read_metrics(tmp_path / "a")
    val = [r for r in rows if "val/lossX" in r]
    assert [r["step"] for r in val] == [50, 100, 120]
    assert s["val_loss"] == [val[-1]["val/lossX"], val[-1]["val/lossY"]] and s["engine"] == engine
    ce = loss == "ce" and engine != "stock"  # the stock loop trains one-output MSE models whatever --loss says
    spec = C.CE_SPEC if ce else C.MSE_SPEC
    st = checkpoint.load(str(tmp_path / "ck"))
    train, held = C.held_out_sets(3, 512, 300, 4 if loss == "ce" else 0)
    want, _ = C.ref_sums(st["params"].float(), spec, held.X, held.Y, "ce" if ce else "mse")
    torch.testing.assert_close(torch.tensor(s["val_loss"], dtype=torch.float64), C.mean_loss(want, 300, spec, "ce" if ce else "mse"),
                               rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    if ce:
        assert all("val/accX" in r and "val/accY" in r for r in val)
        assert s["val_acc"] == [val[-1]["val/accX"], val[-1]["val/accY"]] and all(0 <= a <= 1 for a in s["val_acc"])
    else:
        assert all("val/accX" not in r for r in val) and "val_acc" not in s
    off = _demo([*base, "--log_dir", str(tmp_path / "b")])
    assert "val_loss" not in off
    plain = C.read_metrics(tmp_path / "b")
    assert all("val/lossX" not in r for r in plain)
    # the loss/* rows, in file order (step order), bit for bit those of the run without the flag
    got = [r for r in rows if "loss/lossX" in r or "loss/lossY" in r]
    assert got == plain and sorted({r["step"] for r in got}) == list(range(120))
    assert [r["step"] for r in rows] == sorted(r["step"] for r in rows)


@pytest.mark.parametrize("engine,loss", [("fused", "mse"), ("module", "mse"), ("stock", "mse"), ("fused", "ce"),
                                         ("module", "ce")])
def test_demo_eval_every(tmp_path, engine, loss):
    run_demo_case(tmp_path, engine, loss)


# ----------------------------------------------------------------------------- 8. Trainer
def _lit(cls_name="honest"):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from demo_pytorch_lightning import LitToyModel

    if cls_name == "honest":
        return LitToyModel()

    class SwappedVal(LitToyModel):
        """Declares val_loss_X = MSE(model_X) but logs model Y's loss under that name."""

        def validation_step(self, batch, batch_idx):
            x, y = batch
            ox, oy = self(x)
            self.log("val_loss_X", self.loss(oy, y))
            self.log("val_loss_Y", self.loss(ox, y))

    return SwappedVal()


def _manual_val(model, X, Y):
    with torch.no_grad():
        px, py = model.model_X.flat_params.detach().cpu().double(), model.model_Y.flat_params.detach().cpu().double()
        from distributed_training_pytorch_amd.ops.mlp import mlp_forward_ref

        return {"val_loss_X": float(((mlp_forward_ref(px, C.MSE_SPEC, X.double()) - Y.double()) ** 2).mean()),
                "val_loss_Y": float(((mlp_forward_ref(py, C.MSE_SPEC, X.double()) - Y.double()) ** 2).mean())}


def _fit_val(tmp_path, engine, model):
    from distributed_training_pytorch_amd.trainer import Trainer

    torch.manual_seed(0)
    train = ToyData(seed=0)
    held = train.held_out(130, 1)
    dl = torch.utils.data.DataLoader(train, batch_size=128)
    vdl = torch.utils.data.DataLoader(held, batch_size=64)
    tr = Trainer(gpus=1, max_epochs=2, accelerator="gpu", log_every_n_steps=1, default_root_dir=str(tmp_path),
                 enable_progress_bar=False, enable_checkpointing=False, engine=engine)
    tr.fit(model, dl, val_dataloaders=vdl)
    with open(tr._log_dir / "metrics.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    return tr, held, vdl, rows


@pytest.mark.parametrize("engine", ["module", "fused"])
def test_trainer_validation_rows_and_values(tmp_path, engine):
    model = _lit()
    tr, held, vdl, rows = _fit_val(tmp_path, engine, model)
    assert tr.engine_used == engine and tr.global_step == 8 and tr.val_fused_refused is None
    vrows = [r for r in rows if r.get("val_loss_X")]
    assert [int(r["step"]) for r in vrows] == [4, 8]
    assert len([r for r in rows if r.get("loss/lossX")]) == 8
    want = _manual_val(model, held.X, held.Y)
    got = tr.validate(model, vdl)
    assert isinstance(got, list) and len(got) == 1
    for k, v in want.items():
        assert tr.callback_metrics[k] == pytest.approx(v, rel=C.LOSS_RTOL, abs=C.LOSS_ATOL)
        assert float(vrows[-1][k]) == pytest.approx(v, rel=C.LOSS_RTOL, abs=C.LOSS_ATOL)
        assert got[0][k] == pytest.approx(v, rel=C.LOSS_RTOL, abs=C.LOSS_ATOL)
    assert "loss/lossX" in tr.callback_metrics and model.training


def test_trainer_misdeclared_val_metrics_fall_back(tmp_path):
    model = _lit("swapped")
    tr, held, vdl, rows = _fit_val(tmp_path, "fused", model)
    assert tr.engine_used == "fused" and tr.val_fused_refused and "val_loss_" in tr.val_fused_refused
    want = _manual_val(model, held.X, held.Y)
    # the general loop's values: what validation_step logs, not what fused_spec declares
    assert tr.callback_metrics["val_loss_X"] == pytest.approx(want["val_loss_Y"], rel=C.LOSS_RTOL, abs=C.LOSS_ATOL)
    assert tr.callback_metrics["val_loss_Y"] == pytest.approx(want["val_loss_X"], rel=C.LOSS_RTOL, abs=C.LOSS_ATOL)
    assert [int(r["step"]) for r in rows if r.get("val_loss_X")] == [4, 8]

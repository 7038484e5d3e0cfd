"""Gradient clipping by norm and value inside the fused step kernels (GPU only): the clip twins of
``csrc/mlp_train_one.hip`` and ``csrc/mlp_train_lanes.hip`` (``csrc/clip_core.h``).

* the read-out protocol of ``tests/clip_step_cases.py`` over one cell per twin: the clipped
  gradient the optimizer took is the plain engine's times torch's coefficient, bit for bit;
* trajectories against a clipped fp64 loop (``clip_grad_norm_`` / ``clip_grad_value_`` per model
  between backward and ``opt.step()``) at the step count and tolerances of
  ``tests/test_lanes_gpu.py``;
* persistent, eager and graph launches bitwise equal under clipping;
* the C API's refusals, the forced 8-wave picks, ``demo.py --engine fused --clip_grad_norm``;
* several ranks on one GPU: the xGMI twins, and the xGMI self-test passing under clipping.
"""
import ctypes
import os
import subprocess
import sys
from dataclasses import replace

import pytest
import torch

from distributed_training_pytorch_amd import _native as nat
from distributed_training_pytorch_amd.data.sampler import EpochIndexStream
from distributed_training_pytorch_amd.ops.mlp import mlp_forward_ref
from distributed_training_pytorch_amd.ops.optim import OptimConfig

from . import clip_step_cases as cc
from . import step_cases as sc
from .dist_utils import run_ranks
from .ref_train import loss_fn
from .test_entrypoints_gpu import _run, _summary

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ the protocol
@pytest.mark.parametrize("cell", cc.CLIP_CELLS, ids=[c.id for c in cc.CLIP_CELLS])
def test_clip_twin_readout(cell):
    ros, fails = cc.run_clip_cell(cell, DEV, subset=cell.id in cc.SUBSET_IDS)
    for r in ros:
        ro = r["bind"]
        print(f"CLIP_READOUT {cell.id} t={ro.t} norm={ro.norm.tolist()} "
              f"gA_norm={ro.g_plain.double().square().sum(1).sqrt().tolist()}")
    assert not fails, "\n".join(fails)
    assert len(ros) == len(sc.readout_steps(cell))


# ------------------------------------------------------------------------------ trajectories
def _clipped_fp64_loop(cell, ocfg: OptimConfig, steps: int):
    """Plain autograd + torch.optim in fp64 with torch's clipping per model between backward and
    opt.step(): (params [n, P] fp32, losses [steps, n] fp32, norms before clipping [steps, n])."""
    X, Y = sc.cell_data(cell)
    X = X.double()
    stream = EpochIndexStream(sc.cell_geom(cell))
    params = [torch.nn.Parameter(p.double().clone()) for p in sc.cell_init(cell)]
    plain = replace(ocfg, max_grad_norm=0.0, clip_grad_value=0.0)
    opts = [plain.torch_optimizer([p]) for p in params]
    losses, norms = [], []
    for t in range(steps):
        ix = torch.tensor(stream.indices(t), dtype=torch.long)
        row, nrow = [], []
        for p, opt in zip(params, opts):
            opt.zero_grad()
            lo = loss_fn(mlp_forward_ref(p, cell.spec, X[ix]), Y[ix].double() if cell.loss == "mse" else Y[ix], cell.loss)
            lo.backward()
            nrow.append(p.grad.norm().item())
            if ocfg.max_grad_norm > 0:
                torch.nn.utils.clip_grad_norm_([p], ocfg.max_grad_norm)
            elif ocfg.clip_grad_value > 0:
                torch.nn.utils.clip_grad_value_([p], ocfg.clip_grad_value)
            opt.step()
            row.append(lo.item())
        losses.append(row)
        norms.append(nrow)
    return (torch.stack([p.detach().float() for p in params]), torch.tensor(losses, dtype=torch.float32),
            torch.tensor(norms, dtype=torch.float64))


_ADAM = OptimConfig(lr=1e-2)
_TRAJ = {  # cell, optimizer, clipping ("bind": the cell's C_bind), expected pick
    "T-adam-b256-grp4": (sc.BY_ID["T-adam-mse-fp32-b256-gon"], _ADAM, {"max_grad_norm": 1e-7}),
    "T-sgd-b128": (sc.BY_ID["T-sgd-mse-fp32-b128-goff"], sc.SGD, "bind"),
    "T-sgd-b128-wd": (sc.BY_ID["T-sgd-mse-fp32-b128-goff"], replace(sc.SGD, weight_decay=1e-2), "bind"),
    "C4-ce-adam-b64": (sc._lanes("C4", "adam", "ce", 64, 4), _ADAM, {"max_grad_norm": 1e-7}),
    "H15-adam-b200-one-lane": (sc.BY_ID["H15-adam-mse-fp32-b200-goff"], _ADAM, {"max_grad_norm": 1e-7}),
    "T-sgd-b128-value": (sc.BY_ID["T-sgd-mse-fp32-b128-goff"], sc.SGD, "value"),
}


@pytest.mark.parametrize("name", list(_TRAJ))
def test_clipped_trajectory_matches_clipped_fp64_loop(name):
    cell, ocfg, clip = _TRAJ[name]
    if clip == "bind":
        clip = {"max_grad_norm": cc.bounds(cell).c_bind}
    elif clip == "value":
        clip = {"clip_grad_value": cc.bounds(cell).c_val}
    ocfg = replace(ocfg, **clip)
    steps = 2 * sc.cell_geom(cell).steps_per_epoch + 3
    ref_p, ref_l, ref_n = _clipped_fp64_loop(cell, ocfg, steps)
    # the conditions, on the reference: every step binds with room, and clipping matters --
    # the unclipped reference misses the tolerance tenfold on a quarter of the elements
    if ocfg.max_grad_norm > 0:
        assert (ref_n >= 1.25 * ocfg.max_grad_norm).all(), ref_n.min().item()
    un_p, _, _ = _clipped_fp64_loop(cell, replace(ocfg, max_grad_norm=0.0, clip_grad_value=0.0), steps)
    far = (un_p - ref_p).abs() > 10 * (2e-5 + 1e-4 * ref_p.abs())
    assert far.double().mean() >= 0.25, far.double().mean().item()
    tr = cc.make_clip_trainer(cell, DEV, ocfg, steps_per_launch=7)
    try:
        assert tr.clip_in_kernel and (tr.lanes, tr.kernel_waves, tr.groups) == cell.expect
        tr.train(steps)
        tr.synchronize()
        torch.testing.assert_close(tr.losses(0, steps), ref_l, rtol=2e-4, atol=1e-5)
        torch.testing.assert_close(tr.params.cpu(), ref_p, rtol=1e-4, atol=2e-5)
        assert tr.step_ctr.tolist() == [steps] * sc.N_MODELS
        if ocfg.max_grad_norm > 0:  # the last step's norm before clipping
            torch.testing.assert_close(tr.grad_norm.cpu().double(), ref_n[-1], rtol=1e-3, atol=0)
        else:
            assert tr.grad_norm is None
    finally:
        tr.close()


# ------------------------------------------------------------------------------ launch modes
@pytest.mark.parametrize("cid", ["T-adam-mse-fp32-b256-gon", "T-sgd-mse-fp32-b128-goff", "H15-adam-mse-fp32-b200-goff"])
def test_launch_modes_bitwise_equal_under_clipping(cid):
    """Seven-step persistent launches, one-step eager launches and graph replays: the clip twin
    needs no host work, so it is the same run bit for bit -- grad_norm included."""
    cell = sc.BY_ID[cid]
    ocfg = cc.clip_optim(cell, max_grad_norm=cc.bounds(cell).c_bind)
    res = {}
    for name, cfg in (("persistent", {"steps_per_launch": 7}), ("eager", {"launch": "eager"}),
                      ("graph", {"launch": "graph", "steps_per_launch": 7})):
        tr = cc.make_clip_trainer(cell, DEV, ocfg, **cfg)
        try:
            assert tr.clip_in_kernel and (tr.lanes, tr.kernel_waves, tr.groups) == cell.expect
            tr.train(14)
            tr.synchronize()
            res[name] = [t.detach().cpu().clone() for t in (tr.params, tr.m, tr.v, tr.losses(0, 14), tr.grad_norm)]
        finally:
            tr.close()
    assert torch.isfinite(res["persistent"][4]).all() and (res["persistent"][4] > 0).all()
    for name in ("eager", "graph"):
        for a, b, what in zip(res["persistent"], res[name], ("params", "m", "v", "losses", "grad_norm")):
            assert torch.equal(a, b), (name, what)


# ------------------------------------------------------------------------------ the C API
def _last_error() -> str:
    return (nat.load().dtp_last_error() or b"").decode()


def _engine_variant(lib, tr) -> int:
    rec = nat.StepPick()
    assert lib.dtp_train_engine_pick(tr._engine_handle(), ctypes.byref(rec)) == 0
    return rec.variant


def test_c_api_refusals_and_raw_local_gradients():
    lib = nat.load()
    cell = sc.BY_ID["T-adam-mse-fp32-b256-gon"]
    b = cc.bounds(cell)
    tr = cc.make_clip_trainer(cell, DEV, cc.clip_optim(cell, max_grad_norm=b.c_bind))
    plain = sc.make_trainer(cell, DEV)
    try:
        key = cell.spec.key[:4]

        def refused(a, mode):
            rc = lib.dtp_mlp_train(ctypes.byref(a), *key, mode, nat.stream_ptr())
            assert rc != 0 and "clipping" in _last_error(), (rc, _last_error())
            rec = nat.StepPick(9, 9, 9, 9)
            assert lib.dtp_mlp_train_pick(ctypes.byref(a), *key, mode, ctypes.byref(rec)) != 0
            assert (rec.lanes, rec.waves, rec.groups, rec.variant) == (0, 0, 0, 0)
            assert not lib.dtp_train_engine_create(ctypes.byref(a), *key, mode)

        before = [t.clone() for t in (tr.params, tr.m, tr.v, tr.step_ctr)]
        a = tr._train_args(1, nat.MODE_ADAM, None)
        assert a.max_norm > 0 and a.clip_value == 0 and a.norm_out == tr.grad_norm.data_ptr()
        a.clip_value = 0.5
        refused(a, nat.MODE_ADAM)                      # both fields set
        a = tr._train_args(1, nat.MODE_ADAM, None)
        a.max_norm = -1.0
        refused(a, nat.MODE_ADAM)                      # a negative value
        a = tr._train_args(1, nat.MODE_ADAM, None)
        a.max_norm, a.clip_value = 0.0, -0.5
        refused(a, nat.MODE_ADAM)
        a = tr._train_args(1, nat.MODE_ADAM, None)
        a.norm_out = None
        refused(a, nat.MODE_ADAM)                      # max_norm without norm_out
        for field in ("max_norm", "clip_value"):       # MODE_GRAD writes the raw gradient
            a = tr._train_args(1, nat.MODE_GRAD, None)
            assert a.max_norm == 0 and a.clip_value == 0 and not a.norm_out
            setattr(a, field, 0.5)
            a.norm_out = nat.ptr(tr.grad_norm)
            refused(a, nat.MODE_GRAD)
        torch.cuda.synchronize()
        for x, y in zip(before, (tr.params, tr.m, tr.v, tr.step_ctr)):
            assert torch.equal(x, y)
        # the clipping engine is a twin, the plain one is not; the profile instance has no twin
        assert _engine_variant(lib, tr) == 1 and tr.clip_in_kernel
        assert _engine_variant(lib, plain) == 0 and not plain.clip_in_kernel
        prof = torch.zeros(8 * 4 * 8 * 32, dtype=torch.int64, device=DEV)
        rc = lib.dtp_train_engine_profile(tr._engine_handle(), 1, 0, nat.ptr(prof), nat.stream_ptr())
        assert rc != 0 and "clipping" in _last_error()
        # local_gradients() on a clipping engine: the raw gradient, the plain engine's bits
        g, lo = tr.local_gradients()
        gp, lp = plain.local_gradients()
        assert torch.equal(g, gp) and torch.equal(lo, lp)
        assert (g.double().square().sum(1).sqrt() > 1.9 * b.c_bind).all()
    finally:
        tr.close()
        plain.close()


_FORCED_SCRIPT = r"""
import sys, torch
sys.path.insert(0, {root!r})
from dataclasses import replace
from tests import clip_step_cases as cc, step_cases as sc
cell = replace(sc.BY_ID["T-adam-mse-fp32-b256-gon"], groups={groups!r})
dev = torch.device("cuda", 0)
b = cc.bounds(cell)
tr = cc.make_clip_trainer(cell, dev, cc.clip_optim(cell, max_grad_norm=b.c_bind))
pl = sc.make_trainer(cell, dev)
print("PICK", tr.lanes, tr.kernel_waves, tr.groups, int(tr.clip_in_kernel), pl.lanes, pl.kernel_waves, pl.groups)
tr.train(3)
tr.synchronize()
assert torch.isfinite(tr.params).all() and (tr.grad_norm > b.c_bind).all()
"""


@pytest.mark.parametrize("env,groups,plain", [({"DTP_LANES": "2x8"}, "auto", (2, 8, 1)),
                                              ({"DTP_GRP_NW": "8"}, "on", (4, 8, 2))])
def test_forced_8_wave_pick_resolves_unforced_under_clipping(env, groups, plain):
    """The 8-wave instances have no twin: with clipping the pick is the unforced one (batch 256
    on one rank: the split-batch step with 4 members), while the plain engine runs as forced."""
    r = subprocess.run([sys.executable, "-c", _FORCED_SCRIPT.format(root=ROOT, groups=groups)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=200, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    pick = [int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("PICK")][-1].split()[1:]]
    assert tuple(pick[:4]) == (4, 4, 4, 1) and tuple(pick[4:]) == plain, pick


def test_demo_fused_engine_clips_on_gpu(tmp_path):
    """demo.py --engine fused --clip_grad_norm X runs the fused engine and reports grad_norm; X
    comes from a probe run with a bound that cannot bind, as in tests/test_clip_cpu.py."""
    base = ["demo.py", "--engine", "fused", "--optimizer", "sgd", "--lr", "0.05", "--seed", "11", "--dry_run",
            "--no_progress", "--log_dir", str(tmp_path)]
    probe = _summary(_run([*base, "--iters", "1", "--clip_grad_norm", "1e9"]))
    first = probe["grad_norm"]
    assert probe["engine"] == "fused" and len(first) == 2 and all(0 < n < 1e9 for n in first), probe
    x = 0.1 * min(first)
    plain = _summary(_run([*base, "--iters", "20"]))
    out = _run([*base, "--iters", "20", "--clip_grad_norm", repr(x)])
    clipped = _summary(out)
    assert "engine: fused" in out and "using the module engine" not in out
    assert clipped["engine"] == plain["engine"] == "fused" and clipped["iters"] == 20 and "grad_norm" not in plain
    assert len(clipped["grad_norm"]) == 2 and all(n > x for n in clipped["grad_norm"]), clipped
    assert all(v == v for v in clipped["final_loss"]) and clipped["final_loss"] != plain["final_loss"], (clipped, plain)


# ------------------------------------------------------------------------------ several ranks
_spawned: dict = {}


def _spawn(world):
    if world not in _spawned:
        lost = [k for k, v in _spawned.items() if isinstance(v, BaseException)]
        if lost:  # ranks died or never answered: nothing more is started on that GPU
            _spawned[world] = RuntimeError(f"not started: the spawn of W = {lost[0]} failed")
        else:
            try:
                _spawned[world] = run_ranks(cc.world_rank, world, ([c.id for c in cc.WORLD_CELLS[world]],), timeout=200)
            except BaseException as e:
                _spawned[world] = e
    if isinstance(_spawned[world], BaseException):
        raise AssertionError(f"the spawn of W = {world} failed") from _spawned[world]
    return _spawned[world]


@pytest.fixture(scope="module")
def spawned():
    yield _spawn
    _spawned.clear()


_WORLD = [c for cs in cc.WORLD_CELLS.values() for c in cs]


@pytest.mark.parametrize("cell", _WORLD, ids=[c.id for c in _WORLD])
def test_xgmi_clip_twins_on_several_ranks(cell, spawned):
    """The engine stays on xGMI under clipping (its self-test compares the clipping kernel with
    the clipping flat reference), every rank clips the summed gradient by the same coefficient,
    and norm, parameters and m are equal across the ranks bit for bit."""
    res = spawned(cell.world)
    stopped = [res[r]["stopped"] for r in sorted(res) if res[r]["stopped"]]
    if any(cell.id not in res[r]["cells"] for r in res):
        pytest.fail(f"{cell.id}: not run; the spawn stopped at\n" + "\n".join(stopped[:1]))
    fails = cc.evaluate_world_cell(cell, {r: res[r]["cells"][cell.id] for r in res})
    assert not fails, "\n".join(fails)

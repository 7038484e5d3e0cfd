"""Gradient accumulation inside the several-lanes / split-batch step kernel (GPU only): the
accumulation twins of ``csrc/mlp_train_lanes.hip`` (``csrc/accum_core.h``).

* the read-out protocol of ``tests/accum_cases.py`` over one cell per twin: the gradient the
  optimizer took against the mean over the window's micro-batches of fp64 autograd;
* a window reads the samples of one big batch: (batch 64, A = 4) and (batch 128, A = 2) against the
  plain split-batch step at batch 256;
* the twin at A = 1 (``DTP_ACCUM_TWIN=1``, a child process) is the plain step bit for bit;
* clipping inside the twin; a scheduled trajectory against the fp64 loop; persistent, eager and
  graph launches bitwise equal; the permutation ring refilled by micro-steps; resume;
* the C API's refusals and the picks without a twin;
* two and three ranks on one GPU: the xGMI twins;
* ``demo.py --accumulate_grad_batches`` on the three engines, and the fused engine's fall to the
  module engine where its pick has no twin.
"""
import ctypes
import json
import os
import subprocess
import sys
from dataclasses import replace

import pytest
import torch

from distributed_training_pytorch_amd import _native as nat
from distributed_training_pytorch_amd.data.sampler import SamplerGeometry
from distributed_training_pytorch_amd.data.toy_data import ToyData
from distributed_training_pytorch_amd.engine.fused_trainer import EngineConfig, FusedTrainer
from distributed_training_pytorch_amd.ops.optim import OptimConfig

from . import accum_cases as ac
from . import clip_step_cases as cc
from . import step_cases as sc
from .dist_utils import run_ranks
from .sched_cases import torch_train_sched
from .test_fused_accum_cpu import trajectory_optim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENV_KEYS = ("DTP_LANES", "DTP_FAST", "DTP_GRP_NW", "DTP_GROUPS", "DTP_ACCUM_TWIN")


def _report(recs, fails):
    for r in recs:
        print("ACCUM_MATRIX " + json.dumps(r))
    assert not fails, "\n".join(fails)
    assert recs


# ------------------------------------------------------------------------------ 1. the read-out
@pytest.mark.parametrize("cell", ac.CELLS, ids=[c.id for c in ac.CELLS])
def test_accum_twin_readout(cell):
    _report(*ac.run_accum_cell(cell, DEV))


# ------------------------------------------------------------------------------ 2. one big batch
@pytest.mark.parametrize("batch,A,lanes", [(64, 4, 4), (128, 2, 2)])
def test_window_reads_the_samples_of_one_big_batch(batch, A, lanes):
    """One rank, n = 512, full batches: the window reads exactly the samples of the plain
    split-batch step at batch 256.  The two read-outs (taken at the same parameters) agree within
    the sum of their two fp32 bounds -- not bitwise, the summation order differs."""
    small = ac.AccumCell(sc._lanes("T", "adam", "mse", batch, lanes), A)
    big = sc.BY_ID["T-adam-mse-fp32-b256-gon"]
    X, Y = sc.cell_data(big)
    ta, tb = ac.make_trainer(small, DEV), sc.make_trainer(big, DEV)
    try:
        assert ta.accum_in_kernel and (ta.lanes, ta.kernel_waves, ta.groups) == small.cell.expect
        assert (tb.lanes, tb.kernel_waves, tb.groups) == big.expect
        for t in ac.READOUT_STEPS:
            tb.params.copy_(ta.params)
            sa, sb = sc.step_gradient(ta), sc.step_gradient(tb)
            ia = [ta.step_indices(u) for u in ta.micro_batches(t)]
            assert sorted(sum(ia, [])) == sorted(tb.step_indices(t)) and sum(ia, []) == tb.step_indices(t)
            ra, fa = ac.evaluate_window(small, sa, ia, X, Y)
            rb, fb = sc.evaluate_step(big, sb, tb.step_indices(t), X, Y)
            assert not fa + fb, "\n".join(fa + fb)
            for i in range(sc.N_MODELS):
                d = sc.metric(big.spec, sa.grad[i], sb.grad[i])
                for n, e in d.items():
                    bound = ra[i]["bound"][n] + rb[i]["bound"][n]
                    print(f"BIG_BATCH b{batch} A{A} t={t} model {i} {n}: {e:.3e} bound {bound:.3e}")
                    assert e <= bound, (t, i, n, e, bound)
                el, bl = sc.rel(sa.loss[i], sb.loss[i]), ra[i]["bound_loss"] + rb[i]["bound_loss"]
                assert el <= bl, (t, i, el, bl)
    finally:
        ta.close()
        tb.close()


# ------------------------------------------------------------------------------ 3. the twin at A = 1
_TWIN_IDS = ["T-adam-mse-fp32-b100-goff-n300-A2", "T-adam-mse-fp32-b64-goff-n300-A3", "T-adam-mse-fp32-b192-gon-A2",
             "T-adam-mse-fp32-b256-gon-A2", "T-adam-mse-bf16-b64-goff-n300-A3", "T-sgd-mse-fp32-b100-goff-n300-A2",
             "C4-adam-ce-fp32-b256-gon-A2"]


@pytest.fixture(scope="module")
def twin_child(tmp_path_factory):
    """DTP_ACCUM_TWIN is read once per process: one child runs every cell at accumulate = 1."""
    out = str(tmp_path_factory.mktemp("accum") / "twin.pt")
    base = {k: v for k, v in os.environ.items() if k not in _ENV_KEYS}
    r = subprocess.run([sys.executable, "-m", "tests.accum_cases", "twin", out, *_TWIN_IDS], cwd=ROOT,
                       env={**base, "DTP_ACCUM_TWIN": "1"}, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


@pytest.mark.parametrize("cid", _TWIN_IDS)
def test_twin_at_one_micro_batch_is_the_plain_step(cid, twin_child):
    cell = ac.BY_ID[cid]
    twin, plain = twin_child[cid], ac.twin_state(cell, DEV, A=1)
    assert twin["twin"] and not plain["twin"]
    assert tuple(twin["pick"]) == tuple(plain["pick"]) == cell.cell.expect
    for k in ("params", "m", "v", "step"):
        assert torch.equal(twin[k], plain[k]), k
    assert twin["t"] == plain["t"] == 6
    one = ac.AccumCell(cell.cell, 1)
    fails = []
    for k in range(3):  # the twin scales the loss per micro-batch: held to the reference, not bitwise
        assert torch.equal(twin["before"][k], plain["before"][k])
        fails += ac.loss_failures(one, twin["before"][k], 3 + k, twin["losses"][3 + k])
        fails += ac.loss_failures(one, plain["before"][k], 3 + k, plain["losses"][3 + k])
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------ 4. clipping inside the twin
@pytest.mark.parametrize("cell", [ac.LANES4, ac.AccumCell(ac.GRP4.cell, 3)], ids=["lanes4", "grp4"])
def test_clipping_inside_the_twin(cell):
    """``clip_step_cases``' protocol with a plain accumulating engine A and clipping accumulating
    engines B: by a norm that binds, by one that cannot, by value."""
    b = ac.bounds(cell)
    kinds = {"bind": ("max_grad_norm", b.c_bind), "free": ("max_grad_norm", b.c_free), "value": ("clip_grad_value", b.c_val)}
    A = ac.make_trainer(cell, DEV)
    Bs = {k: ac.make_trainer(cell, DEV, ac.accum_optim(cell, **{f: c})) for k, (f, c) in kinds.items()}
    fails = []
    try:
        for tr in (A, *Bs.values()):
            assert tr.accum_in_kernel and (tr.lanes, tr.kernel_waves, tr.groups) == cell.cell.expect
            assert not tr.clip_in_kernel or tr.optim.clips
        for t in ac.READOUT_STEPS:
            for k, ro in cc.clip_readout(A, Bs).items():
                assert ro.t == t
                fails += cc.evaluate_readout(cell.cell, ro, k, kinds[k][1])
        for tr in (A, *Bs.values()):
            tr.check_comm()
    finally:
        for tr in (A, *Bs.values()):
            tr.close()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------ 5. trajectory
def test_trajectory_matches_the_fp64_loop():
    cell, ocfg = ac.LANES4, trajectory_optim()
    X, Y = sc.cell_data(cell.cell)
    ref_p, ref_l = torch_train_sched(cell.cell.spec, sc.cell_init(cell.cell), X, Y, ac.window_views(cell.cell, cell.A),
                                     12, ocfg)
    tr = ac.make_trainer(cell, DEV, ocfg, steps_per_launch=5)
    try:
        assert tr.accum_in_kernel and (tr.lanes, tr.kernel_waves, tr.groups) == cell.cell.expect
        tr.train(12)
        tr.synchronize()
        got_p = tr.params.cpu()
        print(f"TRAJ max rel param error {((got_p - ref_p).abs() / ref_p.abs()).max().item():.3e}, "
              f"max abs {(got_p - ref_p).abs().max().item():.3e}, min |p| {ref_p.abs().min().item():.3e}; "
              f"max rel loss error {((tr.losses(0, 12) - ref_l).abs() / ref_l.abs()).max().item():.3e}")
        torch.testing.assert_close(tr.losses(0, 12), ref_l, rtol=2e-4, atol=1e-5)
        torch.testing.assert_close(got_p, ref_p, rtol=1e-4, atol=0)
        assert tr.step_ctr.tolist() == [12] * sc.N_MODELS
    finally:
        tr.close()


# ------------------------------------------------------------------------------ 6. launch modes
@pytest.mark.parametrize("cell", [ac.LANES4, ac.AccumCell(ac.GRP4.cell, 3)], ids=["lanes4", "grp4"])
def test_launch_modes_bitwise_equal(cell):
    res = {}
    for name, cfg in (("persistent", {"steps_per_launch": 4}), ("eager", {"launch": "eager"}),
                      ("graph", {"launch": "graph", "steps_per_launch": 4})):
        tr = ac.make_trainer(cell, DEV, **cfg)
        try:
            assert tr.accum_in_kernel and (tr.lanes, tr.kernel_waves, tr.groups) == cell.cell.expect
            tr.train(7)
            tr.synchronize()
            assert tr.t == 7 and tr.step_ctr.tolist() == [7] * sc.N_MODELS
            res[name] = [t.detach().cpu().clone() for t in (tr.params, tr.m, tr.v, tr.losses(0, 7))]
        finally:
            tr.close()
    for name in ("eager", "graph"):
        for a, b, what in zip(res["persistent"], res[name], ("params", "m", "v", "losses")):
            assert torch.equal(a, b), (name, what)


# ------------------------------------------------------------------------------ 7. ring refill
# The ring test compares two fp32 runs of > 2048 optimizer steps at a loss tolerance of 2e-4.
# Their steps differ by roundings (~1e-7), which training amplifies: a perturbation of that size
# in the initial weights moves the CPU engine's own losses by 2e-3 under Adam at lr 1e-3 or SGD
# with momentum, by 5e-5 under plain SGD at lr 1e-3 and by 4e-7 at lr 1e-4 (the loss still falls
# from 3.45 to 1.47).  So the run uses plain SGD at 1e-4: the comparison then measures the
# samples and the arithmetic, not the conditioning of a long trajectory.
_RING_SGD = OptimConfig("sgd", 1e-4)


def _small_trainer(n, device, A, optim, steps_per_launch=1000):
    ds = ToyData(n=n, seed=sc.DATA_SEED)
    g = torch.Generator().manual_seed(sc.INIT_SEED)
    spec = sc.SHAPES["T"]
    init = [torch.randn(spec.P, generator=g) * 0.4]
    geom = SamplerGeometry(n=n, world=1, rank=0, batch=64, seed=sc.SAMPLER_SEED)
    return FusedTrainer(spec, 1, ds.X.to(device), ds.Y.to(device), geom, optim,
                        EngineConfig(sampler="torch", accumulate=A, steps_per_launch=steps_per_launch),
                        init_params=[p.to(device) for p in init])


def test_ring_is_refilled_by_micro_steps():
    """n = 64, batch 64, A = 4: an epoch per micro-step, so the micro-steps pass the permutation
    ring's length while the optimizer steps do not; the losses are the CPU engine's."""
    tr = _small_trainer(64, DEV, 4, _RING_SGD)
    try:
        E = tr._ring.E
        steps = E // 4 + 40
        assert steps < E < steps * 4
        tr.train(steps)
        tr.synchronize()
        assert tr.accum_in_kernel and tr._ring.hi >= steps * 4 - 1 and tr._ring.lo > 0
        got = tr.losses(0, steps)
    finally:
        tr.close()
    cpu = _small_trainer(64, torch.device("cpu"), 4, _RING_SGD)
    cpu.train(steps)
    torch.testing.assert_close(got, cpu.losses(0, steps), rtol=2e-4, atol=1e-5)


def test_ring_refill_feeds_the_right_samples():
    """n = 128 (two batches per epoch, so a stale permutation is other samples): behind the
    ring's length the read-out is still the window's gradient.  The read-out is taken at the
    initial weights, put back after the steps that pass the ring's length: the bound is
    ``step_cases``' for a draw like its cells', not for wherever 4000 steps of training end."""
    tr = _small_trainer(128, DEV, 4, sc.ADAM)
    try:
        E = tr._ring.E
        steps = (2 * E) // 4 + 10
        init = tr.params.detach().clone()
        tr.train(steps)
        tr.synchronize()
        assert tr._ring.lo > 0 and not torch.equal(tr.params, init)
        tr.params.copy_(init)
        p0 = tr.params.detach().cpu().clone()
        sg = sc.step_gradient(tr)
        assert sg.t == steps and torch.equal(sg.params_before, p0)
        idx = [tr.step_indices(u) for u in tr.micro_batches(steps)]
        cell = ac.AccumCell(sc._lanes("T", "adam", "mse", 64, 4, n=128), 4)
        X, Y = sc.cell_data(cell.cell)
        _report(*ac.evaluate_window(cell, sg, idx, X, Y, n_models=1))
    finally:
        tr.close()


# ------------------------------------------------------------------------------ 8. resume
@pytest.mark.parametrize("cell", [ac.LANES4, ac.GRP4], ids=["lanes4", "grp4"])
def test_resume_is_bitwise_the_uninterrupted_run(cell):
    a, b, c = (ac.make_trainer(cell, DEV) for _ in range(3))
    try:
        a.train(4)
        a.synchronize()
        sd = a.state_dict()
        assert sd["accumulate"] == cell.A
        b.load_state_dict(sd)
        b.train(4)
        c.train(8)
        b.synchronize()
        c.synchronize()
        for x, y in zip((b.params, b.m, b.v, b.step_ctr, b.losses(4, 8)), (c.params, c.m, c.v, c.step_ctr, c.losses(4, 8))):
            assert torch.equal(x, y)
        other = ac.make_trainer(cell, DEV, A=cell.A + 1)
        try:
            with pytest.raises(ValueError, match="accumulate"):
                other.load_state_dict(sd)
        finally:
            other.close()
    finally:
        for tr in (a, b, c):
            tr.close()


# ------------------------------------------------------------------------------ 9. the C API
def _last_error() -> str:
    return (nat.load().dtp_last_error() or b"").decode()


def _engine_variant(lib, tr) -> int:
    rec = nat.StepPick()
    assert lib.dtp_train_engine_pick(tr._engine_handle(), ctypes.byref(rec)) == 0
    return rec.variant


def test_c_api_refusals():
    lib = nat.load()
    cell = ac.GRP4
    tr = ac.make_trainer(cell, DEV)
    try:
        key = cell.cell.spec.key[:4]
        before = [t.clone() for t in (tr.params, tr.m, tr.v, tr.step_ctr)]

        def refused(a, mode, word):
            rc = lib.dtp_mlp_train(ctypes.byref(a), *key, mode, nat.stream_ptr())
            assert rc != 0 and word in _last_error(), (rc, _last_error())
            rec = nat.StepPick(9, 9, 9, 9)
            assert lib.dtp_mlp_train_pick(ctypes.byref(a), *key, mode, ctypes.byref(rec)) != 0
            assert (rec.lanes, rec.waves, rec.groups, rec.variant) == (0, 0, 0, 0)
            assert not lib.dtp_train_engine_create(ctypes.byref(a), *key, mode)

        a = tr._train_args(1, nat.MODE_ADAM, None)
        assert a.accum == cell.A and abs(a.hp.grad_scale - 1.0 / cell.A) < 1e-7
        a.accum = -1
        refused(a, nat.MODE_ADAM, "accum")
        a = tr._train_args(1, nat.MODE_GRAD, None)
        assert a.accum == 0 and a.hp.grad_scale == 1.0
        a.accum = 2
        refused(a, nat.MODE_GRAD, "MODE_GRAD")
        a = tr._train_args(1, nat.MODE_ADAM, None)
        a.host_t0 = (1 << 30)  # t0 * accum past 2^31 - 1
        refused(a, nat.MODE_ADAM, "2^31")
        a = tr._train_args(1 << 20, nat.MODE_ADAM, None)
        a.accum = 1 << 12      # n_steps * accum
        refused(a, nat.MODE_ADAM, "2^31")
        # the profile entry points
        a = tr._train_args(1, nat.MODE_ADAM, None)
        assert lib.dtp_mlp_train_profile(ctypes.byref(a), nat.stream_ptr()) != 0 and "accumulation" in _last_error()
        assert lib.dtp_mlp_train_profile_lanes(ctypes.byref(a), 4, nat.stream_ptr()) != 0 and "accumulation" in _last_error()
        prof = torch.zeros(8 * 4 * 8 * 32, dtype=torch.int64, device=DEV)
        assert _engine_variant(lib, tr) == 2
        rc = lib.dtp_train_engine_profile(tr._engine_handle(), 1, 0, nat.ptr(prof), nat.stream_ptr())
        assert rc != 0 and "accumulation" in _last_error()
        # the direct launch has no split-batch step (it owns no exchange buffer): batch 256 picks
        # the one-lane kernel, which has no twin
        a = tr._train_args(1, nat.MODE_ADAM, None)
        a.host_t0 = 0
        rc = lib.dtp_mlp_train(ctypes.byref(a), *key, nat.MODE_ADAM, nat.stream_ptr())
        assert rc == -6 and "without an accumulation twin" in _last_error(), (rc, _last_error())
        torch.cuda.synchronize()
        for x, y in zip(before, (tr.params, tr.m, tr.v, tr.step_ctr)):
            assert torch.equal(x, y)
    finally:
        tr.close()
    # batch 256 with groups="off": the engine refuses, it does not run a plain step
    off = ac.make_trainer(ac.AccumCell(replace(cell.cell, groups="off"), 2), DEV)
    try:
        assert off.lanes == 0
        with pytest.raises(RuntimeError, match="without an accumulation twin"):
            off.train(1)
        assert off.t == 0 and off.step_ctr.tolist() == [0, 0]
    finally:
        off.close()
    plain = ac.make_trainer(cell, DEV, A=1)
    try:
        assert _engine_variant(lib, plain) == 0 and not plain.accum_in_kernel
    finally:
        plain.close()


def test_forced_picks_under_accumulation(tmp_path):
    """A forced one-lane pick has no twin: an error.  A forced 8-wave pick is ignored."""
    base = {k: v for k, v in os.environ.items() if k not in _ENV_KEYS}
    res = {}
    for env in ("1", "4x8"):
        out = str(tmp_path / f"pick_{env}.json")
        r = subprocess.run([sys.executable, "-m", "tests.accum_cases", "pick", out, ac.LANES4.id], cwd=ROOT,
                           env={**base, "DTP_LANES": env}, capture_output=True, text=True, timeout=200)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(out) as fh:
            res[env] = json.load(fh)[ac.LANES4.id]
    assert res["1"]["error"] and "without an accumulation twin" in res["1"]["error"], res["1"]
    assert res["4x8"]["error"] is None and tuple(res["4x8"]["pick"]) == (4, 4, 1), res["4x8"]


# ------------------------------------------------------------------------------ 10. several ranks
def _world_rank(rank: int, world: int) -> dict:
    import torch.distributed as dist

    cell = ac.WORLD_CELLS[world]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"rank": rank, "readouts": [], "fails": []}
    tr = ac.make_trainer(cell, dev, rank=rank)
    try:
        out["pick"] = [tr.lanes, tr.kernel_waves, tr.groups]
        out["comm"], out["fallback"], out["twin"] = tr.comm, tr.comm_fallback_reason, tr.accum_in_kernel
        ok = tr.comm == "xgmi" and tuple(out["pick"]) == cell.cell.expect and out["twin"]
        if not sc._all_ranks(ok):
            return out
        tr.synchronize()
        tr.exchange_stats_reset()
        for t in ac.READOUT_STEPS:
            err = None
            try:
                sg = sc.step_gradient_world(tr)
                assert sg.t == t
                out["readouts"].append(tuple(sg))
                out["indices"] = [tr.step_indices(u) for u in tr.micro_batches(t)]
            except Exception as e:  # an exchange timeout, a launch error
                err = f"rank {rank} t={t}: {type(e).__name__}: {e}"
                out["fails"].append(err)
            if not sc._all_ranks(err is None):
                return out
        out["stats"] = tr.exchange_stats_full()
        out["step_ctr"], out["t"] = tr.step_ctr.tolist(), tr.t
        dist.barrier()
    finally:
        tr.close()
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_xgmi_twins_on_several_ranks(world):
    """The engine's xGMI self-test passes under accumulation, the read-out is the mean over ranks
    and micro-batches of fp64 autograd, equal across the ranks bit for bit, and the exchange
    runs once per optimizer step."""
    cell = ac.WORLD_CELLS[world]
    res = run_ranks(_world_rank, world, (), timeout=200)
    assert sorted(res) == list(range(world))
    fails = []
    for r in range(world):
        o = res[r]
        fails += o["fails"]
        if o["comm"] != "xgmi" or o["fallback"] is not None or not o["twin"] or tuple(o["pick"]) != cell.cell.expect:
            fails.append(f"rank {r}: comm {o['comm']!r} (fallback: {o['fallback']}), twin {o['twin']}, pick {o['pick']}")
    assert not fails, "\n".join(fails)
    X, Y = sc.cell_data(cell.cell)
    recs = []
    for k, t in enumerate(ac.READOUT_STEPS):
        sgs = [sc.StepGradient(*res[r]["readouts"][k]) for r in range(world)]
        for r in range(1, world):
            for name in ("params_before", "grad", "loss", "params_after"):
                assert torch.equal(getattr(sgs[r], name), getattr(sgs[0], name)), (t, r, name)
        rc, f = ac.evaluate_window(cell, sgs[0], ac.window_indices(cell, t), X, Y)
        recs += rc
        fails += f
    for r in range(world):
        assert res[r]["step_ctr"] == [3] * sc.N_MODELS and res[r]["t"] == 3
        assert res[r]["stats"]["exchanges"] == 3, res[r]["stats"]
        own = ac.window_indices(cell, 2)[r * cell.A:(r + 1) * cell.A]
        assert res[r]["indices"] == own
    _report(recs, fails)


# ------------------------------------------------------------------------------ 11. the entry point
def test_demo_three_engines_agree(tmp_path):
    """demo.py --accumulate_grad_batches 3 --iters 12 --batch_size 64 on the fused, module and
    stock engines, same seed and data: the final losses agree pairwise at the tolerance
    tests/test_eval_gpu.py holds its loss values to."""
    from . import eval_cases as C
    from .test_entrypoints_gpu import _run, _summary

    base = ["demo.py", "--accumulate_grad_batches", "3", "--iters", "12", "--batch_size", "64", "--seed", "11",
            "--dry_run", "--no_progress"]
    final = {}
    for engine in ("fused", "module", "stock"):
        out = _run([*base, "--engine", engine, "--log_dir", str(tmp_path / engine)])
        s = _summary(out)
        assert s["engine"] == engine and s["accumulate_grad_batches"] == 3 and s["iters"] == 12, s
        if engine == "fused":
            assert "engine: fused" in out and "using the module engine" not in out
        final[engine] = torch.tensor(s["final_loss"], dtype=torch.float64)
        print(f"DEMO_ACCUM {engine} {s['final_loss']}")
    for a, b in (("fused", "module"), ("fused", "stock"), ("module", "stock")):
        torch.testing.assert_close(final[a], final[b], rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL, msg=lambda m: f"{a} vs {b}: {m}")


def test_demo_fused_falls_to_the_module_engine_without_a_twin(tmp_path):
    """2048 samples are past the several-lanes step's LDS budget: the fused pick is the one-lane
    kernel, which has no accumulation twin, so the run prints a note and takes the module engine
    -- and ends where the module engine asked for by name ends."""
    from .test_entrypoints_gpu import _run, _summary

    base = ["demo.py", "--accumulate_grad_batches", "2", "--iters", "6", "--n_samples", "2048", "--seed", "11",
            "--dry_run", "--no_progress"]
    out = _run([*base, "--engine", "fused", "--log_dir", str(tmp_path / "fused")])
    s = _summary(out)
    assert "has no accumulation twin: using the module engine" in out and s["engine"] == "module", out[-2000:]
    assert s["accumulate_grad_batches"] == 2 and s["iters"] == 6
    m = _summary(_run([*base, "--engine", "module", "--log_dir", str(tmp_path / "module")]))
    assert m["final_loss"] == s["final_loss"]
    # without accumulation the same run stays on the fused engine
    plain = _summary(_run([*base[:1], *base[3:], "--engine", "fused", "--log_dir", str(tmp_path / "plain")]))
    assert plain["engine"] == "fused" and plain["accumulate_grad_batches"] == 1

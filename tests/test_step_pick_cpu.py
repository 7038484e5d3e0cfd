"""The fused step's dispatcher on the CPU: ``dtp_mlp_train_pick`` validates a ``TrainArgs`` and
resolves the kernel instance a train engine would launch -- host code of ``csrc/mlp_train.hip``
over the tables of ``csrc/mlp_train_one.hip`` and ``csrc/mlp_train_lanes.hip`` -- without a
launch.  The argument block is filled by hand as ``FusedTrainer`` fills it; no pointer in it is
dereferenced, so one dummy address stands for every buffer.

Asserted: for every cell of ``step_cases`` the (lanes, waves, groups) its GPU matrix expects and
the plain variant; the clip twin (variant 1) of the same pick when the cell clips, the
accumulation twin (variant 2) for the cells of ``accum_cases``; an error code and a zeroed record
for instances that do not exist (-6 where an accumulating launch picks one without a twin) and
for what the validation refuses.  The environment variables that force an instance are read once
per process, so the cells that set one run in a child process per value
(``python -m tests.test_step_pick_cpu QUERIES.json OUT.json``)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCING = ("DTP_LANES", "DTP_FAST", "DTP_GRP_NW", "DTP_GROUPS", "DTP_ACCUM_TWIN")
DUMMY = 0x1000
TOY = (2, 10, 5, 1)
PLAIN, CLIP, ACCUM = 0, 1, 2  # DtpStepPick.variant
NONE = [0, 0, 0, 0]


def query(shape=TOY, mode=1, batch=256, n=512, world=1, loss=0, bf16=0, groups=0, cache=1, slope=0.01,
          grad_out=True, max_norm=0.0, clip_value=0.0, accum=0) -> dict:
    return dict(shape=list(shape), mode=mode, batch=batch, n=n, world=world, loss=loss, bf16=bf16, groups=groups,
                cache=cache, slope=slope, grad_out=grad_out, max_norm=max_norm, clip_value=clip_value, accum=accum)


def pick(lib, nat, q: dict) -> list:
    """[[lanes, waves, groups, variant], return code] of the step for query q (a zeroed record and
    a non-zero code: refused or no instance)."""
    a = nat.TrainArgs()
    for f in ("X", "Y", "params", "opt_m", "opt_v", "step", "status", "peers", "epoch", "norm_out"):
        setattr(a, f, DUMMY)
    if q["grad_out"]:
        a.grad_out = DUMMY
    a.n_models, a.n_steps, a.host_t0 = 2, 1, 0
    a.loss, a.cache_data, a.bf16, a.groups = q["loss"], q["cache"], q["bf16"], q["groups"]
    a.max_norm, a.clip_value, a.accum = q["max_norm"], q["clip_value"], q["accum"]
    a.hp.slope = q["slope"]
    s = a.smp
    s.mode, s.perm, s.perm_epochs = nat.SAMPLER_TABLE, DUMMY, 4
    s.n, s.world, s.rank, s.batch = q["n"], q["world"], 0, q["batch"]
    s.num_samples = -(-q["n"] // q["world"])
    s.steps_per_epoch = -(-s.num_samples // q["batch"])
    rec = nat.StepPick(9, 9, 9, 9)
    rc = lib.dtp_mlp_train_pick(ctypes.byref(a), *q["shape"], q["mode"], ctypes.byref(rec))
    return [[rec.lanes, rec.waves, rec.groups, rec.variant], rc]


def picks(queries: list, env: tuple = ()) -> list:
    """pick() of every query: in this process, or in a child under ``env`` (also when this
    process itself runs under one of the forcing variables)."""
    if not env and not any(k in os.environ for k in FORCING):
        from distributed_training_pytorch_amd import _native as nat

        lib = nat.load()
        return [pick(lib, nat, q) for q in queries]
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        qf, of = os.path.join(d, "q.json"), os.path.join(d, "out.json")
        with open(qf, "w") as fh:
            json.dump(queries, fh)
        base = {k: v for k, v in os.environ.items() if k not in FORCING}
        r = subprocess.run([sys.executable, "-m", "tests.test_step_pick_cpu", qf, of], cwd=ROOT,
                           env={**base, **dict(env)}, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(of) as fh:
            return json.load(fh)


@pytest.fixture(scope="module")
def native():
    from distributed_training_pytorch_amd import _native as nat

    try:
        nat.load()
    except nat.NativeUnavailable as e:
        pytest.skip(f"native library not built: {e}")
    return nat


def _cell_query(nat, c) -> dict:
    adam = c.opt == "adam"
    if c.world > 1:
        mode = nat.MODE_XGMI_ADAM if adam else nat.MODE_XGMI_SGD
    else:
        mode = nat.MODE_ADAM if adam else nat.MODE_SGD
    return query(c.spec.key[:4], mode, c.batch, c.n, c.world, nat.LOSS_CE if c.loss == "ce" else nat.LOSS_MSE,
                 int(c.prec == "bf16"), {"auto": 0, "on": 1, "off": -1}[c.groups], int(c.cache), c.spec.slope)


def _wrong(native, cells: list, variant: int, extra_env: tuple = (), **fields) -> list:
    """The cells whose query (with ``fields`` set) does not resolve to the cell's expected
    (lanes, waves, groups) in ``variant``; each under its own forcing environment."""
    wrong = []
    for env in sorted({c.env for c in cells}):
        group = [c for c in cells if c.env == env]
        got = picks([{**_cell_query(native, c), **fields} for c in group], env + extra_env)
        wrong += [(c.id, g) for c, g in zip(group, got) if g != [[*c.expect, variant], 0]]
    return wrong


def test_every_cell_gets_the_instance_its_matrix_expects(native):
    from . import step_cases as sc

    assert not _wrong(native, sc.ALL_CELLS + sc.ALL_XGMI, PLAIN)


@pytest.mark.parametrize("field", ["max_norm", "clip_value"])
def test_a_clipping_cell_gets_the_clip_twin_of_its_pick(native, field):
    """Every cell picks a 4-wave instance or is forced to an 8-wave one; the 4-wave ones have twins."""
    from . import step_cases as sc

    cells = [c for c in sc.ALL_CELLS + sc.ALL_XGMI if c.expect[1] == 4]
    assert len(cells) > 100
    assert not _wrong(native, cells, CLIP, **{field: 0.5})


def _accum_cells():
    from . import accum_cases as acc

    return acc.CELLS + list(acc.WORLD_CELLS.values())


@pytest.mark.parametrize("max_norm", [0.0, 0.5])
def test_an_accumulating_cell_gets_the_accumulation_twin_of_its_pick(native, max_norm):
    """... with clipping too: the accumulation twin clips at run time."""
    wrong = []
    for A in sorted({ac.A for ac in _accum_cells()}):
        wrong += _wrong(native, [ac.cell for ac in _accum_cells() if ac.A == A], ACCUM, accum=A, max_norm=max_norm)
    assert not wrong, wrong


def test_the_forced_accumulation_twin(native):
    """DTP_ACCUM_TWIN=1: a launch without accumulation runs the twin of its pick."""
    from . import step_cases as sc

    cells = [c for c in sc.CELLS + list(sc.XGMI_CELLS) if c.kind in ("lanes", "grp") and c.expect[1] == 4]
    assert {c.kind for c in cells} == {"lanes", "grp"} and not any(c.env for c in cells)
    assert not _wrong(native, cells, ACCUM, extra_env=(("DTP_ACCUM_TWIN", "1"),))


def test_a_pick_without_an_accumulation_twin_is_error_6(native):
    """Toy shape, batch 256, the split-batch step off: the one-lane kernel.  It has a clip twin."""
    assert picks([query(TOY, batch=256, groups=-1, accum=2)]) == [[NONE, -6]]
    assert picks([query(TOY, batch=256, groups=-1, max_norm=0.5)]) == [[[1, 4, 1, CLIP], 0]]


def test_a_forced_8_wave_pick_is_ignored_by_the_twins(native):
    """The 8-wave instances have no twins: a clipping or accumulating launch resolves as if
    DTP_LANES=4x8 had not been given (batch 100: 2 lanes), a plain one as forced."""
    env = (("DTP_LANES", "4x8"),)
    qs = [query(TOY, batch=100), query(TOY, batch=100, max_norm=0.5), query(TOY, batch=100, clip_value=0.5),
          query(TOY, batch=100, accum=2)]
    assert picks(qs, env) == [[[4, 8, 1, PLAIN], 0], [[2, 4, 1, CLIP], 0], [[2, 4, 1, CLIP], 0], [[2, 4, 1, ACCUM], 0]]
    assert picks(qs) == [[[2, 4, 1, PLAIN], 0], [[2, 4, 1, CLIP], 0], [[2, 4, 1, CLIP], 0], [[2, 4, 1, ACCUM], 0]]


def test_mode_grad_refuses_the_twins(native):
    nat = native
    qs = [query(TOY, nat.MODE_GRAD, 64, accum=2), query(TOY, nat.MODE_GRAD, 64, max_norm=0.5),
          query(TOY, nat.MODE_GRAD, 64, clip_value=0.5)]
    assert picks(qs) == [[NONE, -4]] * 3
    assert picks([query(TOY, nat.MODE_GRAD, 64)]) == [[[1, 4, 1, PLAIN], 0]]


def test_absent_instances_answer_zero(native):
    """An error code and a zeroed record."""
    nat = native
    qs = [query((2, 15, 5, 4), nat.MODE_ADAM, b) for b in (64, 128, 256)]                 # a shape outside the lists
    qs += [query((2, 10, 3, 1), nat.MODE_ADAM, b, bf16=1) for b in (64, 128, 256)]        # no bf16 instance
    assert picks(qs) == [[NONE, -2]] * len(qs)
    qs = [query(TOY, nat.MODE_GRAD, b, grad_out=False) for b in (64, 256)]                # refused by the validation
    assert picks(qs) == [[NONE, -1]] * len(qs)
    # the same calls with an instance behind them
    assert picks([query((2, 15, 5, 1), nat.MODE_ADAM, 256), query((2, 10, 3, 1), nat.MODE_ADAM, 256),
                  query(TOY, nat.MODE_GRAD, 256)]) == [[[1, 4, 1, PLAIN], 0]] * 3


@pytest.mark.parametrize("mode", [5, -1])
def test_a_mode_outside_the_enum_answers_zero(native, mode):
    qs = [query(TOY, mode, b, groups=1) for b in (64, 128, 256)]
    assert picks(qs) == [[NONE, -1]] * 3


if __name__ == "__main__":
    from distributed_training_pytorch_amd import _native as _nat

    with open(sys.argv[1]) as _fh:
        _qs = json.load(_fh)
    _lib = _nat.load()
    with open(sys.argv[2], "w") as _fh:
        json.dump([pick(_lib, _nat, q) for q in _qs], _fh)

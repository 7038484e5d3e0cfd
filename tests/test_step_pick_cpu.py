"""The fused step's dispatcher on the CPU: ``dtp_mlp_train_lanes`` validates a ``TrainArgs`` and
resolves the kernel instance a train engine would launch -- host code of ``csrc/mlp_train.hip``
over the tables of ``csrc/mlp_train_one.hip`` and ``csrc/mlp_train_lanes.hip`` -- without a
launch.  The argument block is filled by hand as ``FusedTrainer`` fills it; no pointer in it is
dereferenced, so one dummy address stands for every buffer.

Asserted: for every cell of ``step_cases`` the (lanes, waves, groups) its GPU matrix expects;
0 for instances that do not exist; 0 for a mode outside ``DtpMode``.  The environment
variables that force an instance are read once per process, so the cells that set one run in a
child process per value (``python -m tests.test_step_pick_cpu QUERIES.json OUT.json``)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCING = ("DTP_LANES", "DTP_FAST", "DTP_GRP_NW", "DTP_GROUPS")
DUMMY = 0x1000
TOY = (2, 10, 5, 1)


def query(shape=TOY, mode=1, batch=256, n=512, world=1, loss=0, bf16=0, groups=0, cache=1, slope=0.01,
          grad_out=True) -> dict:
    return dict(shape=list(shape), mode=mode, batch=batch, n=n, world=world, loss=loss, bf16=bf16, groups=groups,
                cache=cache, slope=slope, grad_out=grad_out)


def pick(lib, nat, q: dict) -> list:
    """[lanes, waves, groups] of the step for query q ([0, 0, 0]: refused or no instance)."""
    a = nat.TrainArgs()
    for f in ("X", "Y", "params", "opt_m", "opt_v", "step", "status", "peers", "epoch"):
        setattr(a, f, DUMMY)
    if q["grad_out"]:
        a.grad_out = DUMMY
    a.n_models, a.n_steps, a.host_t0 = 2, 1, 0
    a.loss, a.cache_data, a.bf16, a.groups = q["loss"], q["cache"], q["bf16"], q["groups"]
    a.hp.slope = q["slope"]
    s = a.smp
    s.mode, s.perm, s.perm_epochs = nat.SAMPLER_TABLE, DUMMY, 4
    s.n, s.world, s.rank, s.batch = q["n"], q["world"], 0, q["batch"]
    s.num_samples = -(-q["n"] // q["world"])
    s.steps_per_epoch = -(-s.num_samples // q["batch"])
    r = lib.dtp_mlp_train_lanes(ctypes.byref(a), *q["shape"], q["mode"])
    return [r & 255, (r >> 8) & 255, r >> 16]


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


def test_every_cell_gets_the_instance_its_matrix_expects(native):
    from . import step_cases as sc

    cells = sc.ALL_CELLS + sc.ALL_XGMI
    wrong = []
    for env in sorted({c.env for c in cells}):
        group = [c for c in cells if c.env == env]
        got = picks([_cell_query(native, c) for c in group], env)
        wrong += [(c.id, g, c.expect) for c, g in zip(group, got) if tuple(g) != c.expect]
    assert not wrong, wrong


def test_absent_instances_answer_zero(native):
    nat = native
    qs = [query((2, 15, 5, 4), nat.MODE_ADAM, b) for b in (64, 128, 256)]                 # a shape outside the lists
    qs += [query((2, 10, 3, 1), nat.MODE_ADAM, b, bf16=1) for b in (64, 128, 256)]        # no bf16 instance
    qs += [query(TOY, nat.MODE_GRAD, b, grad_out=False) for b in (64, 256)]               # refused by the validation
    assert picks(qs) == [[0, 0, 0]] * len(qs)
    # the same calls with an instance behind them
    assert picks([query((2, 15, 5, 1), nat.MODE_ADAM, 256), query((2, 10, 3, 1), nat.MODE_ADAM, 256),
                  query(TOY, nat.MODE_GRAD, 256)]) == [[1, 4, 1]] * 3


@pytest.mark.parametrize("mode", [5, -1])
def test_a_mode_outside_the_enum_answers_zero(native, mode):
    qs = [query(TOY, mode, b, groups=1) for b in (64, 128, 256)]
    assert picks(qs) == [[0, 0, 0]] * 3


if __name__ == "__main__":
    from distributed_training_pytorch_amd import _native as _nat

    with open(sys.argv[1]) as _fh:
        _qs = json.load(_fh)
    _lib = _nat.load()
    with open(sys.argv[2], "w") as _fh:
        json.dump([pick(_lib, _nat, q) for q in _qs], _fh)

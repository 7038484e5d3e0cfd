"""The layer-split engines' host code on the CPU: the shape table (``dtp_split_shape_id``,
``dtp_split_stage_supported``), the buffer sizes (``dtp_split_link_bytes``,
``dtp_split_lanes_grp_bytes``) and every refusal of the two launch checks (``dtp_split_launch``:
one workgroup per stage, ``dtp_split_lanes_launch``: M member workgroups per stage) with its
return code and its ``dtp_last_error()`` text.

The launch block is filled by hand; validation only tests its pointers for null, so one dummy
address stands for every buffer.  :func:`block` alone would PASS validation and reach a kernel
launch, so it is never handed to a launch function as it is: every case breaks exactly one field
of it, and :func:`refusal` asserts a non-zero code for every call it makes."""
import ctypes
import itertools

import pytest

from .split_cases import SHAPES

DUMMY = 0x1000
WHOLE, FIRST1, MID2, LAST1 = 0, 1, 6, 8  # shape ids: the whole model, a first, a middle and a last stage
POINTERS = ("X", "Y", "params", "opt_m", "opt_v", "step", "loss_log", "status", "act_in", "act_out", "grad_in",
            "grad_out", "dp_peers", "grp_buf")


@pytest.fixture(scope="module")
def native():
    from distributed_training_pytorch_amd import _native as nat

    try:
        nat.load()
    except nat.NativeUnavailable as e:
        pytest.skip(f"native library not built: {e}")
    return nat


def block(nat, shape: int, members: int, n: int = 1):
    """A launch block of ``n`` stages of one shape that both checks accept: never launched as is."""
    L = nat.SplitLaunch()
    L.n, L.members = n, members
    for i in range(n):
        L.shape_id[i] = shape
        a = L.stage[i]
        for f in POINTERS:
            setattr(a, f, DUMMY)
        a.loss_log_cap, a.n_steps, a.optim, a.dp_world, a.dp_rank = 16, 1, nat.MODE_ADAM, 1, 0
        s = a.smp
        s.mode, s.perm, s.perm_epochs = nat.SAMPLER_TABLE, DUMMY, 4
        s.n, s.world, s.rank, s.batch, s.num_samples, s.steps_per_epoch = 512, 1, 0, 64, 512, 8
    return L


def _set(obj, path: str, value):
    *head, leaf = path.split(".")
    for name in head:
        obj = getattr(obj, name)
    setattr(obj, leaf, value)


def refusal(nat, engine: str, shape: int, members: int, n: int, breaks: dict):
    """(return code, message) of the launch check for the block with ``breaks`` applied: paths
    from the block (``n``, ``members``, ``shape_id``) or from stage ``n - 1`` (everything else)."""
    assert breaks, "an unbroken block would be launched"
    lib = nat.load()
    L = block(nat, shape, members, n)
    for path, value in breaks.items():
        if path in ("n", "members"):
            setattr(L, path, value)
        elif path == "shape_id":
            L.shape_id[n - 1] = value
        else:
            _set(L.stage[n - 1], path, value)
    fn = lib.dtp_split_launch if engine == "one" else lib.dtp_split_lanes_launch
    rc = fn(ctypes.byref(L), None)
    assert rc != 0, f"{engine} {breaks}: the check passed a block meant to be refused"
    return rc, (lib.dtp_last_error() or b"").decode()


def _case(engine, name, shape, breaks, msg, rc=-1, members=1, n=1):
    return pytest.param(engine, shape, members, n, breaks, rc, msg, id=f"{engine}-{name}")


def _shared(engine: str, pre: str) -> list:
    """The refusals both engines have, from one check; ``pre``: the engine's message prefix."""
    dp = f"{pre}: the cross-rank exchange serves ranks x members <= 8 with a peer table"
    c = []
    for f in ("params", "opt_m", "step", "status"):
        c.append(_case(engine, f"no-{f}", WHOLE, {f: None}, f"{pre}: missing buffers"))
    c += [
        _case(engine, "n_steps-0", WHOLE, {"n_steps": 0}, f"{pre}: n_steps must be positive"),
        _case(engine, "optim-grad", WHOLE, {"optim": 0}, f"{pre}: adam or sgd"),
        _case(engine, "optim-7", WHOLE, {"optim": 7}, f"{pre}: adam or sgd"),
        _case(engine, "adam-no-opt_v", WHOLE, {"opt_v": None}, f"{pre}: Adam needs opt_v"),
        _case(engine, "first-no-X", FIRST1, {"X": None}, f"{pre}: the first stage needs the inputs"),
        _case(engine, "whole-no-X", WHOLE, {"X": None}, f"{pre}: the first stage needs the inputs"),
        _case(engine, "last-no-Y", LAST1, {"Y": None}, f"{pre}: the last stage needs the targets"),
        _case(engine, "whole-no-Y", WHOLE, {"Y": None}, f"{pre}: the last stage needs the targets"),
        _case(engine, "mid-no-act_in", MID2, {"act_in": None}, f"{pre}: missing links to the previous stage"),
        _case(engine, "mid-no-grad_out", MID2, {"grad_out": None}, f"{pre}: missing links to the previous stage"),
        _case(engine, "last-no-act_in", LAST1, {"act_in": None}, f"{pre}: missing links to the previous stage"),
        _case(engine, "mid-no-act_out", MID2, {"act_out": None}, f"{pre}: missing links to the next stage"),
        _case(engine, "mid-no-grad_in", MID2, {"grad_in": None}, f"{pre}: missing links to the next stage"),
        _case(engine, "first-no-grad_in", FIRST1, {"grad_in": None}, f"{pre}: missing links to the next stage"),
        _case(engine, "dp-no-peers", WHOLE, {"dp_world": 2, "dp_peers": None}, dp),
        _case(engine, "dp-world-9", WHOLE, {"dp_world": 9}, dp),
        _case(engine, "dp-rank-neg", WHOLE, {"dp_world": 2, "dp_rank": -1}, dp),
        _case(engine, "dp-rank-world", WHOLE, {"dp_world": 2, "dp_rank": 2}, dp),
        _case(engine, "loss_log_cap-0", WHOLE, {"loss_log_cap": 0}, f"{pre}: loss_log_cap"),
        _case(engine, "last-loss_log_cap-neg", LAST1, {"loss_log_cap": -1}, f"{pre}: loss_log_cap"),
    ]
    return c


ONE_BATCH = "split stage: batch must be 1..256 samples (one lane each) with a device sampler"
LANES_DP = "split lanes: the cross-rank exchange serves ranks x members <= 8 with a peer table"
LANES_RING = "split lanes: the gathering stages read the device permutation ring (SAMPLER_TABLE)"
LANES_64 = "split lanes: batch / members must be <= 64"

CASES = [
    # ---- one workgroup per stage
    _case("one", "n-0", WHOLE, {"n": 0}, "split launch: 1..8 stages per GPU"),
    _case("one", "n-9", WHOLE, {"n": 9}, "split launch: 1..8 stages per GPU"),
    _case("one", "shape-neg", WHOLE, {"shape_id": -1}, "split launch: stage shape not instantiated", rc=-2),
    _case("one", "shape-12", WHOLE, {"shape_id": len(SHAPES)}, "split launch: stage shape not instantiated", rc=-2),
    _case("one", "shape-12-second", WHOLE, {"shape_id": len(SHAPES)}, "split launch: stage shape not instantiated",
          rc=-2, n=2),
    *_shared("one", "split stage"),
    _case("one", "batch-0", WHOLE, {"smp.batch": 0}, ONE_BATCH),
    _case("one", "batch-257", WHOLE, {"smp.batch": 257}, ONE_BATCH),
    _case("one", "sampler-explicit", WHOLE, {"smp.mode": 0}, ONE_BATCH),
    _case("one", "mid-sampler-explicit", MID2, {"smp.mode": 0}, ONE_BATCH),
    _case("one", "n_steps-differ", MID2, {"n_steps": 2}, "split launch: stages disagree on n_steps", n=2),
    # ---- M member workgroups per stage
    _case("lanes", "n-0", WHOLE, {"n": 0}, "split lanes: 1..8 stages per GPU"),
    _case("lanes", "n-9", WHOLE, {"n": 9}, "split lanes: 1..8 stages per GPU"),
    _case("lanes", "members-0", WHOLE, {"members": 0}, "split lanes: 1..8 members per stage"),
    _case("lanes", "members-9", WHOLE, {"members": 9}, "split lanes: 1..8 members per stage"),
    _case("lanes", "shape-neg", WHOLE, {"shape_id": -1}, "split lanes: stage shape not instantiated", rc=-2),
    _case("lanes", "shape-12", WHOLE, {"shape_id": len(SHAPES)}, "split lanes: stage shape not instantiated", rc=-2),
    _case("lanes", "shape-12-second", WHOLE, {"shape_id": len(SHAPES)}, "split lanes: stage shape not instantiated",
          rc=-2, n=2),
    *_shared("lanes", "split lanes"),
    _case("lanes", "n_steps-differ", MID2, {"n_steps": 2}, "split lanes: n_steps", n=2),
    _case("lanes", "batch-0", WHOLE, {"smp.batch": 0}, LANES_64),
    _case("lanes", "batch-65-m1", WHOLE, {"smp.batch": 65}, LANES_64),
    _case("lanes", "batch-129-m2", WHOLE, {"smp.batch": 129}, LANES_64, members=2),
    _case("lanes", "batch-513-m8", WHOLE, {"smp.batch": 513}, LANES_64, members=8),
    _case("lanes", "m4-batch-3", WHOLE, {"smp.batch": 3}, "split lanes: at most one member per sample", members=4),
    _case("lanes", "sampler-shuffle", WHOLE, {"smp.mode": 1}, LANES_RING),
    _case("lanes", "first-sampler-explicit", FIRST1, {"smp.mode": 0}, LANES_RING),
    _case("lanes", "last-no-perm", LAST1, {"smp.perm": None}, LANES_RING),
    _case("lanes", "perm_epochs-0", WHOLE, {"smp.perm_epochs": 0}, LANES_RING),
    _case("lanes", "perm_epochs-3", WHOLE, {"smp.perm_epochs": 3}, LANES_RING),
    _case("lanes", "whole-n-1366", WHOLE, {"smp.n": 1366}, "split lanes: dataset exceeds the LDS cache"),
    _case("lanes", "first-n-2049", FIRST1, {"smp.n": 2049}, "split lanes: dataset exceeds the LDS cache"),
    _case("lanes", "last-n-4097", LAST1, {"smp.n": 4097}, "split lanes: dataset exceeds the LDS cache"),
    _case("lanes", "dp2-m5", WHOLE, {"dp_world": 2}, LANES_DP, members=5),
    _case("lanes", "dp3-m3", WHOLE, {"dp_world": 3}, LANES_DP, members=3),
    _case("lanes", "m2-no-grp_buf", WHOLE, {"grp_buf": None},
          "split lanes: members > 1 need the member exchange buffer", members=2),
]


@pytest.mark.parametrize("engine,shape,members,n,breaks,rc,msg", CASES)
def test_launch_refuses(native, engine, shape, members, n, breaks, rc, msg):
    assert refusal(native, engine, shape, members, n, breaks) == (rc, msg)


@pytest.mark.parametrize("fn", ["dtp_split_launch", "dtp_split_lanes_launch"])
def test_launch_refuses_a_null_block(native, fn):
    lib = native.load()
    assert getattr(lib, fn)(None, None) == -1
    pre = "split launch" if fn == "dtp_split_launch" else "split lanes"
    assert (lib.dtp_last_error() or b"").decode() == f"{pre}: 1..8 stages per GPU"


GRID = list(itertools.product((1, 2, 10, 11), (9, 10), range(7), (1, 2, 10), (0, 1), (0, 1)))


def test_shape_id_is_the_row_index(native):
    lib = native.load()
    rows = {(i, h, nl, o, int(f), int(fi)): k for k, (i, h, nl, o, f, fi) in enumerate(SHAPES)}
    assert len(rows) == len(SHAPES) == 12
    wrong = [(q, got) for q in GRID if (got := lib.dtp_split_shape_id(*q)) != rows.get(q, -1)]
    assert not wrong, wrong[:8]
    assert sum(q in rows for q in GRID) == len(SHAPES)  # the grid holds every row


def test_supported_is_an_id(native):
    lib = native.load()
    wrong = [q for q in GRID if lib.dtp_split_stage_supported(*q) != int(lib.dtp_split_shape_id(*q) >= 0)]
    assert not wrong, wrong[:8]


@pytest.mark.parametrize("width,batch", [(10, 256), (10, 1), (1, 200), (2, 64), (3, 7), (9, 130)])
def test_link_bytes(native, width, batch):
    assert native.load().dtp_split_link_bytes(width, batch) == batch * ((width + 1) // 2) * 16


@pytest.mark.parametrize("P,members", [(481, 4), (481, 1), (30, 8), (121, 2), (256, 3), (257, 3), (11, 5)])
def test_lanes_grp_bytes(native, P, members):
    npt = (P + 255) // 256                      # parameters per thread of a 256-thread member
    nthr = (P + npt - 1) // npt                 # threads that own some
    slot16 = (nthr * ((npt + 1) // 2) + 1 + 3) & ~3  # their granules and the loss's, rounded to 64 bytes
    assert native.load().dtp_split_lanes_grp_bytes(P, members) == 2 * members * slot16 * 16

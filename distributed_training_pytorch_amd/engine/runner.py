"""The demo training loop shared by demo.py and demo_assume_started_with_mpiexec.py.

Reference: ``demo.py:19-137`` / ``demo_assume_started_with_mpiexec.py:29-127``:
two ToyModels (X, Y) trained on ToyData with DDP + Adam + MSE for 1000
iterations, the global mean loss of each model reduced every iteration and
logged by rank 0 (``loss/lossX``, ``loss/lossY``), tqdm on rank 0, rank-prefixed
status prints.

Engines (``--engine``):
* ``fused``  -- FusedTrainer: the whole iteration in one kernel (or one persistent
                kernel for many iterations); gradient all-reduce in-kernel over
                xGMI or through RCCL; losses read lazily from a device ring.
* ``module`` -- nn.Module path: ModelBank (both models in one flat buffer) with fused
                per-op kernels, FlatDDP (bucketed RCCL all-reduce overlapped with
                backward), FlatOptimizer (one Adam launch for both models).
* ``stock``  -- plain PyTorch eager DDP, the reference loop verbatim (baseline).
"""
from __future__ import annotations

import contextlib
import datetime
import os
import socket
import time

import torch
import torch.distributed as dist

from ..data.sampler import BatchIndexer, SamplerGeometry
from ..data.toy_data import ToyData
from ..ops.gather import gather_rows2, gather_rows2_ring, gather_rows2_sampler, ring_gather_ok
from ..ops.loss import MSELoss
from ..ops.mlp import ParamBackwardFusion
from ..ops.optim import OptimConfig
from ..parallel import comm_util
from ..runtime import bootstrap, checkpoint
from ..runtime.errors import FaultInjector, check_replicas
from ..utils.logging import LossRing, MetricLogger, rank_print
from ..utils.profiling import PhaseTimer
from ..utils.profiling import enabled as trace_enabled


def setup(config, launcher: str | None = None, gpus_per_proc: int = 1):
    """Discover ranks, bind the device, init the process group, print the reference's status lines."""
    bootstrap.configure_collective_env()
    if launcher == "mpi":
        env = bootstrap.detect(torchrun=False)
        if env.launcher == "single" and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise RuntimeError("expected an MPI launch (OMPI_/PMI_ rank variables not found)")
    else:
        env = bootstrap.detect(torchrun=True if config.torchrun else None, use_node_rank=config.use_node_rank)
    device = bootstrap.bind_device(env, config.device, gpus_per_proc)
    backend = config.backend
    if device.type == "cpu" and backend == "nccl":
        backend = "gloo"
    bootstrap.init_process_group(env, backend, device, datetime.timedelta(minutes=config.timeout_min))
    rank, world = dist.get_rank(), dist.get_world_size()
    # the reference draws --seed independently in every process (argument_parser.py:17)
    # and never applies it; here rank 0's seed is broadcast so the data and model init
    # agree across ranks, and each worker gets seed + rank for its own randomness
    seed_t = torch.tensor([config.seed], dtype=torch.int64)
    comm_util.broadcast_(seed_t, 0)
    config.seed = int(seed_t.item())
    if rank == 0:
        rank_print(rank, f"World_size: {world}")
    rank_print(rank, f"Hello from {socket.gethostname()}")
    if env.local_rank == 0:
        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
        rank_print(rank, f"Available devices on machine: {n}")
    base_seed = config.seed
    worker_seed = base_seed + rank
    rank_print(rank, f"Base seed: {base_seed} and  worker seed: {worker_seed}")
    torch.manual_seed(worker_seed)
    rank_print(rank, f"Using torchrun: {config.torchrun}")
    rank_print(rank, f"Using backend: {dist.get_backend()}")
    rank_print(rank, f"Launcher: {env.launcher}; device: {device}")
    return env, device, rank, world


def _dataset(config, rank):
    return ToyData(n=config.n_samples, seed=config.seed, rank=rank, per_rank=config.per_rank_data,
                   classes=4 if config.loss == "ce" else 0)


def _geom(config, rank, world):
    return SamplerGeometry(n=config.n_samples, world=world, rank=rank, batch=config.batch_size,
                           shuffle=True, distributed=config.dataloader == "distributed", seed=0)


def _compute_dtype(config) -> torch.dtype:
    return torch.bfloat16 if getattr(config, "precision", "fp32") == "bf16" else torch.float32


def _fused_supported(config) -> bool:
    from .. import _native as nat
    from ..ops.mlp import MlpSpec

    spec = MlpSpec(2, config.hidden, config.depth + 2, 4 if config.loss == "ce" else 1)
    if _compute_dtype(config) == torch.bfloat16:
        try:
            return bool(nat.load().dtp_mlp_train_bf16_supported(*spec.key[:4]))
        except nat.NativeUnavailable:
            return False
    return spec.native_supported()


def _optim(config) -> OptimConfig:
    return OptimConfig(config.optimizer, config.lr, momentum=config.momentum, weight_decay=config.weight_decay,
                       max_grad_norm=_clip_norm(config), clip_grad_value=_clip_value(config),
                       schedule=lr_schedule(config))


def lr_schedule(config):
    """The ``LrSchedule`` of --lr_schedule / --warmup_iters / --lr_decay_iters / --lr_min_ratio /
    --lr_step_size / --lr_gamma; None with the defaults (the fixed --lr, no table at all).
    A function of the step number alone, so --resume with the same flags continues the curve."""
    from ..ops.schedule import LrSchedule

    kind = getattr(config, "lr_schedule", "constant") or "constant"
    warm = int(getattr(config, "warmup_iters", 0) or 0)
    if kind == "constant" and warm <= 0:
        return None
    decay = getattr(config, "lr_decay_iters", None)
    return LrSchedule.make(kind, config.lr, warmup_iters=warm,
                           decay_iters=config.iters if decay is None else decay,
                           min_ratio=getattr(config, "lr_min_ratio", 0.0),
                           step_size=getattr(config, "lr_step_size", None),
                           gamma=getattr(config, "lr_gamma", 0.1), total=max(int(config.iters), 1))


def _lr_summary(config, iters: int) -> dict:
    """``lr_schedule`` and ``lr_last`` (the rate of the last step taken) of the run summary."""
    sched = lr_schedule(config)
    last = float(config.lr) if sched is None or iters <= 0 else sched.lr(iters - 1)
    return {"lr_schedule": getattr(config, "lr_schedule", "constant"), "lr_last": last}


def _clip_norm(config) -> float:
    return max(float(getattr(config, "clip_grad_norm", 0.0) or 0.0), 0.0)


def _accumulate(config) -> int:
    a = int(getattr(config, "accumulate_grad_batches", 1) or 1)
    if a < 1:
        raise SystemExit("--accumulate_grad_batches must be >= 1")
    return a


def _clip_value(config) -> float:
    return max(float(getattr(config, "clip_grad_value", 0.0) or 0.0), 0.0)


class _Validation:
    """``--eval_every K``: the held-out set, when it is due, and rank 0's ``val/*`` rows.

    The set is ``train.held_out(--val_samples, seed + 1)`` of the SHARED training set (the
    same rows and, with ``--loss ce``, the same label edges on every rank even with
    ``--per_rank_data``); rank r evaluates rows ``r::world`` of it."""

    def __init__(self, config, train_ds, rank, world, device, logger):
        self.every = max(int(getattr(config, "eval_every", 0) or 0), 0)
        self.iters, self.rank, self.world, self.logger = config.iters, rank, world, logger
        self.ce = config.loss == "ce"
        self.last: dict | None = None
        self.X = self.Y = None
        if self.every:
            if config.per_rank_data:
                train_ds = ToyData(n=config.n_samples, seed=config.seed, classes=train_ds.classes)
            held = train_ds.held_out(int(config.val_samples), config.seed + 1)
            self.X, self.Y = held.device_tensors(device)

    def due(self, done: int) -> bool:
        """After ``done`` iterations: every K-th, and the last one."""
        return bool(self.every) and done > 0 and (done % self.every == 0 or done == self.iters)

    def to_next(self, done: int) -> int:
        """Iterations from ``done`` to the next evaluation point (launch chunks are cut there)."""
        return self.every - done % self.every if self.every else 1 << 62

    def sums_torch(self, forward) -> tuple[torch.Tensor, int]:
        """This rank's shard through ``forward(x) -> outputs per model`` and torch's loss: the
        sums of ``ops.eval.evaluate`` (fp32 per-sample values added in fp64)."""
        x, y = self.X[self.rank::self.world].contiguous(), self.Y[self.rank::self.world].contiguous()
        n = x.shape[0]
        with torch.no_grad():
            outs = forward(x) if n else []
            sums = torch.zeros(2, 2, dtype=torch.float64, device=self.X.device)
            for i, o in enumerate(outs):
                o = o.float()
                if self.ce:
                    cls = y.view(-1).long()
                    sums[i, 0] = torch.nn.functional.cross_entropy(o, cls, reduction="none").double().sum()
                    sums[i, 1] = (o.argmax(1) == cls).sum().double()
                else:
                    sums[i, 0] = ((o - y.view_as(o)) ** 2).sum(1).double().sum()
        return sums, n

    def reduce(self, sums: torch.Tensor, n: int, out_features: int) -> dict:
        """One all-reduce of the sums and the count -> the dict of ``FusedTrainer.evaluate``."""
        from ..ops.eval import EvalResult

        buf = torch.cat([sums.reshape(-1), torch.tensor([float(n)], dtype=torch.float64, device=sums.device)])
        host = comm_util.all_reduce_(buf).cpu()
        res = EvalResult(host[:-1].view(-1, 2), int(host[-1].item()), out_features, "ce" if self.ce else "mse")
        return {"loss": res.mean_loss, "accuracy": res.accuracy, "count": res.count}

    def report(self, done: int, res: dict) -> None:
        self.last = res
        row = {"val/lossX": float(res["loss"][0]), "val/lossY": float(res["loss"][1])}
        if res["accuracy"] is not None:
            row.update({"val/accX": float(res["accuracy"][0]), "val/accY": float(res["accuracy"][1])})
        self.logger.log(row, step=done)

    def summary(self) -> dict:
        if self.last is None:
            return {}
        out = {"val_loss": [float(v) for v in self.last["loss"]]}
        if self.last["accuracy"] is not None:
            out["val_acc"] = [float(v) for v in self.last["accuracy"]]
        return out


def _progress(rank, total, config):
    if rank != 0 or config.no_progress:
        return None
    try:
        from tqdm import tqdm

        return tqdm(total=total, desc="Iteration")
    except ImportError:  # pragma: no cover
        return None


def train(config, env, device, rank, world, group: str = "base-demo") -> dict:
    logger = MetricLogger(project=config.project, group=group, log_dir=config.log_dir, rank=rank,
                          config={k: v for k, v in vars(config).items() if isinstance(v, (int, float, str, bool))})
    faults = FaultInjector(config.fail_at_iter, config.fail_rank, rank)
    t_start = time.perf_counter()
    engine = config.engine
    if engine == "fused" and device.type == "cuda" and not _fused_supported(config):
        # widths / dtypes the fused step kernel is not instantiated for train through
        # nn.Modules whose Linears run on the MFMA GEMM (FlatDDP + FlatOptimizer)
        rank_print(rank, f"fused step kernel has no instance for hidden={config.hidden} depth={config.depth} "
                         f"precision={config.precision}: using the module engine (MFMA GEMM layers)")
        engine = "module"
    if engine == "fused" and device.type != "cuda" and (_clip_norm(config) > 0 or _clip_value(config) > 0):
        # on a GPU the fused step clips in its kernel (the clip twins, csrc/clip_core.h); a CPU
        # run keeps taking the module engine, whose flat optimizer clips
        rank_print(rank, "gradient clipping (--clip_grad_norm / --clip_grad_value) is not in the fused step "
                         "kernel: using the module engine")
        engine = "module"
    summary = None
    if engine == "fused":
        summary = _train_fused(config, device, rank, world, logger, faults)
        if summary is None:
            # the fused step accumulates in its several-lanes / split-batch kernel
            # (csrc/accum_core.h); this run's pick -- the one-lane kernel -- has no such twin
            rank_print(rank, f"--accumulate_grad_batches {_accumulate(config)}: the fused step instance of this run "
                             "has no accumulation twin: using the module engine")
            engine = "module"
    if summary is not None:
        pass
    elif engine == "module":
        summary = _train_module(config, device, rank, world, logger, faults)
    else:
        summary = _train_stock(config, device, rank, world, logger, faults)
    wall = time.perf_counter() - t_start
    logger.finish()
    summary["wall_s"] = wall
    # what ran: the stock loop keeps the reference's verbatim Adam(lr=1e-3) pair unless the run
    # asks for AdamW (it ignores --optimizer sgd, --lr and --weight_decay otherwise)
    summary["optimizer"] = "adam" if summary.get("engine") == "stock" and config.optimizer != "adamw" \
        else _optim(config).label
    summary.update(_lr_summary(config, int(summary.get("iters", 0))))
    rank_print(rank, "Finished")
    return summary


# ----------------------------------------------------------------------------- fused engine
def _train_fused(config, device, rank, world, logger, faults) -> dict:
    from ..engine.fused_trainer import EngineConfig, FusedTrainer
    from ..models.toy import ToyModel
    from ..ops.mlp import MlpSpec

    ds = _dataset(config, rank)
    X, Y = ds.device_tensors(device)
    geom = _geom(config, rank, world)
    torch.manual_seed(config.seed)
    out_f = 4 if config.loss == "ce" else 1
    spec = MlpSpec(2, config.hidden, config.depth + 2, out_f)
    init = [ToyModel(hidden=config.hidden, depth=config.depth, out_features=out_f).flat_params.detach().clone()
            for _ in range(2)]
    ecfg = EngineConfig(comm=config.comm, launch=config.launch, steps_per_launch=config.steps_per_launch,
                        sampler=config.sampler, loss=config.loss, precision=config.precision,
                        accumulate=_accumulate(config))
    tr = FusedTrainer(spec, 2, X, Y, geom, _optim(config), ecfg, init_params=init)
    if tr.A > 1 and tr.native and tr.comm not in ("rccl", "host") and tr.lanes == 0:
        tr.close()  # no accumulation twin for this pick (the same on every rank): the caller falls back
        return None
    start = 0
    if config.resume and config.checkpoint_dir:
        st = checkpoint.load(config.checkpoint_dir)
        if st is not None:
            if st.get("engine", "fused") != "fused":
                raise RuntimeError(f"{config.checkpoint_dir} holds a {st['engine']!r}-engine checkpoint; "
                                   "resume it with the same engine")
            tr.load_state_dict(st)
            start = tr.t
            rank_print(rank, f"resumed from {config.checkpoint_dir} at iteration {start}")
    rank_print(rank, f"engine: fused ({tr.comm} comm, {config.launch} launch)")
    pbar = _progress(rank, config.iters, config)
    if pbar is not None and start:
        pbar.update(start)
    it = start
    chunk = max(1, min(config.log_every, config.steps_per_launch))
    timer = PhaseTimer(device)
    val = _Validation(config, ds, rank, world, device, logger)

    def ckpt_due(i):
        return bool(config.checkpoint_dir and config.checkpoint_every and i % config.checkpoint_every == 0)

    # Chunks are pipelined: chunk k+1 is queued on the GPU before the host logs chunk
    # k, whose losses (and the xGMI status word) were copied to pinned memory behind
    # it, so logging overlaps the next chunk instead of idling the GPU.
    pending = None

    def process(p):
        it0, n, handle = p
        with timer.phase("loss_readback"):
            ls = handle.wait_tensor()  # raises on a sticky xGMI timeout: never train on partial sums
        logger.log_rows(list(range(it0, it0 + n)), ["loss/lossX", "loss/lossY"], ls[:n])
        if pbar is not None:
            pbar.update(n)

    t0 = time.perf_counter()
    while it < config.iters:
        n = min(chunk, config.iters - it)
        if faults.armed() and it <= config.fail_at_iter < it + n:
            n = config.fail_at_iter - it
        n = min(n, val.to_next(it))  # launches are cut at the evaluation points
        val_due = n > 0 and val.due(it + n)
        if n > 0:
            with timer.phase("train_chunk"):
                tr.train(n)
            handle = tr.losses_async(it, it + n)
            if pending is not None:
                process(pending)
            pending = (it, n, handle)
            it += n
        if pending is not None and (it >= config.iters or ckpt_due(it) or val_due or
                                    (faults.armed() and it >= config.fail_at_iter)):
            process(pending)
            pending = None
        if val_due:
            # stream-ordered behind the chunk just queued; its loss rows are logged (above)
            # before the val/* row of step `it`
            with timer.phase("validation"):
                val.report(it, tr.evaluate(val.X, val.Y))
        faults.check(it)
        if ckpt_due(it):
            tr.synchronize()
            checkpoint.save({**tr.state_dict(), "engine": "fused", "config": vars(config)},
                            config.checkpoint_dir, it)
            # the other ranks wait for rank 0's write on the host (process-group
            # timeout), not inside the next launch's first in-kernel xGMI exchange,
            # whose bounded spin a slow checkpoint filesystem could outlast
            comm_util.barrier()
    if pending is not None:
        process(pending)
    tr.synchronize()
    dt = time.perf_counter() - t0
    if pbar is not None:
        pbar.close()
    if config.check_replicas:
        check_replicas(tr.params)
    if config.checkpoint_dir:
        checkpoint.save({**tr.state_dict(), "engine": "fused", "config": vars(config)}, config.checkpoint_dir, it)
    final = tr.losses(it - 1, it)[0].tolist() if it > 0 else [float("nan")] * 2
    samples = geom.batch * (it - start) * world * tr.A
    # clipping by norm: each model's gradient norm at the last step, before clipping
    gnorm = {"grad_norm": tr.grad_norm.tolist()} if tr.grad_norm is not None else {}
    tr.close()
    return {"final_loss": final, "iters": it, "samples_per_s": samples / max(dt, 1e-9), "engine": "fused",
            "accumulate_grad_batches": tr.A, **gnorm, **val.summary(),
            **({"phases": timer.summary()} if trace_enabled() else {})}


# ----------------------------------------------------------------------------- module engine
def _train_module(config, device, rank, world, logger, faults) -> dict:
    from ..models.bank import ModelBank
    from ..ops.optim import FlatOptimizer
    from ..parallel.ddp import FlatDDP

    ds = _dataset(config, rank)
    X, Y = ds.device_tensors(device)
    geom = _geom(config, rank, world)
    # batch indices on the device: the native sampler kernel, or the exact torch order
    # uploaded once per epoch (no per-step host index math or copies)
    indexer = BatchIndexer(geom, device, exact_torch=config.sampler == "torch")
    torch.manual_seed(config.seed)
    out_f = 4 if config.loss == "ce" else 1
    bank = ModelBank(2, hidden=config.hidden, depth=config.depth, out_features=out_f,
                     compute_dtype=_compute_dtype(config)).to(device)
    ddp = FlatDDP(bank, flat_params=bank.flat, flat_grad=bank.flat_grad,
                  comm=config.comm if config.comm in ("auto", "rccl", "xgmi") else "rccl")
    rank_print(rank, f"engine: module (FlatDDP over {ddp.comm})")
    from .graph_step import CapturedStep
    opt = FlatOptimizer(bank.flat, bank.flat_grad, _optim(config))
    lossf = torch.nn.CrossEntropyLoss() if config.loss == "ce" else MSELoss()  # fused drop-in (ops/loss.py)
    # gradient accumulation, the plain form: A micro-batches per optimizer step, each loss scaled
    # by 1/A through the backward seed, the first A - 1 backwards under ddp.no_sync(), one
    # flat-optimizer step; iteration `it` reads batches it A .. it A + A - 1
    A = _accumulate(config)
    start = 0
    if config.resume and config.checkpoint_dir:
        st = checkpoint.load(config.checkpoint_dir)
        if st is not None:
            if st.get("engine") != "module":
                raise RuntimeError(f"{config.checkpoint_dir} holds a {st.get('engine', 'fused')!r}-engine "
                                   "checkpoint; resume it with the same engine")
            if int(st.get("accumulate", 1)) != A:  # the data position is iteration * A
                raise ValueError(f"checkpoint taken with --accumulate_grad_batches {int(st.get('accumulate', 1))}, "
                                 f"this run has {A}")
            with torch.no_grad():
                bank.flat.copy_(st["params"].to(bank.flat.dtype))
            opt.load_state_dict(st["optim_state"])
            start = int(st["iteration"])
            rank_print(rank, f"resumed from {config.checkpoint_dir} at iteration {start}")

    def _save(it_done):
        checkpoint.save({"engine": "module", "params": bank.flat.detach(), "optim_state": opt.state_dict(),
                         "accumulate": A, "config": vars(config)}, config.checkpoint_dir, it_done)

    pbar = _progress(rank, config.iters, config)
    if pbar is not None and start:
        pbar.update(start)
    timer = PhaseTimer(device)
    val = _Validation(config, ds, rank, world, device, logger)
    val_native = device.type == "cuda" and bank.spec.native_supported(bf16=_compute_dtype(config) == torch.bfloat16)

    def _validate(done):
        # between graph replays, never inside one: the toy shapes in one launch of the
        # evaluation kernel over the bank's flat rows, wide models through the bank's forward
        if val_native:
            from ..ops.eval import evaluate as eval_sums, shard_rows

            n = shard_rows(val.X.shape[0], rank, world)
            sums = eval_sums(bank.flat.detach(), bank.spec, val.X, val.Y, loss=config.loss,
                             bf16=_compute_dtype(config) == torch.bfloat16, row0=rank, row_stride=world, n=n)
        else:
            sums, n = val.sums_torch(bank)
        val.report(done, val.reduce(sums, n, out_f))

    t0 = time.perf_counter()
    # per-step losses stay on the device; the global means are reduced and logged once
    # per log_every steps (one all-reduce of the chunk, one host sync), with the same
    # per-step values and keys as the reference's per-step gloo reduce + wandb.log
    ring = LossRing(max(1, config.log_every), 2, device, world)
    last = [float("nan")] * 2

    def _flush(wait: bool = True):
        nonlocal last
        # check the sticky xGMI timeout word at every log point (one host read, with
        # several ranks only), so a timed-out exchange stops the run there instead of
        # training on partial sums until the end
        ddp.check_comm()
        for step, (vx, vy) in ring.flush(wait):
            if rank == 0:
                logger.log({"loss/lossX": vx}, step=step, commit=False)
                logger.log({"loss/lossY": vy}, step=step)
            last = [vx, vy]

    # the batch indices of the current iteration, refreshed before each step (the
    # captured graph reads this static buffer)
    idx_static = torch.zeros(geom.batch, dtype=torch.int64, device=device)

    # the flat optimizer zeroes the gradient it consumed, so the next step's zero_grad fill
    # is skipped (reset whenever a capture is abandoned: its zeroing never ran)
    grads_clean = [False]
    xb = {}
    fuse_opt = world == 1 and A == 1 and os.environ.get("DTP_MODULE_FUSE_OPT", "1") != "0"
    seed = _Seeds(device)
    loss_log = os.environ.get("DTP_MODULE_LOSSLOG", "1") != "0"  # A/B: the separate ring put
    sync_flush = os.environ.get("DTP_MODULE_SYNC_FLUSH", "0") == "1"  # A/B: the blocking flush

    def step_body(size):
        with timer.phase("data"):
            if size not in xb:
                xb[size] = (torch.empty(size, X.shape[1], device=device), torch.empty(size, Y.shape[1], device=device))
            x, y = xb[size]
            if samp_cfg is not None:  # indices from the device sampler, step cursor advanced on the device
                gather_rows2_sampler(X, Y, samp_cfg, samp_cursor, x, y)
            elif epoch_ring is not None:  # indices from the device epoch ring, cursor advanced on the device
                gather_rows2_ring(X, Y, epoch_ring, geom.batch, geom.steps_per_epoch, x, y)
            else:
                gather_rows2(X, Y, idx_static[:size], x, y)  # both tensors in one launch
            if config.loss == "ce":
                y = y.view(-1).long()
        if not grads_clean[0]:
            bank.zero_grad()
        logged = False
        with timer.phase("forward"):
            ox, oy = ddp(x)  # both models' forwards in one launch (ModelBank.forward)
            if isinstance(lossf, MSELoss):
                # both losses, their sum and the loss-log row in one launch
                lx, ly, lsum = lossf.pair(ox, oy, y, log=ring.device_log() if loss_log else None)
                logged = loss_log
            else:
                lx, ly = lossf(ox, y), lossf(oy, y)
                lsum = lx + ly
        # one rank: both models' stage backwards and the flat Adam over both as ONE launch
        # (ParamBackwardFusion; nothing reads the gradient in between without an all-reduce)
        with (ParamBackwardFusion() if fuse_opt else contextlib.nullcontext()) as fus:
            with timer.phase("backward+allreduce"):
                # independent models: one backward, one bucketed all-reduce; the seed from a
                # cached tensor of ones (autograd's own is a fill launch per step)
                lsum.backward(seed.get(lsum.shape) if device.type == "cuda" else None)
            with timer.phase("optimizer"):
                grads_clean[0] = opt.step(zero_grad=True, fused=fus.take() if fus is not None else None)
        if not logged:
            ring.put_device(lx, ly)

    # accumulation: the indices of the window's micro-batches where the host uploads them
    idx_window = torch.zeros(A, geom.batch, dtype=torch.int64, device=device) if A > 1 else None

    def window_body(sizes):
        """One optimizer step over the window's micro-batches (``sizes``: their batch sizes)."""
        if not grads_clean[0]:
            bank.zero_grad()
        tx = ty = None
        for j, size in enumerate(sizes):
            with timer.phase("data"):
                if size not in xb:
                    xb[size] = (torch.empty(size, X.shape[1], device=device),
                                torch.empty(size, Y.shape[1], device=device))
                x, y = xb[size]
                if samp_cfg is not None:  # the device sampler's cursor advances per gather
                    gather_rows2_sampler(X, Y, samp_cfg, samp_cursor, x, y)
                else:
                    gather_rows2(X, Y, idx_window[j, :size], x, y)
                if config.loss == "ce":
                    y = y.view(-1).long()
            with timer.phase("forward"):
                ox, oy = ddp(x)
                if isinstance(lossf, MSELoss):
                    lx, ly, lsum = lossf.pair(ox, oy, y)
                else:
                    lx, ly = lossf(ox, y), lossf(oy, y)
                    lsum = lx + ly
            with timer.phase("backward+allreduce"):
                with (ddp.no_sync() if j < len(sizes) - 1 else contextlib.nullcontext()):
                    lsum.backward(seed.get(lsum.shape, 1.0 / A))  # d (sum_j loss_j / A) / d loss_j
            tx = lx.detach() if tx is None else tx + lx.detach()
            ty = ly.detach() if ty is None else ty + ly.detach()
        with timer.phase("optimizer"):
            grads_clean[0] = opt.step(zero_grad=True)
        ring.put_device(tx * (1.0 / A), ty * (1.0 / A))

    def _abort():
        grads_clean[0] = False
        ddp.reset_hooks()

    # hipGraph replay of the whole iteration (engine/graph_step.py) where it can be
    # captured: one rank, xGMI buckets (device-side exchange epochs) or RCCL buckets;
    # not gloo-staged buckets (host-driven)
    graphable = device.type == "cuda" and config.launch != "eager" and not trace_enabled() and ddp.graph_safe()
    if A > 1:
        # the window is captured whole where one rank runs it (nothing is reduced); with several
        # ranks its single reduction follows A - 1 held-back backwards: run eagerly
        graphable = graphable and world == 1
        rank_print(rank, f"accumulation window of {A} micro-batches: "
                         f"{'captured in one graph' if graphable else 'run eagerly'}")
    stepper = CapturedStep(step_body if A == 1 else window_body, device, enabled=graphable, on_abort=_abort)
    # the device epoch ring {cursor, the epoch's indices} of the replayed step's gather: one
    # fill per epoch instead of an index copy per step (DTP_MODULE_RING=0: the copies, A/B)
    # better still, the step's indices computed on the device by the engine's own sampler
    # (sampler.h, reading the device permutation ring for DistributedSampler's exact order):
    # no host index work per epoch either (DTP_MODULE_RING=epoch: the epoch ring, A/B)
    epoch_ring, ring_epoch = None, None
    samp_cfg, samp_cursor, perm_ring = None, None, None
    ring_mode = os.environ.get("DTP_MODULE_RING", "sampler")
    if graphable and ring_gather_ok(X, Y, geom.batch) and ring_mode == "sampler" and geom.batch <= 1024:
        perm_ring = indexer.permutation_ring()
        if perm_ring is not None or not indexer.needs_ring():
            samp_cfg = geom.to_native()
            if perm_ring is not None:
                perm_ring.native(samp_cfg)
            samp_cursor = torch.full((1,), start * A, dtype=torch.int64, device=device)
    if (samp_cfg is None and graphable and indexer.can_fill_epoch() and ring_gather_ok(X, Y, geom.batch)
            and ring_mode != "0" and A == 1):  # (a window can span two epochs: the one-epoch ring serves A = 1)
        epoch_ring = torch.zeros(1 + geom.steps_per_epoch * geom.batch, dtype=torch.int64, device=device)
        epoch_ring[0] = geom.batch_pos(start)[1] // geom.batch  # the cursor: the first step's batch in its epoch
    # steady-state clock (the summary's steady_samples_per_s): from the end of step
    # steady_from on -- the first kernels' code-object loads, the warm-up runs and the
    # graph captures fall before it (they are a fixed cost that dominates short runs and
    # varies by box); synchronised at both ends
    steady_from = start + min(50, (config.iters - start) // 2)
    t_steady = None
    for it in range(start, config.iters):
        if it == steady_from and device.type == "cuda":
            torch.cuda.synchronize(device)
            t_steady = time.perf_counter()
        faults.check(it)
        if A > 1:
            micro = range(it * A, it * A + A)
            sizes = tuple(geom.batch_size_at(u) for u in micro)
            if samp_cfg is not None:
                eps = (geom.batch_pos(micro[0])[0], geom.batch_pos(micro[-1])[0])
                if perm_ring is not None and eps != ring_epoch:  # resident before the replay that reads them
                    perm_ring.ensure(*eps)
                    ring_epoch = eps
            else:
                for j, u in enumerate(micro):
                    idx_window[j, :sizes[j]].copy_(indexer(u))
            stepper.run(sizes)
        size = geom.batch_size_at(it)
        if A > 1:
            pass
        elif samp_cfg is not None:
            ep = geom.batch_pos(it)[0]
            if perm_ring is not None and ep != ring_epoch:  # resident before the replay that reads it
                perm_ring.ensure(ep, ep)
                ring_epoch = ep
        elif epoch_ring is not None:
            ep = geom.batch_pos(it)[0]
            if ep != ring_epoch:  # stream-ordered after the last replay that read the old epoch
                indexer.epoch_into(ep, epoch_ring[1:1 + geom.num_samples])
                ring_epoch = ep
        else:
            idx_static[:size].copy_(indexer(it))
        if A == 1:
            stepper.run(size)
        ring.mark(it)
        if ring.full():
            with timer.phase("loss_reduce"):
                _flush(wait=sync_flush)  # no device sync: the rows are logged when they arrive
        if pbar is not None:
            pbar.update(1)
        if val.due(it + 1):
            _flush()  # the loss rows up to here first: the log stays in step order
            with timer.phase("validation"):
                _validate(it + 1)
        if config.checkpoint_dir and config.checkpoint_every and (it + 1) % config.checkpoint_every == 0:
            _flush()
            _save(it + 1)
            # as in the fused engine: the other ranks wait for rank 0's write on the host
            # (process-group timeout), not inside the next step's bounded xGMI spin
            comm_util.barrier()
    _flush()
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    ddp.check_comm()
    t_end = time.perf_counter()
    dt = t_end - t0
    steady = None
    if t_steady is not None and config.iters > steady_from:
        steady = geom.batch * A * (config.iters - steady_from) * world / max(t_end - t_steady, 1e-9)
    if pbar is not None:
        pbar.close()
    if config.check_replicas:
        check_replicas(bank.flat)
    if config.checkpoint_dir:
        _save(config.iters)
    return {"final_loss": last, "iters": config.iters,
            "samples_per_s": geom.batch * A * (config.iters - start) * world / max(dt, 1e-9),
            "steady_samples_per_s": steady, "engine": "module", "accumulate_grad_batches": A, **val.summary(),
            "graph_replays": stepper.replays,
            # clipping by norm: each model's gradient norm at the last step, before clipping
            **({"grad_norm": opt.grad_norm.tolist()} if _clip_norm(config) > 0 else {}),
            **({"phases": timer.summary()} if trace_enabled() else {})}


class _Seeds:
    """d loss / d loss: one cached tensor of ones per shape (a captured step replays it)."""

    def __init__(self, device):
        self.device = device
        self._t: dict = {}

    def get(self, shape, value: float = 1.0):
        t = self._t.get((tuple(shape), value))
        if t is None:
            t = self._t[(tuple(shape), value)] = torch.full(shape, value, dtype=torch.float32, device=self.device)
        return t


# ----------------------------------------------------------------------------- stock engine
def _train_stock(config, device, rank, world, logger, faults) -> dict:
    from ..baselines.stock import StockLoop

    ds = _dataset(config, rank)
    loop = StockLoop(ds, device, batch=config.batch_size, seed=config.seed,
                     clip_grad_norm=_clip_norm(config), clip_grad_value=_clip_value(config),
                     schedule=lr_schedule(config), accumulate=_accumulate(config),
                     # the verbatim Adam(lr=1e-3) pair unless the run asks for AdamW
                     optim=_optim(config) if config.optimizer == "adamw" else None)
    pbar = _progress(rank, config.iters, config)
    timer = PhaseTimer(device)
    val = _Validation(config, ds, rank, world, device, logger)
    val.ce = False  # the stock loop trains one-output models with MSE whatever --loss says
    t0 = time.perf_counter()
    for it in range(config.iters):
        faults.check(it)
        with timer.phase("step"):
            loop.step()
        if rank == 0:
            logger.log({"loss/lossX": loop.last[0]}, step=it, commit=False)
            logger.log({"loss/lossY": loop.last[1]}, step=it)
        if val.due(it + 1):
            with timer.phase("validation"):
                val.report(it + 1, val.reduce(*val.sums_torch(loop.forward_eval), 1))
        if pbar is not None:
            pbar.update(1)
    dt = time.perf_counter() - t0
    if pbar is not None:
        pbar.close()
    if config.checkpoint_dir:
        # the trained weights as the other engines' flat rows (torch order), so a run's
        # validation loss can be checked against them; the stock loop does not resume
        flat = torch.stack([torch.nn.utils.parameters_to_vector(m.parameters()).detach() for m in (loop.mx, loop.my)])
        checkpoint.save({"engine": "stock", "params": flat, "config": vars(config)}, config.checkpoint_dir,
                        config.iters)
    loop.close()
    return {"final_loss": list(loop.last), "iters": config.iters,
            "samples_per_s": loop.samples * world / max(dt, 1e-9), "engine": "stock",
            "accumulate_grad_batches": loop.accumulate, **val.summary(),
            **({"phases": timer.summary()} if trace_enabled() else {})}


def teardown():
    if dist.is_initialized():
        comm_util.barrier()
        dist.destroy_process_group()

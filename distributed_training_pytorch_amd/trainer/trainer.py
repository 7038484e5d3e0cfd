"""Trainer: a PyTorch-Lightning-1.5-compatible training driver (the parts the reference
uses: ``pl.Trainer(gpus, num_nodes, max_steps, precision=32, accelerator='gpu',
log_every_n_steps, strategy='ddp')`` + ``fit``, ``demo_pytorch_lightning.py:57-62``).

Semantics kept from PL 1.5.10:
* cluster environment: SLURM (SLURM_PROCID/LOCALID/NODEID/NTASKS + MASTER_ADDR/PORT)
  or torchrun env, else one process; backend from ``PL_TORCH_DISTRIBUTED_BACKEND``;
* ``strategy='ddp'``: rank-0 parameter broadcast, gradient averaging on every
  backward (FlatDDP: flat buffer, bucketed RCCL all-reduce overlapped with the
  backward, unused-parameter tolerant), DistributedSampler auto-injected into a
  sampler-less DataLoader;
* several optimizers: per batch, for each optimizer: toggle (only its params
  require grad), training_step(batch, batch_idx, optimizer_idx), backward, step,
  zero_grad; ``global_step`` advances once per BATCH (PL 1.5, not 1.6+);
* ``log_every_n_steps`` (a float in the reference, 0.03125) is clamped to an int >= 1;
* default checkpointing: ``{root}/lightning_logs/version_N/checkpoints/
  epoch={e}-step={s}.ckpt`` at the end of training; CSV metrics alongside.
MI355X-first: a dataset exposing device tensors (``ToyData``) is gathered on the GPU
(no collation/pin-memory per batch), the model's layers run as fused HIP kernels.
"""
from __future__ import annotations

import contextlib
import copy
import dataclasses
import ctypes
import csv
import datetime
import math
import os
import time
import warnings
from pathlib import Path

import torch
import torch.distributed as dist

from .. import _native as nat
from ..data.sampler import SamplerGeometry, torch_distributed_indices
from ..ops.mlp import ParamBackwardFusion
from ..parallel import comm_util
from ..parallel.ddp import FlatDDP
from ..runtime import bootstrap
from ..utils.logging import rank_print


class CSVLogger:
    def __init__(self, root: str, rank: int):
        self.rank = rank
        self.dir = None
        if rank != 0:
            return
        base = Path(root) / "lightning_logs"
        base.mkdir(parents=True, exist_ok=True)
        n = 0
        while (base / f"version_{n}").exists():
            n += 1
        self.dir = base / f"version_{n}"
        self.dir.mkdir(parents=True)
        self._f = open(self.dir / "metrics.csv", "w", newline="")
        self._w = None
        self._widen = False

    def allow_new_columns(self) -> None:
        """From now on a row with metrics the header lacks widens the header (validation
        metrics arrive after the first training rows) instead of dropping them."""
        self._widen = True

    def _fit_header(self, keys) -> None:
        """Add the columns of ``keys`` the header lacks: the file is rewritten once under
        the wider header, the rows written so far keep their text, their new cells empty."""
        if not self._widen or self._w is None:
            return
        new = [k for k in keys if k not in self._w.fieldnames]
        if not new:
            return
        path = self.dir / "metrics.csv"
        self._f.close()
        with open(path, newline="") as f:
            old = list(csv.DictReader(f))
        self._f = open(path, "w", newline="")
        self._w = csv.DictWriter(self._f, fieldnames=[*self._w.fieldnames, *new], extrasaction="ignore")
        self._w.writeheader()
        self._w.writerows(old)

    def log(self, step: int, metrics: dict):
        if self.dir is None:
            return
        row = {"step": step, **{k: float(v) for k, v in metrics.items()}}
        self._fit_header(row.keys())
        if self._w is None:
            self._w = csv.DictWriter(self._f, fieldnames=list(row.keys()), extrasaction="ignore")
            self._w.writeheader()
        self._w.writerow(row)

    def log_rows(self, steps, names, rows):
        """One row per (step, values): ``names[i]`` = ``values[i]`` plus their sum as
        ``train_loss`` (the fused engine's per-launch loss block, written in one call)."""
        if self.dir is None or not steps:
            return
        if self._w is None:
            self.log(steps[0], {**dict(zip(names, rows[0])), "train_loss": sum(rows[0])})
            steps, rows = steps[1:], rows[1:]
        self._fit_header(["step", *names, "train_loss"])
        if list(self._w.fieldnames) == ["step", *names, "train_loss"]:
            # the csv module's own text for these rows (floats as repr, excel's \r\n), formatted
            # directly: ~5 us per row through DictWriter made the host, not the GPU, the
            # limit of the fused engine's every-step logging (a step is ~3 us)
            self._f.write("".join(f"{s},{','.join(map(repr, r))},{sum(r)!r}\r\n" for s, r in zip(steps, rows)))
            return
        self._w.writerows({"step": s, **dict(zip(names, r)), "train_loss": sum(r)} for s, r in zip(steps, rows))

    def log_block(self, step0: int, every: int, names, rows: torch.Tensor, first: int = 0) -> None:
        """``log_rows`` for a host tensor of loss rows ([n, len(names)] fp32): rows
        ``first, first + every, ...`` at steps ``step0, step0 + every, ...``, formatted
        natively (``csrc/host_log.hip``, the csv module's exact text, ~0.5 us per row
        instead of ~5) when the library is loaded."""
        if self.dir is None:
            return
        sel = rows[first::every]
        n = sel.shape[0]
        if n == 0:
            return
        if self._w is None:
            self._w = csv.DictWriter(self._f, fieldnames=["step", *names, "train_loss"], extrasaction="ignore")
            self._w.writeheader()
        self._fit_header(["step", *names, "train_loss"])
        r = rows.detach()
        if (nat.native_enabled() and os.environ.get("DTP_NATIVE_LOG", "1") != "0"
                and r.device.type == "cpu" and r.dtype == torch.float32 and r.dim() == 2
                and r.is_contiguous() and r.shape[1] == len(names)
                and list(self._w.fieldnames) == ["step", *names, "train_loss"]):
            lib = nat.load()
            cap = lib.dtp_format_loss_rows_bound(len(names), n)
            buf = ctypes.create_string_buffer(cap)
            m = lib.dtp_format_loss_rows(nat.ptr(r), len(names), first, n, every, step0, every, 1, buf, cap)
            if m >= 0:
                self._f.write(buf.raw[:m].decode("ascii"))
                return
        self.log_rows(list(range(step0, step0 + n * every, every)), names, sel.tolist())

    def flush(self):
        if self.dir is not None:
            self._f.flush()

    def close(self):
        if self.dir is not None:
            self._f.close()


class _DeviceBatches:
    """Device-resident replacement for DataLoader(DistributedSampler(ds), batch_size).

    With ``use_ring()`` (a GPU and batches one workgroup gathers, the Trainer's replayed
    step) the epoch's indices live in a device ring ``{cursor, indices}`` that the
    replayed step's gather reads and advances itself (``ops.gather.gather_rows2_ring``):
    one asynchronous upload from pinned memory per epoch -- none at all while the order
    does not change (one rank: no shuffle) -- instead of a pageable upload per epoch and
    an index copy per batch.  ``skip`` (set before iterating) is the number of leading
    batches the caller will not run (a mid-epoch resume): the cursor starts there."""

    def __init__(self, X, Y, batch, world, rank, shuffle, seed=0):
        self.X, self.Y = X, Y
        self.geom = SamplerGeometry(n=X.shape[0], world=world, rank=rank, batch=batch, shuffle=shuffle, seed=seed)
        self.epoch = 0
        self.skip = 0
        self.ring = None  # int64 [1 + steps * batch] on the device: cursor, then the epoch's indices
        self._ring_idx = None  # the indices the ring holds (host copy)
        self._ring_clean = False  # the last epoch ran to its end: cursor mod steps == 0

    def __len__(self):
        return self.geom.steps_per_epoch

    def set_epoch(self, e):
        self.epoch = e

    def use_ring(self) -> bool:
        from ..ops.gather import ring_gather_ok

        if os.environ.get("DTP_TRAINER_RING", "1") == "0":  # A/B switch: the per-batch index copy
            return False
        if self.ring is None and ring_gather_ok(self.X, self.Y, self.geom.batch):
            self.ring = torch.zeros(1 + len(self) * self.geom.batch, dtype=torch.int64, device=self.X.device)
        return self.ring is not None

    def __iter__(self):
        g = self.geom
        idx = torch_distributed_indices(g.n, g.world, g.rank, self.epoch, g.seed, g.shuffle)
        skip, self.skip = self.skip, 0
        if self.ring is not None:
            idx_h = torch.tensor(idx, dtype=torch.int64)
            if not (self._ring_clean and skip == 0 and self._ring_idx is not None
                    and torch.equal(idx_h, self._ring_idx)):
                host = torch.empty(self.ring.numel(), dtype=torch.int64, pin_memory=self.ring.is_cuda)
                host.zero_()
                host[0] = skip
                host[1:1 + idx_h.numel()] = idx_h
                self.ring.copy_(host, non_blocking=True)  # stream-ordered after the last epoch's gathers
                self._ring_idx = idx_h
            idx_t = self.ring[1:1 + idx_h.numel()]
        else:
            idx_t = torch.tensor(idx, device=self.X.device)
        self._ring_clean = False
        for b in range(len(self)):
            yield _DevBatch(self.X, self.Y, idx_t[b * g.batch:(b + 1) * g.batch], self)
        self._ring_clean = True


class _DevBatch:
    """One batch of ``_DeviceBatches``: the sample indices, gathered on demand.  A
    replayed step gathers inside its graph into the static batch buffers: from the
    epoch ring (nothing per batch on the host side) or from a static index buffer the
    caller refreshes (one small index copy per batch)."""

    __slots__ = ("X", "Y", "sel", "src")

    def __init__(self, X, Y, sel, src):
        self.X, self.Y, self.sel, self.src = X, Y, sel, src

    @property
    def ring(self):
        return self.src.ring

    def materialize(self):
        return [self.X[self.sel], self.Y[self.sel]]

    def gather_into(self, idx, out):
        # both tensors in ONE launch (two index_selects otherwise): each launch costs ~4 us in
        # the replayed step
        from ..ops.gather import gather_rows2, gather_rows2_ring

        if idx is None:
            g = self.src.geom
            gather_rows2_ring(self.X, self.Y, self.src.ring, g.batch, g.steps_per_epoch, out[0], out[1])
        else:
            gather_rows2(self.X, self.Y, idx, out[0], out[1])


_STEADY_AFTER = 10  # batches excluded from Trainer.steady_time


class _MetricRing:
    """Logged metrics of many steps, reduced and written in one go.

    PL logs (``self.log``) every ``log_every_n_steps`` batches -- every batch in the
    reference (``log_every_n_steps=0.03125``).  Reducing and printing each of those on
    the host costs a collective and a device->host sync per batch, which would stall
    the replayed step after every batch.  Instead each logged step's values are stacked
    into a device row, and every ``rows`` logged steps -- and before a checkpoint and at
    the end of ``fit`` -- the block is averaged over ranks with ONE all-reduce, copied to
    the host once and written to ``metrics.csv`` row by row -- without a device sync:
    a block's rows are written once its copy has arrived (``flush``).
    ``callback_metrics`` is the last row of the newest written block, so it trails the
    live step by less than 2 x ``rows`` logged steps during training and is exact after
    ``fit``.

    The stack itself is deferred: a logged step's tensors are kept (``pending``) until
    ``defer`` steps are waiting or the graph copy that wrote them (``owner``) is about to
    be replayed again (``release``), then all waiting rows are stacked in ONE launch --
    with the Trainer's ``graph_copies`` replayed graphs per batch shape, one stack per
    ``graph_copies`` batches instead of one per batch."""

    def __init__(self, trainer, logger, rows: int = 64, defer: int = 1):
        self.tr = trainer
        self.logger = logger
        self.rows = rows
        self.defer = max(1, int(defer))
        self.buf = None
        self.keys: list = []
        self.steps: list = []
        self.pending: list = []  # (step, [tensors], owner)
        self._inflight: list = []  # (event, pinned rows, steps, keys) copied but not yet written
        self._sync_flush = os.environ.get("DTP_TRAINER_SYNC_FLUSH", "0") == "1"  # A/B: the blocking flush

    def push(self, step: int, logged: dict, owner=None) -> None:
        keys = list(logged.keys())
        if not keys:
            return
        if self.buf is None or keys != self.keys:
            self.flush()
            self.keys = keys
            self.buf = torch.empty(self.rows, len(keys), dtype=torch.float32, device=self.tr.device)
        self.pending.append((step, [v.detach() for v in logged.values()], owner))
        if len(self.pending) >= self.defer or len(self.steps) + len(self.pending) >= self.rows:
            self._stack_pending()
            if len(self.steps) == self.rows:
                self.flush(wait=self._sync_flush)

    def release(self, owner) -> None:
        """``owner``'s output tensors are about to be overwritten: stack what waits."""
        if any(o == owner for _, _, o in self.pending):
            self._stack_pending()

    def _stack_pending(self) -> None:
        if not self.pending:
            return
        n0, k = len(self.steps), len(self.pending)
        vals = [v.float().reshape(()) for _, vs, _ in self.pending for v in vs]
        torch.stack(vals, out=self.buf[n0:n0 + k].view(-1))
        self.steps.extend(st for st, _, _ in self.pending)
        self.pending = []

    def flush(self, wait: bool = True) -> None:
        """Reduce the block and start its copy to the host.  ``wait=False`` (the periodic
        flush inside training): no device sync -- the copy lands in pinned memory behind
        the queued batches and its rows are written at a later flush once it has arrived,
        so the replayed steps queued behind it keep the GPU busy while the host writes
        CSV.  ``wait=True`` (checkpoint, end of ``fit``): everything written now."""
        self._stack_pending()
        if self.steps:
            block = self.buf[:len(self.steps)]
            if self.tr.world_size > 1:
                comm_util.all_reduce_(block)
                block /= self.tr.world_size
            ev = None
            if block.is_cuda:
                host = torch.empty(block.shape, dtype=block.dtype, pin_memory=True)
                host.copy_(block, non_blocking=True)  # stream-ordered before the rows are reused
                ev = torch.cuda.Event()
                ev.record()
            else:
                host = block.clone()
            self._inflight.append((ev, host, self.steps, self.keys))
            self.steps = []
        while self._inflight and (wait or self._inflight[0][0] is None or self._inflight[0][0].query()):
            ev, host, steps, keys = self._inflight.pop(0)
            if ev is not None:
                ev.synchronize()
            rows = host.tolist()
            for step, vals in zip(steps, rows):
                self.logger.log(step, dict(zip(keys, vals)))
            self.logger.flush()
            self.tr.callback_metrics = {**dict(zip(keys, rows[-1])), **self.tr._val_metrics}


class Trainer:
    def __init__(self, gpus: int | None = None, num_nodes: int = 1, max_steps: int = -1, max_epochs: int | None = None,
                 precision: int = 32, accelerator: str | None = None, strategy: str | None = None,
                 log_every_n_steps: float = 50, default_root_dir: str | None = None,
                 enable_checkpointing: bool = True, enable_progress_bar: bool = True, seed: int | None = None,
                 use_graphs: bool = True, native_optimizers: bool = True, every_n_train_steps: int = 0,
                 engine: str = "auto", graph_copies: int | None = None, gradient_clip_val: float | None = None,
                 gradient_clip_algorithm: str = "norm", check_val_every_n_epoch: int = 1,
                 val_check_interval: int | None = None, **unused):
        if precision in (32, "32", "32-true"):
            self.autocast_dtype = None
        elif precision in ("bf16", "bf16-mixed"):
            # PL: torch.autocast(bf16) around training_step; fp32 master weights and optimizer
            self.autocast_dtype = torch.bfloat16
        else:
            raise NotImplementedError(f"precision={precision!r}: supported are 32 and 'bf16'")
        self.precision = precision
        # PL 1.5: clip each optimizer's gradients after its backward (and the all-reduce),
        # before its step; None or 0 = off.  "norm": clip_grad_norm_, "value": clip_grad_value_
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm={gradient_clip_algorithm!r}: 'norm' or 'value'")
        self.gradient_clip_val = float(gradient_clip_val or 0.0)
        if self.gradient_clip_val < 0:
            raise ValueError(f"gradient_clip_val={gradient_clip_val!r}: must be >= 0")
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.gpus = gpus
        self.num_nodes = num_nodes
        self.max_steps = -1 if max_steps is None else int(max_steps)  # PL 1.5: None = unbounded
        self.max_epochs = max_epochs if max_epochs is not None else (1000 if self.max_steps < 0 else None)
        self.accelerator = accelerator or ("gpu" if torch.cuda.is_available() and gpus else "cpu")
        self.strategy = strategy
        self.log_every_n_steps = max(1, int(log_every_n_steps))  # reference passes 0.03125
        self.root = default_root_dir or os.getcwd()
        self.enable_checkpointing = enable_checkpointing
        self.enable_progress_bar = enable_progress_bar
        self.seed = seed
        self.use_graphs = use_graphs  # replay each batch's optimizer steps as a hipGraph (GPU)
        # graphs captured per batch shape, replayed in turn: each keeps its logged outputs
        # until its next replay, so the metric rows are stacked once per `graph_copies` batches
        # (default 4; DTP_TRAINER_GRAPH_COPIES overrides the default, for A/Bs)
        if graph_copies is None:
            graph_copies = int(os.environ.get("DTP_TRAINER_GRAPH_COPIES", "4"))
        self.graph_copies = max(1, int(graph_copies))
        # run a plain torch Adam/SGD over a flat-buffer span as ONE flat-optimizer kernel (GPU)
        self.native_optimizers = native_optimizers
        self._flat_opts: list = []
        # configure_optimizers' schedulers: {"scheduler", "interval", "frequency", "opt"} each
        self._sched_recs: list = []
        self.lr_tables: list = []  # per optimizer: the tabulated rates the kernels read, or None
        self._opt_zeroes = False  # the flat optimizers zero the gradient they consume (fit)
        # the backward's last stage kernel fused with the flat optimizer step (one rank);
        # DTP_TRAINER_FUSE_OPT=0 launches them separately (A/B)
        self._fuse_backward_opt = os.environ.get("DTP_TRAINER_FUSE_OPT", "1") != "0"
        self.graph_replays = 0
        self.global_step = 0
        self.current_epoch = 0
        self.callback_metrics: dict = {}
        self.checkpoint_path: str | None = None
        # ModelCheckpoint(every_n_train_steps=N): also save ``last.ckpt`` every N batches
        # (what a restarted job resumes from, fit(ckpt_path="last"))
        self.every_n_train_steps = int(every_n_train_steps or 0)
        # "auto": the fused train-step engine when the LightningModule declares its step
        # (``fused_spec``) and everything it needs matches; "module": always the
        # per-batch nn.Module path; "fused": the fused engine or an error
        if engine not in ("auto", "fused", "module"):
            raise ValueError(f"engine={engine!r}: auto, fused or module")
        self.engine = engine
        self.engine_used = "module"
        self.fused_refused: str | None = None  # why fused_spec() was not trusted (checked on the first batch)
        # validation (PL 1.5 subset): after every check_val_every_n_epoch-th epoch, or --
        # val_check_interval, an int -- after every that many batches of those epochs
        self.check_val_every_n_epoch = max(1, int(check_val_every_n_epoch or 1))
        if val_check_interval is not None and (isinstance(val_check_interval, float) or int(val_check_interval) < 1):
            raise ValueError(f"val_check_interval={val_check_interval!r}: an int count of batches >= 1")
        self.val_check_interval = None if val_check_interval is None else int(val_check_interval)
        self.val_fused_refused: str | None = None  # why fused_spec()'s val_metrics were not trusted
        self._val_metrics: dict = {}
        self._skip_batches = 0
        self._batch_in_epoch = 0
        self._log_dir = None

    # ------------------------------------------------------------------ distributed
    def _setup(self):
        bootstrap.configure_collective_env()  # before bind_device: HSA reads the IPC mode at its first touch
        env = bootstrap.detect()
        device = torch.device("cpu")
        if self.accelerator == "gpu" and torch.cuda.is_available():
            device = bootstrap.bind_device(env, "cuda")
        if self.strategy in ("ddp", "ddp_spawn", "ddp_find_unused_parameters_false") or env.world_size > 1:
            backend = os.environ.get("PL_TORCH_DISTRIBUTED_BACKEND", "nccl" if device.type == "cuda" else "gloo")
            bootstrap.init_process_group(env, backend, device, datetime.timedelta(minutes=60))
        self.env = env
        self.device = device
        self.world_size = dist.get_world_size() if dist.is_initialized() else 1
        self.global_rank = dist.get_rank() if dist.is_initialized() else 0
        expected = (self.gpus or 1) * self.num_nodes
        if self.global_rank == 0 and dist.is_initialized() and self.world_size != expected:
            rank_print(0, f"note: world size {self.world_size} != gpus*num_nodes {expected}")

    def _loader(self, dl):
        ds = getattr(dl, "dataset", dl)
        bs = getattr(dl, "batch_size", None) or 1
        if hasattr(ds, "device_tensors"):
            X, Y = ds.device_tensors(self.device)
            return _DeviceBatches(X, Y, bs, self.world_size, self.global_rank, shuffle=self.world_size > 1)
        if self.world_size > 1 and not isinstance(getattr(dl, "sampler", None),
                                                   torch.utils.data.distributed.DistributedSampler):
            from torch.utils.data import DataLoader, DistributedSampler

            s = DistributedSampler(ds, shuffle=True)
            return DataLoader(ds, batch_size=bs, sampler=s, num_workers=getattr(dl, "num_workers", 0),
                              pin_memory=self.device.type == "cuda")
        return dl

    # ------------------------------------------------------------------ fit
    def fit(self, model, train_dataloaders=None, train_dataloader=None, ckpt_path: str | None = None, *,
            val_dataloaders=None):
        """Train ``model``.  ``val_dataloaders`` (keyword only) with a ``validation_step``:
        validation epochs between training batches (``_run_validation``).  ``ckpt_path`` resumes (PL's ``fit(ckpt_path=...)``): a
        checkpoint file, or ``"last"`` for the newest ``last.ckpt`` / final checkpoint
        under ``{root}/lightning_logs``; weights, optimizer states, ``global_step``,
        epoch and the position inside the epoch are restored, so a restarted job
        (torchrun ``--max_restarts``) continues where the checkpoint was taken."""
        dl = train_dataloaders if train_dataloaders is not None else train_dataloader
        self._setup()
        if self.seed is not None:
            torch.manual_seed(self.seed)
        model.trainer = self
        model.to(self.device)
        opts, self._sched_recs = _parse_optimizers(model.configure_optimizers())
        self.lr_tables = [None] * len(opts)
        resume = self._resolve_ckpt(ckpt_path)
        if resume is not None:
            self._restore(model, opts, resume)
        self._val_metrics = {}
        val_dl = val_dataloaders if _has_validation_step(model) else None
        plan = self._fused_plan(model, opts, dl)
        if plan is not None:
            done = self._fit_fused(model, opts, plan, val_dl)
            if done is not None:
                return done
        # the flat gradient buffer of FlatDDP also serves one process: fused kernels add
        # their parameter gradients into its views in place (no AccumulateGrad adds)
        single_ok = self.device.type == "cuda" and all(
            p.dtype == torch.float32 and p.device == self.device for p in model.parameters() if p.requires_grad)
        ddp = FlatDDP(model) if (self.world_size > 1 or single_ok) else None
        loader = self._loader(dl)
        self._flat_opts = [_flat_optimizer_for(o, ddp, self._clip_fields()) if self.native_optimizers else None
                           for o in opts]
        # every trainable parameter under exactly one flat optimizer (one optimizer, or
        # several toggled per PL 1.5 so a backward touches only the stepping optimizer's
        # gradients): each flat step leaves the whole flat gradient zero
        self._opt_zeroes = False
        if ddp is not None and self._flat_opts and all(f is not None for f in self._flat_opts):
            owned = [id(p) for f in self._flat_opts for p in f.params]
            self._opt_zeroes = len(owned) == len(set(owned)) and set(owned) == {id(p) for p in ddp._params}
        stepper, static = self._batch_stepper(model, ddp, opts)
        if stepper is not None and isinstance(loader, _DeviceBatches):
            loader.use_ring()  # the replayed step reads its batches from the device epoch ring
        logged_by_key: dict = {}
        logger = CSVLogger(self.root, self.global_rank)
        self._log_dir = logger.dir
        copies = self.graph_copies if stepper is not None else 1
        metrics = _MetricRing(self, logger, defer=copies)
        vloader = None
        if val_dl is not None:
            vloader = self._val_loader(val_dl)
            logger.allow_new_columns()
        spe = len(loader) if hasattr(loader, "__len__") else None
        self._table_flat_opts(opts, spe)
        pbar = None
        if self.enable_progress_bar and self.global_rank == 0:
            try:
                from tqdm import tqdm

                pbar = tqdm(total=self.max_steps if self.max_steps > 0 else None, desc="Epoch 0",
                            initial=self.global_step)
            except ImportError:  # pragma: no cover
                pbar = None
        model.on_train_start()
        t0 = time.perf_counter()
        # steady-state clock: from the end of batch _STEADY_AFTER on (warm-up batches,
        # graph capture and first kernel loads excluded); synchronised at both ends
        # (the warm-up runs and every graph copy's capture come first)
        self.steady_time, self.steady_steps, steady_t0 = None, 0, None
        steady_from = self.global_step + max(_STEADY_AFTER, copies + 6)
        done = 0 <= self.max_steps <= self.global_step or \
            (self.max_epochs is not None and self.current_epoch >= self.max_epochs)
        try:
            while not done:
                if isinstance(loader, _DeviceBatches):
                    loader.skip = self._skip_batches
                if hasattr(loader, "set_epoch"):
                    loader.set_epoch(self.current_epoch)
                elif hasattr(getattr(loader, "sampler", None), "set_epoch"):
                    loader.sampler.set_epoch(self.current_epoch)
                for batch_idx, batch in enumerate(loader):
                    if batch_idx < self._skip_batches:  # resumed mid-epoch: these already ran
                        continue
                    dev = batch if isinstance(batch, _DevBatch) else None
                    if dev is not None and stepper is None:
                        batch = dev.materialize()
                    elif dev is None:
                        batch = [b.to(self.device, non_blocking=True) for b in batch]
                    if self._refresh_flat_opts() and stepper is not None:
                        stepper.reset()  # the captured optimizer launches hold the old hyperparameters
                    if stepper is not None and (dev is not None or self._static_ok(static, batch)):
                        if dev is not None:  # gather inside the replayed step
                            key = ("idx", dev.sel.shape[0])
                            if key not in static:
                                static[key] = _StaticBatch(dev.materialize(),
                                                           None if dev.ring is not None else dev.sel.clone(), dev)
                            if static[key].idx is not None:  # no ring: the batch's indices in
                                static[key].idx.copy_(dev.sel)
                        else:
                            key = tuple(tuple(b.shape) for b in batch)
                            if key not in static:
                                static[key] = _StaticBatch([b.clone() for b in batch])
                            for dst, src in zip(static[key].tensors, batch):
                                dst.copy_(src)
                        self._cur_batch_idx = batch_idx  # read by the body only while capturing
                        # several graph copies per batch shape, replayed in turn: a copy's
                        # logged outputs stay valid until its next replay (_MetricRing.release)
                        gkey = (key, self.global_step % copies)
                        replay = stepper.is_captured(gkey)
                        if replay:
                            metrics.release(gkey)
                        stepper.run(gkey, warm_key=key)
                        # logged tensors of a replay are that copy's graph outputs (refreshed in place)
                        if replay:
                            model._logged.update(logged_by_key[gkey])
                        else:
                            logged_by_key[gkey] = dict(model._logged)
                        owner = gkey
                    else:
                        self._optimizer_steps(model, ddp, opts, batch, batch_idx)
                        owner = None
                    self.global_step += 1  # PL 1.5: once per batch, whatever the optimizer count
                    # the schedulers, before any hook, log or checkpoint can observe them
                    for fo in self._flat_opts:
                        if fo is not None:
                            fo.host_t += 1
                    self._advance_schedulers(self.global_step, spe)
                    if self.global_step == steady_from:
                        if self.device.type == "cuda":
                            torch.cuda.synchronize(self.device)
                        steady_t0 = time.perf_counter()
                    self._batch_in_epoch = batch_idx + 1
                    if self.global_step % self.log_every_n_steps == 0:
                        metrics.push(self.global_step, model._logged, owner)
                    if pbar is not None:
                        pbar.update(1)
                    if self.every_n_train_steps and self.global_step % self.every_n_train_steps == 0:
                        metrics.flush()
                        self._save(model, opts, "last.ckpt")
                    if vloader is not None and self._val_due(self.current_epoch, batch_idx + 1, spe):
                        metrics.flush()  # the training rows up to here first
                        self._log_validation(logger, self._run_validation(model, vloader))
                    if 0 <= self.max_steps <= self.global_step:
                        done = True
                        break
                else:
                    self.current_epoch += 1
                    self._batch_in_epoch = 0
                    if spe is None:  # an unsized loader: the epoch's end is known only here
                        self._advance_schedulers(self.current_epoch, None, epoch_end=True)
                self._skip_batches = 0
                if self.max_epochs is not None and self.current_epoch >= self.max_epochs:
                    done = True
            metrics.flush()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self.fit_time = time.perf_counter() - t0
            if steady_t0 is not None and self.global_step > steady_from:
                self.steady_time = time.perf_counter() - steady_t0
                self.steady_steps = self.global_step - steady_from
            if stepper is not None:
                self.graph_replays = stepper.replays
        finally:
            # the user's torch optimizers hold the trained state again -- before any
            # user hook runs, and also when training raised
            self._export_flat_opts()
            if pbar is not None:
                pbar.close()
        model.on_train_end()
        if self.enable_checkpointing:
            final = f"epoch={max(self.current_epoch - 1, 0) if self._batch_in_epoch == 0 else self.current_epoch}" \
                    f"-step={self.global_step}.ckpt"
            self._save(model, opts, final)
        logger.close()
        return self

    # ------------------------------------------------------------------ fused engine
    def _fused_plan(self, model, opts, dl):
        """The fused train-step engine (engine/fused_trainer.py) runs the fit when the
        LightningModule declares what its ``training_step`` computes --
        ``fused_spec() -> {"models": [m_0, ...], "loss": "mse", "metrics": [name_0, ...]}``:
        optimizer i trains ``models[i]`` (a ToyModel) on ``loss(models[i](x), y)`` of the
        same batch -- and the rest matches: a GPU, plain Adam / SGD optimizers with one
        param group over exactly one model's parameters each and equal hyperparameters,
        a dataset with ``device_tensors``, precision 32 or bf16.  Otherwise None (the
        per-batch module path); ``engine="fused"`` turns a mismatch into an error.

        PL-1.5 semantics kept: each optimizer's update uses the gradient of its own
        model's loss (the models are independent, so toggling the other optimizer's
        parameters changes nothing), ``global_step`` counts batches, the
        DistributedSampler order is exact at world > 1.  One difference in the logs:
        every model's loss is its loss BEFORE this batch's update, where Lightning's
        second ``training_step`` call would log the first model's post-update loss."""
        from ..models.toy import ToyModel

        if self.engine == "module":
            return None

        def no(why):
            if self.engine == "fused":
                raise RuntimeError(f"Trainer(engine='fused'): {why}")
            return None

        if self.gradient_clip_val > 0:
            # the Trainer does not drive the fused engine's clip twins (FusedTrainer with a clipping
            # OptimConfig): the module path's flat optimizer kernel clips
            why = f"gradient clipping (gradient_clip_val={self.gradient_clip_val:g}) is not in the fused engine"
            no(why)
            if self.global_rank == 0:
                rank_print(0, f"Trainer: not using the fused engine ({why}); per-batch module path")
            self.fused_refused = why
            return None

        fs = getattr(model, "fused_spec", None)
        fs = fs() if callable(fs) else None
        if not fs:
            return no("the LightningModule defines no fused_spec()")
        if self.device.type != "cuda":
            return no("the fused engine needs a GPU")
        models, names = list(fs["models"]), list(fs.get("metrics") or [])
        loss = fs.get("loss", "mse")
        if loss not in ("mse", "ce") or len(names) != len(models) or len(opts) != len(models):
            return no("fused_spec must name one metric per model and match one optimizer per model")
        if not all(isinstance(m, ToyModel) for m in models) or any(m.spec != models[0].spec for m in models):
            return no("fused_spec models must be ToyModels of one architecture")
        cfgs = []
        for o, m in zip(opts, models):
            cfg = _optim_config(o)
            ps = list(m.parameters())
            if cfg is None or len(o.param_groups) != 1 or len(o.param_groups[0]["params"]) != len(ps) or \
                    any(a is not b for a, b in zip(o.param_groups[0]["params"], ps)):
                return no("each optimizer must be a plain Adam/SGD over exactly its model's parameters")
            cfgs.append(cfg)
        if any(c != cfgs[0] for c in cfgs):
            return no("the optimizers' hyperparameters differ")
        ds = getattr(dl, "dataset", None)
        if not hasattr(ds, "device_tensors"):
            return no("the dataset has no device_tensors()")
        optim = cfgs[0]
        if self._sched_recs:
            # the engine reads ONE table by its step counter: every optimizer's scheduler must
            # tabulate (nothing but lr moves) and to the same values
            distributed = self.world_size > 1
            spe = SamplerGeometry(n=len(ds), world=self.world_size, rank=self.global_rank,
                                  batch=int(getattr(dl, "batch_size", None) or 1), shuffle=distributed,
                                  distributed=distributed, seed=0).steps_per_epoch
            tabs = [self._tabulate(opts, i, self.global_step, spe) for i in range(len(opts))]
            why = None
            if any(t is None for i, t in enumerate(tabs) if any(r["opt"] == i for r in self._sched_recs)):
                why = "a learning-rate scheduler cannot be tabulated (it moves more than lr, or has no planned length)"
            elif any(t != tabs[0] for t in tabs):
                why = "the optimizers' learning-rate tables differ (the fused engine has one OptimConfig)"
            if why is not None:
                self.fused_refused = why
                if self.global_rank == 0 and self.engine != "fused":
                    rank_print(0, f"Trainer: not using the fused engine ({why}); per-batch module path")
                return no(why)
            if tabs[0] is not None:
                from ..ops.schedule import LrSchedule

                optim = dataclasses.replace(optim, schedule=LrSchedule.from_values(tabs[0]))
                self.lr_tables = list(tabs)
        prec = "fp32" if self.autocast_dtype is None else "bf16"
        return {"models": models, "names": names, "loss": loss, "optim": optim, "dataset": ds,
                "val_names": list(fs.get("val_metrics") or []),
                "batch": int(getattr(dl, "batch_size", None) or 1), "precision": prec, "spec": models[0].spec}

    def _fit_fused(self, model, opts, plan, val_dl=None):
        from ..engine.fused_trainer import EngineConfig, FusedTrainer

        models, names = plan["models"], plan["names"]
        X, Y = plan["dataset"].device_tensors(self.device)
        distributed = self.world_size > 1  # PL injects DistributedSampler(shuffle=True) under DDP
        geom = SamplerGeometry(n=X.shape[0], world=self.world_size, rank=self.global_rank, batch=plan["batch"],
                               shuffle=distributed, distributed=distributed, seed=0)
        ecfg = EngineConfig(loss=plan["loss"], precision=plan["precision"])
        tr = FusedTrainer(plan["spec"], len(models), X, Y, geom, plan["optim"], ecfg,
                          init_params=[m.flat_params.detach() for m in models])
        self._skip_batches = 0  # the engine positions its sampler from the step count
        # DDP construction semantics: the engine broadcast rank 0's weights; the modules
        # take them too, so the check below runs training_step on the weights the engine
        # trains (ranks that built their models from different seeds agree from here on)
        for i, m in enumerate(models):
            m.load_flat_(tr.model_params(i))
        why = None
        if self.global_step:  # resumed: the torch optimizers' state continues in the engine
            why = self._import_fused_state(tr, models, opts, self.global_step)
        # fused_spec() is a declaration: check it against training_step on the first batch
        # before the engine trains anything (every rank agrees on the outcome)
        if why is None:
            why = self._verify_fused_spec(model, opts, plan, tr, X, Y)
        if self.world_size > 1:  # every rank takes the same decision
            flag = torch.tensor([0.0 if why is None else 1.0])
            comm_util.all_reduce_(flag)
            if why is None and flag.item() > 0:
                why = "the fused engine was refused on another rank"
        if why is not None:
            tr.close()
            if self.engine == "fused":
                raise RuntimeError(f"Trainer(engine='fused'): {why}")
            if self.global_rank == 0:
                rank_print(0, f"Trainer: not using the fused engine ({why}); per-batch module path")
            self.fused_refused = why
            return None
        self.engine_used = "fused"
        spe = geom.steps_per_epoch
        # the same stopping rule as the module loop: whichever of max_steps / max_epochs
        # comes first (max_epochs defaults to 1000 when max_steps is unset, __init__)
        limits = [self.max_steps] if self.max_steps >= 0 else []
        if self.max_epochs is not None:
            limits.append(self.max_epochs * spe)
        total = min(limits)
        logger = CSVLogger(self.root, self.global_rank)
        self._log_dir = logger.dir
        vloader, vdev, vchecked = None, None, False
        if val_dl is not None:
            vloader = self._val_loader(val_dl)
            logger.allow_new_columns()
            vds = getattr(val_dl, "dataset", val_dl)
            vnames = list(plan.get("val_names") or [])
            if len(vnames) == len(models) and hasattr(vds, "device_tensors"):
                vdev = vds.device_tensors(self.device)  # the engine's own evaluation kernel

        def validate():
            # weights back into the modules (stream-ordered copies) for the general loop;
            # with declared val_metrics the engine evaluates them itself -- checked once
            # against the general loop on the same weights, like fused_spec itself
            nonlocal vdev, vchecked
            if vdev is not None:
                ev = tr.evaluate(*vdev)
                res = {k: float(v) for k, v in zip(vnames, ev["loss"])}
                if not vchecked:
                    vchecked = True
                    for i, m in enumerate(models):
                        m.load_flat_(tr.model_params(i))
                    ref = self._run_validation(model, vloader)
                    tol = 1e-2 if plan["precision"] == "bf16" else 1e-5
                    bad = [k for k in vnames if k not in ref or not math.isclose(
                        res[k], ref[k], rel_tol=tol, abs_tol=1e-2 if tol > 1e-3 else 1e-6)]
                    if bad or set(ref) != set(vnames):
                        k = bad[0] if bad else sorted(set(ref) ^ set(vnames))[0]
                        self.val_fused_refused = (f"{k} of validation_step is {ref.get(k)!r}, the declared "
                                                  f"val_metrics give {res.get(k)!r}")
                        if self.global_rank == 0:
                            rank_print(0, f"Trainer: not using the engine's evaluation ({self.val_fused_refused})")
                        vdev = None
                        res = ref
                return res
            for i, m in enumerate(models):
                m.load_flat_(tr.model_params(i))
            return self._run_validation(model, vloader)

        model.on_train_start()
        if self.global_rank == 0:
            rank_print(0, f"Trainer: fused train-step engine ({tr.comm} comm, {plan['precision']})")
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        last = None
        # steady-state clock: the first launch runs _STEADY_AFTER steps (engine set-up and
        # first kernel loads), the clock runs from its end (synchronised by its loss readback)
        steady_t0, steady_from = None, None
        # launch k+1 is queued before launch k's loss rows are waited for and written
        # (losses_async: a pinned copy + event behind launch k), so the CSV writing
        # overlaps the next launch instead of idling the GPU
        pending = None

        def drain(p):
            nonlocal last
            s0_, s1_, handle = p
            rows = handle.wait_tensor()
            every = self.log_every_n_steps
            first = -(s0_ + 1) % every  # index of the first logged step of the launch
            logger.log_block(s0_ + first + 1, every, names, rows, first)
            last = rows[-1].tolist()

        try:
            while self.global_step < total:
                n = min(tr.cfg.steps_per_launch if steady_t0 is not None else _STEADY_AFTER, total - self.global_step)
                if self.every_n_train_steps:
                    n = min(n, self.every_n_train_steps - self.global_step % self.every_n_train_steps)
                val_at = self._val_next(self.global_step, spe) if vloader is not None else None
                if val_at is not None:  # launches are cut at the validation points
                    n = min(n, val_at - self.global_step)
                s0 = self.global_step
                tr.train(n)
                self.global_step += n
                # the real schedulers, to the count the engine's table has reached, before any
                # hook, log or checkpoint can observe them
                if self._sched_recs:
                    for g in range(s0 + 1, self.global_step + 1):
                        self._advance_schedulers(g, spe)
                handle = tr.losses_async(s0, self.global_step)
                if pending is not None:
                    drain(pending)
                pending = (s0, self.global_step, handle)
                if steady_t0 is None:
                    drain(pending)
                    pending = None
                    steady_t0, steady_from = time.perf_counter(), self.global_step
                # PL's bookkeeping: the batch that reaches max_steps ends the fit inside its
                # epoch (epoch e, batch_in_epoch = its index + 1), it does not open the next
                e, b = divmod(self.global_step - 1, spe)
                self.current_epoch, self._batch_in_epoch = e, b + 1
                if self.every_n_train_steps and self.global_step % self.every_n_train_steps == 0:
                    if pending is not None:
                        drain(pending)
                        pending = None
                    self._export_fused_state(tr, models, opts)
                    self._save(model, opts, "last.ckpt")
                if self.global_step == val_at:
                    if pending is not None:  # the training rows up to here first
                        drain(pending)
                        pending = None
                    self._log_validation(logger, validate())
            if pending is not None:
                drain(pending)
                pending = None
            torch.cuda.synchronize(self.device)
            t1 = time.perf_counter()
            self.fit_time = t1 - t0
            self.steady_time, self.steady_steps = None, 0
            if steady_t0 is not None and self.global_step > steady_from:
                self.steady_time, self.steady_steps = t1 - steady_t0, self.global_step - steady_from
            if last is not None:
                self.callback_metrics = {**dict(zip(names, last)), "train_loss": sum(last), **self._val_metrics}
        finally:
            self._export_fused_state(tr, models, opts)
            tr.close()
        model.on_train_end()
        if self.enable_checkpointing:
            final = f"epoch={max(self.current_epoch - 1, 0) if self._batch_in_epoch == 0 else self.current_epoch}" \
                    f"-step={self.global_step}.ckpt"
            self._save(model, opts, final)
        logger.close()
        return self

    def _verify_fused_spec(self, model, opts, plan, tr, X, Y) -> str | None:
        """Run ``training_step`` once on the batch the engine trains first (module path,
        autograd, no optimizer step) and compare every model's logged loss and parameter
        gradient with the engine's gradient-only launch of the same step (MODE_GRAD:
        local means, nothing updated).  Returns None when they agree (rtol 1e-4, atol
        1e-5: fp32 under different summation orders), else the reason (the caller makes
        every rank take the same decision)."""
        models, names = plan["models"], plan["names"]
        why = None
        try:
            idx = torch.as_tensor(tr.step_indices(self.global_step), dtype=torch.long, device=X.device)
            batch = [X[idx], Y[idx]]
            eng_g, eng_l = tr.local_gradients()
            saved = [p.requires_grad for p in model.parameters()]
            try:
                for oi, m in enumerate(models):
                    if len(opts) > 1:
                        model.toggle_optimizer(opts[oi], oi, opts)
                    with self._autocast():
                        out = model.training_step(batch, 0, oi) if len(opts) > 1 else model.training_step(batch, 0)
                    loss = out["loss"] if isinstance(out, dict) else out
                    ps = list(m.parameters())
                    gs = torch.autograd.grad(loss, ps, allow_unused=True)
                    g = torch.cat([(torch.zeros_like(p) if q is None else q).reshape(-1) for p, q in zip(ps, gs)])
                    logged = model._logged.get(names[oi])
                    if len(opts) > 1:
                        model.untoggle_optimizer(oi)
                    if logged is None:
                        why = f"training_step does not log {names[oi]!r}"
                        break
                    lv = float(torch.as_tensor(logged).detach().float().reshape(-1)[0])
                    tol = 1e-2 if plan["precision"] == "bf16" else 1e-4
                    if not math.isclose(lv, float(eng_l[oi]), rel_tol=tol, abs_tol=1e-5):
                        why = f"{names[oi]} of training_step is {lv:.6g}, the declared step gives {float(eng_l[oi]):.6g}"
                        break
                    if not torch.allclose(g.float(), eng_g[oi], rtol=tol, atol=1e-5 if tol < 1e-3 else 1e-3):
                        err = (g.float() - eng_g[oi]).abs().max().item()
                        why = f"model {oi}'s gradient from training_step differs from fused_spec's (max err {err:.3g})"
                        break
            finally:
                for p, r in zip(model.parameters(), saved):
                    p.requires_grad_(r)
                model._logged.clear()
        except Exception as e:  # noqa: BLE001 - any failure of the check refuses the engine
            why = f"fused_spec check failed: {e}"
        return why

    @staticmethod
    def _import_fused_state(tr, models, opts, global_step: int) -> str | None:
        """A resumed fit: the torch optimizers' restored moments (Adam exp_avg /
        exp_avg_sq, SGD momentum_buffer) and step count continue in the fused engine
        (the parameters came in through init_params); ``global_step`` batches ran.
        Returns None, or why the engine cannot continue this state (the caller refuses
        the engine: the module path under engine='auto', an error under 'fused')."""
        for i, (m, o) in enumerate(zip(models, opts)):
            st = [o.state.get(p, {}) for p in m.parameters()]
            keys = ("exp_avg", "exp_avg_sq") if isinstance(o, torch.optim.Adam) else ("momentum_buffer",)
            for key, dst in zip(keys, (tr.m[i], tr.v[i])):
                if all(s.get(key) is not None for s in st):
                    dst.copy_(torch.cat([s[key].reshape(-1).to(dst) for s in st]))
            steps = [s["step"] for s in st if "step" in s]
            step = int(float(steps[0])) if steps else global_step
            # the persistent engine positions its sampler AND its Adam bias corrections from
            # one step number (host_t0 = tr.t): a restored optimizer that stepped a different
            # number of times than the batches that ran cannot continue bit-exactly there
            if step != global_step:
                return (f"resumed optimizer {i} has step {step} but global_step is {global_step}: the fused "
                        "engine needs one optimizer step per batch")
            tr.step_ctr[i] = step
        tr.t = global_step
        return None

    @staticmethod
    def _export_fused_state(tr, models, opts) -> None:
        """Weights back into the modules and the optimizer state into torch format, so
        checkpoints, hooks and a later module-path fit see the trained state."""
        tr.synchronize()
        for i, (m, o) in enumerate(zip(models, opts)):
            m.load_flat_(tr.model_params(i))
            step = float(tr.step_ctr[i].item())
            off = 0
            for p in m.parameters():
                n = p.numel()
                if isinstance(o, torch.optim.Adam):
                    o.state[p] = {"step": torch.tensor(step), "exp_avg": tr.m[i, off:off + n].view_as(p).clone(),
                                  "exp_avg_sq": tr.v[i, off:off + n].view_as(p).clone()}
                elif o.param_groups[0].get("momentum", 0.0):
                    o.state[p] = {"momentum_buffer": tr.m[i, off:off + n].view_as(p).clone()}
                off += n

    # ------------------------------------------------------------------ validation
    def _val_due(self, epoch: int, batches_done: int, spe: int | None) -> bool:
        """Is a validation epoch due after ``batches_done`` batches of ``epoch`` (of ``spe``)?"""
        if (epoch + 1) % self.check_val_every_n_epoch:
            return False
        if self.val_check_interval is not None:
            return batches_done % self.val_check_interval == 0
        return spe is not None and batches_done == spe

    def _val_next(self, step: int, spe: int) -> int | None:
        """The first global step after ``step`` at which ``_val_due`` holds (epochs of ``spe``
        batches), None if there is none."""
        every = self.check_val_every_n_epoch
        if self.val_check_interval is None:
            return (step // (spe * every) + 1) * spe * every
        vci = self.val_check_interval
        if vci > spe:
            return None
        base = (-(-(step // spe + 1) // every) * every - 1) * spe  # first step of the next validated epoch
        at = base + (max(step - base, 0) // vci + 1) * vci
        return at if at <= base + spe else base + every * spe + vci

    def _val_loader(self, dl):
        """This rank's validation batches: rows ``rank::world`` of the set, unpadded (no
        sample counted twice, unlike a DistributedSampler) -- device slices when the dataset
        has ``device_tensors``, else a strided ``Subset`` behind a DataLoader."""
        ds = getattr(dl, "dataset", dl)
        bs = int(getattr(dl, "batch_size", None) or 1)
        r, w = self.global_rank, self.world_size
        if hasattr(ds, "device_tensors"):
            X, Y = ds.device_tensors(self.device)
            X, Y = X[r::w].contiguous(), Y[r::w].contiguous()
            return [[X[i:i + bs], Y[i:i + bs]] for i in range(0, X.shape[0], bs)]
        if w > 1:
            from torch.utils.data import DataLoader, Subset

            return DataLoader(Subset(ds, range(r, len(ds), w)), batch_size=bs,
                              num_workers=getattr(dl, "num_workers", 0))
        return dl

    def _run_validation(self, model, vloader) -> dict:
        """One validation epoch, eager, outside the captured train graphs: ``model.eval()``
        and ``no_grad``; every value ``validation_step`` logs is reduced to the epoch mean
        weighted by batch size, summed over ranks as (value x size, size).  Returns
        {name: float}, the same on every rank."""
        was_training = model.training
        model.eval()
        sums: dict = {}
        try:
            model.on_validation_epoch_start()
            with torch.no_grad():
                for bi, batch in enumerate(vloader):
                    batch = [b.to(self.device, non_blocking=True) for b in batch]
                    size = int(batch[0].shape[0])
                    model._val_logged = {}
                    with self._autocast():
                        model.validation_step(batch, bi)
                    for k, v in model._val_logged.items():
                        s = sums.setdefault(k, [torch.zeros((), dtype=torch.float64, device=self.device), 0])
                        s[0] += v.to(self.device).double().reshape(-1)[0] * size
                        s[1] += size
        finally:
            model._val_logged = None
            model.train(was_training)
        keys = sorted(sums)
        if self.world_size > 1:  # a rank whose shard is empty logged nothing: agree on the names
            every = [None] * self.world_size
            dist.all_gather_object(every, keys)
            keys = sorted({k for ks in every for k in ks})
        out = {}
        if keys:
            zero = torch.zeros((), dtype=torch.float64, device=self.device)
            buf = torch.stack([sums[k][0] if k in sums else zero for k in keys] +
                              [torch.tensor(float(sums[k][1] if k in sums else 0), dtype=torch.float64,
                                            device=self.device) for k in keys])
            host = comm_util.all_reduce_(buf).cpu().tolist()
            n = len(keys)
            out = {k: host[i] / host[n + i] for i, k in enumerate(keys) if host[n + i] > 0}
        model.on_validation_epoch_end()
        return out

    def _log_validation(self, logger, res: dict) -> None:
        self._val_metrics = dict(res)
        self.callback_metrics = {**self.callback_metrics, **res}
        if res:
            logger.log(self.global_step, res)
            logger.flush()

    def validate(self, model, dataloaders=None, ckpt_path: str | None = None) -> list:
        """One validation epoch of ``model`` over ``dataloaders`` (PL's ``Trainer.validate``):
        a list with one dict of the reduced metrics, also merged into ``callback_metrics``.
        ``ckpt_path``: weights from a checkpoint file (or ``"last"``) first."""
        if not _has_validation_step(model):
            raise RuntimeError("Trainer.validate: the LightningModule defines no validation_step")
        if not hasattr(self, "device"):
            self._setup()
        model.trainer = self
        model.to(self.device)
        path = self._resolve_ckpt(ckpt_path)
        if path is not None:
            model.load_state_dict(torch.load(path, map_location="cpu", weights_only=True)["state_dict"])
        res = self._run_validation(model, self._val_loader(dataloaders))
        self._val_metrics = dict(res)
        self.callback_metrics = {**self.callback_metrics, **res}
        return [res]

    # ------------------------------------------------------------------ checkpoints
    def _ckpt_dir(self) -> Path | None:
        if self._log_dir is None:
            return None
        d = self._log_dir / "checkpoints"
        d.mkdir(exist_ok=True)
        return d

    def _save(self, model, opts, name: str) -> None:
        """Rank-0 atomic save (tmp + rename) of weights, optimizer states and the loop
        position; every rank then waits for it (a barrier), so no rank can run ahead
        into a collective while rank 0 is still writing."""
        self._export_flat_opts()  # torch-format optimizer state of the flat-kernel optimizers
        d = self._ckpt_dir() if self.global_rank == 0 else None
        if d is not None:
            path = d / name
            tmp = path.with_suffix(".tmp")
            torch.save({"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                        "global_step": self.global_step, "epoch": self.current_epoch,
                        "batch_in_epoch": self._batch_in_epoch,
                        "optimizer_states": [_cpu_state(o.state_dict()) for o in opts],
                        "lr_schedulers": [_cpu_state(r["scheduler"].state_dict()) for r in self._sched_recs]}, tmp)
            os.replace(tmp, path)
            self.checkpoint_path = str(path)
        if dist.is_initialized():
            comm_util.barrier()

    def _resolve_ckpt(self, ckpt_path):
        if ckpt_path is None:
            return None
        if ckpt_path != "last":
            return Path(ckpt_path)
        base = Path(self.root) / "lightning_logs"
        cands = sorted(base.glob("version_*/checkpoints/*.ckpt"), key=lambda p: p.stat().st_mtime)
        return cands[-1] if cands else None

    def _restore(self, model, opts, path: Path) -> None:
        ck = torch.load(path, map_location="cpu", weights_only=True)
        model.load_state_dict(ck["state_dict"])
        for o, st in zip(opts, ck["optimizer_states"]):
            o.load_state_dict(st)
        for r, st in zip(self._sched_recs, ck.get("lr_schedulers", [])):
            r["scheduler"].load_state_dict(st)
        self.global_step = int(ck["global_step"])
        self.current_epoch = int(ck["epoch"])
        self._skip_batches = self._batch_in_epoch = int(ck.get("batch_in_epoch", 0))
        self.resumed_from = str(path)
        if self.global_rank == 0:
            rank_print(0, f"resumed from {path} at global_step {self.global_step}")

    # ------------------------------------------------------------------ lr schedulers
    @property
    def lr_schedulers(self) -> list:
        return [r["scheduler"] for r in self._sched_recs]

    def _advance_schedulers(self, done: int, spe, epoch_end: bool = False) -> None:
        """The schedulers due after batch number ``done`` (= global_step once it ran): a
        step-interval one every ``frequency`` batches, after its own optimizer's step; an
        epoch-interval one at the end of every ``frequency``-th epoch (``done`` a multiple
        of the epoch's ``spe`` batches; ``epoch_end``: ``done`` counts epochs instead)."""
        for r in self._sched_recs:
            if _sched_due(r, done, spe, epoch_end):
                if getattr(r["scheduler"], "_step_count", 2) <= 1:
                    # torch warns once, at a scheduler's first step, when its optimizer's own
                    # step() has not run: where the flat kernel or the fused engine steps, it never does
                    with warnings.catch_warnings():
                        warnings.filterwarnings("ignore", message="Detected call of `lr_scheduler.step")
                        r["scheduler"].step()
                else:
                    r["scheduler"].step()

    def _planned_steps(self, spe) -> int | None:
        limits = [self.max_steps] if self.max_steps >= 0 else []
        if self.max_epochs is not None and spe is not None:
            limits.append(self.max_epochs * spe)
        return min(limits) if limits else None

    def _tabulate(self, opts, i: int, t0: int, spe):
        """Optimizer i's rate of every planned step as a tuple indexed by its step count
        (``t0`` steps taken so far; the entries below t0 are never read), from stepping a deep
        copy of its schedulers as the fit will step the real ones.  None: no scheduler, no
        planned length, or something other than ``lr`` moves in the param group."""
        recs = [r for r in self._sched_recs if r["opt"] == i]
        total = self._planned_steps(spe)
        if not recs or total is None or total - self.global_step > _MAX_LR_TABLE or \
                (spe is None and any(r["interval"] == "epoch" for r in recs)):
            return None
        return _tabulate_lr(opts[i], recs, t0, self.global_step, total, spe)

    def _table_flat_opts(self, opts, spe) -> None:
        """Module path: every flat-kernel optimizer whose schedulers tabulate reads its rate
        from a device table by its own step counter -- graph replays included, with no
        recapture; the others keep the per-batch ``refresh()`` of their param group."""
        if not self._sched_recs:
            return
        for i, fo in enumerate(self._flat_opts):
            if fo is None:
                continue
            if fo.cfg.name == "sgd" and self.global_step:
                # torch's SGD keeps no step count: the restored counter only says "not the
                # first step"; the table is indexed by the steps taken, one per batch
                fo.flat.step_ctr.fill_(self.global_step)
            t0 = int(fo.flat.step_ctr[0].item())
            tab = self._tabulate(opts, i, t0, spe)
            self.lr_tables[i] = tab
            if tab is not None:
                fo.set_table(tab, t0)

    def _refresh_flat_opts(self) -> bool:
        """Re-read every flat-kernel optimizer's param group (hooks may change lr, ...).
        True if a hyperparameter changed; an optimizer that left the flat kernel's
        domain hands its state back to torch and runs torch's own step from now on."""
        changed = False
        for i, fo in enumerate(self._flat_opts):
            if fo is None:
                continue
            r = fo.refresh()
            if r is None:
                fo.export_state()
                self._flat_opts[i] = None
                self._opt_zeroes = False  # torch's step leaves its gradient: zero_grad fills again
                changed = True
            else:
                changed |= r
        return changed

    def _export_flat_opts(self) -> None:
        for fo in self._flat_opts:
            if fo is not None:
                fo.export_state()

    def _optimizer_steps(self, model, ddp, opts, batch, batch_idx):
        """One batch: for each optimizer (PL 1.5): toggle, zero_grad, training_step,
        backward, step, untoggle."""
        for oi, opt in enumerate(opts):
            if len(opts) > 1:
                model.toggle_optimizer(opt, oi, opts)
            if ddp is not None:
                ddp.zero_grad()
            else:
                opt.zero_grad(set_to_none=False)
            with self._autocast():
                out = model.training_step(batch, batch_idx, oi) if len(opts) > 1 else \
                    model.training_step(batch, batch_idx)
            loss = out["loss"] if isinstance(out, dict) else out
            flat = self._flat_opts[oi] if oi < len(self._flat_opts) else None
            # one rank (nothing reads the gradient between the backward and the step): the
            # backward's last stage kernel and the flat optimizer step as ONE launch
            fuse = flat is not None and self._fuse_backward_opt and (ddp is None or ddp.world == 1)
            with (ParamBackwardFusion() if fuse else contextlib.nullcontext()) as fus:
                # the seed from a cached tensor of ones (autograd's own would be a fill launch per step)
                loss.backward(self._backward_seed(loss))
                if flat is not None:
                    # the flat kernel zeroes the gradient it consumed: the next zero_grad is free
                    if flat.step(zero_grad=self._opt_zeroes, fused=fus.take() if fus is not None else None) \
                            and ddp is not None:
                        ddp.mark_grad_clean()
                else:
                    self._clip_torch(opt)
                    opt.step()
            if len(opts) > 1:
                model.untoggle_optimizer(oi)
            model._logged[f"train_loss_opt{oi}"] = loss.detach()

    def _clip_fields(self) -> dict:
        """The Trainer's clipping as OptimConfig fields (the flat optimizer kernel clips)."""
        if self.gradient_clip_val <= 0:
            return {}
        key = "max_grad_norm" if self.gradient_clip_algorithm == "norm" else "clip_grad_value"
        return {key: self.gradient_clip_val}

    def _clip_torch(self, opt) -> None:
        """Where torch's own step runs (CPU, optimizers outside the flat kernel's domain):
        torch's clipping over that optimizer's parameters, before its step."""
        if self.gradient_clip_val <= 0:
            return
        params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
        if self.gradient_clip_algorithm == "norm":
            torch.nn.utils.clip_grad_norm_(params, self.gradient_clip_val)
        else:
            torch.nn.utils.clip_grad_value_(params, self.gradient_clip_val)

    def _backward_seed(self, loss: torch.Tensor):
        """d loss / d loss for a scalar loss, cached per (dtype, device); None otherwise."""
        if loss.numel() != 1 or not loss.is_cuda:
            return None
        key = (loss.dtype, loss.device, tuple(loss.shape))
        seeds = self.__dict__.setdefault("_seeds", {})
        t = seeds.get(key)
        if t is None:
            t = seeds[key] = torch.ones_like(loss)
        return t

    def _autocast(self):
        """precision='bf16': torch.autocast around the forward (PL's bf16 plugin); the
        weight-cast cache stays off so a captured hipGraph re-reads the live weights."""
        if self.autocast_dtype is None:
            return contextlib.nullcontext()
        return torch.autocast(self.device.type, dtype=self.autocast_dtype, cache_enabled=False)

    @staticmethod
    def _static_ok(static, batch) -> bool:
        return all(isinstance(b, torch.Tensor) and b.is_cuda for b in batch)

    def _batch_stepper(self, model, ddp, opts):
        """A CapturedStep replaying one batch's optimizer steps as a hipGraph, when the
        run allows it: a GPU, buckets that can be captured (one rank, the in-kernel xGMI
        all-reduce, or RCCL: ``FlatDDP.graph_safe``), and optimizers that can keep
        their step counts on the device (torch's ``capturable`` param-group flag).

        What a replay repeats is what the capture recorded: device work on the static
        batch buffers.  Host-side decisions inside ``training_step`` (e.g. on
        ``batch_idx`` or a Python counter) are frozen at capture time, and a step that
        syncs with the host cannot be captured (that batch shape then runs eagerly);
        ``Trainer(use_graphs=False)`` runs every batch eagerly."""
        if not (self.use_graphs and self.device.type == "cuda"):
            return None, None
        if ddp is not None and not ddp.graph_safe():
            return None, None
        for opt in opts:
            if not all("capturable" in g for g in opt.param_groups) and not isinstance(opt, torch.optim.SGD):
                return None, None
        for opt in opts:
            for g in opt.param_groups:
                if "capturable" in g:
                    g["capturable"] = True
        from ..engine.graph_step import CapturedStep

        static: dict = {}

        def body(gkey):
            sb = static[gkey[0]]  # (batch shape, graph copy)
            if sb.src is not None:  # device batch: the gather is part of the replayed step
                sb.src.gather_into(sb.idx, sb.tensors)
            self._optimizer_steps(model, ddp, opts, sb.tensors, self._cur_batch_idx)

        def abort():
            if getattr(model, "_toggled", None):
                model.untoggle_optimizer(-1)
            if ddp is not None:
                ddp.reset_hooks()
                ddp._grad_clean = False  # the abandoned capture's gradient zeroing never ran

        stepper = CapturedStep(body, self.device, on_abort=abort)
        self._stepper = stepper
        return stepper, static

    def teardown(self):
        if dist.is_initialized():
            comm_util.barrier()
            dist.destroy_process_group()


def _has_validation_step(model) -> bool:
    """Does the module define its own ``validation_step`` (the base class's does nothing)?"""
    from .module import LightningModule

    f = getattr(type(model), "validation_step", None)
    return callable(f) and f is not LightningModule.validation_step


class _StaticBatch:
    """The batch buffers a captured step reads (and, for device batches, the index
    buffer it gathers them with)."""

    __slots__ = ("tensors", "idx", "src")

    def __init__(self, tensors, idx=None, src=None):
        self.tensors, self.idx, self.src = tensors, idx, src


def _cpu_state(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu_state(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu_state(v) for v in x)
    return x


_MAX_LR_TABLE = 1 << 20  # entries of a tabulated scheduler (8 MiB of float64 on the device)


def _parse_optimizers(ret):
    """``configure_optimizers``' Lightning 1.5 forms -> (optimizers, scheduler records): an
    optimizer; a list / tuple of optimizers; ``([optimizers], [schedulers])``; a dict
    ``{"optimizer", "lr_scheduler": scheduler | {"scheduler", "interval", "frequency"}}``; a
    tuple / list of such dicts.  A bare scheduler steps per epoch."""
    Optimizer = torch.optim.Optimizer
    opts, raw = [], []
    if isinstance(ret, Optimizer):
        opts = [ret]
    elif isinstance(ret, dict):
        ret = [ret]
    if isinstance(ret, (list, tuple)) and not opts:
        if len(ret) == 2 and all(isinstance(x, (list, tuple)) for x in ret) and \
                all(isinstance(o, Optimizer) for o in ret[0]):
            opts, raw = list(ret[0]), [{"scheduler": s} if not isinstance(s, dict) else s for s in ret[1]]
        elif all(isinstance(x, dict) for x in ret):
            for d in ret:
                opts.append(d["optimizer"])
                if "monitor" in d:
                    raise NotImplementedError("configure_optimizers: 'monitor' (metric-driven schedulers) is not supported")
                ls = d.get("lr_scheduler")
                if ls is not None:
                    raw.append(ls if isinstance(ls, dict) else {"scheduler": ls})
        elif all(isinstance(x, Optimizer) for x in ret):
            opts = list(ret)
        else:
            raise TypeError("configure_optimizers: an optimizer, a list of optimizers, ([optimizers], [schedulers]), "
                            "a dict with 'optimizer' / 'lr_scheduler', or a tuple of such dicts")
    recs = []
    for d in raw:
        s = d["scheduler"]
        if "monitor" in d:
            raise NotImplementedError("configure_optimizers: 'monitor' (metric-driven schedulers) is not supported")
        if isinstance(s, torch.optim.lr_scheduler.ReduceLROnPlateau):
            raise NotImplementedError("configure_optimizers: ReduceLROnPlateau (a metric-driven scheduler) is not "
                                      "supported")
        interval, freq = d.get("interval", "epoch"), int(d.get("frequency", 1))
        if interval not in ("epoch", "step") or freq < 1:
            raise ValueError(f"lr_scheduler: interval {interval!r} (epoch or step), frequency {freq} (>= 1)")
        own = [i for i, o in enumerate(opts) if o is s.optimizer]
        if not own:
            raise ValueError("lr_scheduler: its optimizer is not among the returned optimizers")
        recs.append({"scheduler": s, "interval": interval, "frequency": freq, "opt": own[0]})
    # stepping order within a batch: the step-interval ones first, then the epoch's end
    recs.sort(key=lambda r: r["interval"] == "epoch")
    return opts, recs


def _sched_due(r, done: int, spe, epoch_end: bool = False) -> bool:
    if epoch_end:
        return r["interval"] == "epoch" and done % r["frequency"] == 0
    if r["interval"] == "step":
        return done % r["frequency"] == 0
    return spe is not None and done % spe == 0 and (done // spe) % r["frequency"] == 0


def _tabulate_lr(opt, recs, t0: int, g0: int, total: int, spe):
    """Step a deep copy of ``opt`` + its schedulers (parameters and state shared, not copied)
    through batches g0 .. total - 1 as ``Trainer._advance_schedulers`` will step the real ones;
    entry t0 + k is the rate of the k-th of them.  None if anything but lr moves (OneCycleLR's
    cycle_momentum), lr is a tensor, there are several param groups, or a scheduler raises."""
    if len(opt.param_groups) != 1 or isinstance(opt.param_groups[0].get("lr"), torch.Tensor):
        return None
    memo = {id(p): p for g in opt.param_groups for p in g["params"]}
    for st in opt.state.values():
        for v in (st.values() if isinstance(st, dict) else ()):
            if isinstance(v, torch.Tensor):
                memo[id(v)] = v
    try:
        o2, s2 = copy.deepcopy((opt, [r["scheduler"] for r in recs]), memo)
    except Exception:  # noqa: BLE001 - a scheduler that cannot be copied is not tabulated
        return None
    rest = lambda o: _group_key(o)[:2] + _group_key(o)[3:]  # noqa: E731 - everything but lr
    key0 = rest(o2)
    vals = []
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "lr_scheduler.step() before optimizer.step()": no step is taken here
            for g in range(g0, total):
                vals.append(float(o2.param_groups[0]["lr"]))
                for r, sc in zip(recs, s2):
                    if _sched_due(r, g + 1, spe):
                        sc.step()
                if rest(o2) != key0:
                    return None
    except Exception:  # noqa: BLE001 - e.g. OneCycleLR stepped past its total_steps
        return None
    if not vals:
        return None
    return tuple([vals[0]] * t0 + vals)


_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "momentum", "dampening", "nesterov", "amsgrad", "maximize",
               "differentiable", "decoupled_weight_decay")


def _group_key(opt):
    g = opt.param_groups[0]
    return (type(opt), len(opt.param_groups)) + tuple(g.get(k) for k in _GROUP_KEYS)


def _optim_config(opt):
    """OptimConfig of a plain Adam/SGD's single param group, or None if the flat kernel
    cannot run it (several groups, tensor lr, amsgrad, nesterov, ...)."""
    from ..ops.optim import OptimConfig

    if len(opt.param_groups) != 1:
        return None
    g = opt.param_groups[0]
    lr = g.get("lr")
    if isinstance(lr, torch.Tensor) or g.get("maximize") or g.get("differentiable"):
        return None
    if type(opt) is torch.optim.Adam:
        if g.get("amsgrad") or g.get("decoupled_weight_decay"):
            return None
        return OptimConfig("adam", float(lr), tuple(float(b) for b in g["betas"]), float(g["eps"]),
                           float(g["weight_decay"]))
    if type(opt) is torch.optim.SGD:
        if g.get("nesterov") or g.get("dampening", 0):
            return None
        return OptimConfig("sgd", float(lr), weight_decay=float(g["weight_decay"]), momentum=float(g["momentum"]))
    return None


class _FlatTorchOptimizer:
    """A user's plain ``torch.optim.Adam`` / ``SGD`` run as ONE flat-optimizer kernel
    (``csrc/optim.hip``, the element-for-element mirror of torch's math) over the span
    of the flat parameter buffer its single param group covers, instead of torch's
    ~5 multi-tensor launches plus per-parameter step bookkeeping.  The moments live
    in flat buffers (imported from ``opt.state`` when the optimizer was restored from
    a checkpoint); ``export_state`` writes them back into ``opt.state`` in torch's own
    format (checkpoints, continued use of the optimizer).  ``refresh`` re-reads the
    param group, so hyperparameter edits between steps (manual LR decay) apply."""

    def __init__(self, opt, params, flat_p, flat_g, cfg, clip: dict | None = None):
        from ..ops.optim import FlatOptimizer

        self.opt = opt
        self.params = params
        # the Trainer's gradient clipping: OptimConfig fields kept over every refresh
        self.clip = dict(clip or {})
        cfg = dataclasses.replace(cfg, **self.clip)
        self.cfg = cfg
        self.flat = FlatOptimizer(flat_p, flat_g, cfg)
        self._key = _group_key(opt)
        # a tabulated scheduler (Trainer._table_flat_opts): the kernel reads table[step counter];
        # host_t mirrors the counter (advanced by the Trainer once per batch, replays included)
        self.table: tuple | None = None
        self.host_t = 0
        self._import_state()

    def _import_state(self):
        st0 = [self.opt.state.get(p) for p in self.params]
        if not any(st0):
            return
        steps = {int(float(st["step"])) if st and "step" in st else 0 for st in st0}
        o = 0
        m, v = self.flat.m.view(-1), self.flat.v.view(-1)
        with torch.no_grad():
            for p, st in zip(self.params, st0):
                n = p.numel()
                if st:
                    if self.cfg.name == "adam":
                        m[o:o + n].copy_(st["exp_avg"].reshape(-1))
                        v[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                    elif st.get("momentum_buffer") is not None:
                        m[o:o + n].copy_(st["momentum_buffer"].reshape(-1))
                o += n
        # SGD keeps no step count in torch: a restored momentum buffer means "not the first step"
        step = max(steps) if self.cfg.name == "adam" else (1 if any(st0) else 0)
        self.flat.step_ctr.fill_(step)
        self.opt.state.clear()  # the flat buffers are the live state until export_state

    def refresh(self):
        """True if the param group's hyperparameters changed (now applied), False if
        not, None if the optimizer no longer fits the flat kernel.  Called every batch:
        an unchanged param group is recognised from a tuple of its entries."""
        key = _group_key(self.opt)
        if key == self._key:
            return False
        if self.table is not None:
            # the scheduler's own move of lr to the table's value is no hyperparameter edit
            lr = self.opt.param_groups[0].get("lr")
            if key[:2] + key[3:] == self._key[:2] + self._key[3:] and not isinstance(lr, torch.Tensor) and \
                    float(lr) == self.table[min(self.host_t, len(self.table) - 1)]:
                self._key = key
                return False
            self.table = None  # an edit from outside the schedule: back to the param group, re-read per batch
        self._key = key
        cfg = _optim_config(self.opt)
        if cfg is None or cfg.name != self.cfg.name:
            return None
        cfg = dataclasses.replace(cfg, **self.clip)
        if cfg == self.cfg:
            return False
        self.cfg = self.flat.cfg = cfg
        return True

    def set_table(self, values, t0: int) -> None:
        from ..ops.schedule import LrSchedule

        self.table, self.host_t = tuple(values), int(t0)
        self.cfg = self.flat.cfg = dataclasses.replace(self.cfg, schedule=LrSchedule.from_values(self.table))
        # the device copy is made here, never during a capture of the step
        self.cfg.schedule.device_table(self.flat.params.device)

    def step(self, zero_grad: bool = False, fused=None) -> bool:
        return self.flat.step(zero_grad=zero_grad, fused=fused)

    def export_state(self):
        step = int(self.flat.step_ctr[0].item())
        if step == 0:
            return
        group = self.opt.param_groups[0]
        o = 0
        m, v = self.flat.m.view(-1), self.flat.v.view(-1)
        for p in self.params:
            n = p.numel()
            st = self.opt.state[p]
            if self.cfg.name == "adam":
                cap = bool(group.get("capturable", False))
                st["step"] = torch.tensor(float(step), dtype=torch.float32, device=p.device if cap else "cpu")
                st["exp_avg"] = m[o:o + n].view_as(p).clone()
                st["exp_avg_sq"] = v[o:o + n].view_as(p).clone()
            elif self.cfg.momentum:
                st["momentum_buffer"] = m[o:o + n].view_as(p).clone()
            o += n


def _flat_optimizer_for(opt, ddp, clip: dict | None = None):
    """_FlatTorchOptimizer for ``opt`` if it is a plain Adam/SGD whose one param group
    is a contiguous span of the flat buffers on a GPU, else None (torch's step runs)."""
    from ..ops.mlp import _flat_view_of

    if ddp is None or not ddp.flat_params.is_cuda:
        return None
    cfg = _optim_config(opt)
    if cfg is None:
        return None
    params = list(opt.param_groups[0]["params"])
    if not params or any(p.dtype != torch.float32 or p.grad is None for p in params):
        return None
    flat_p = _flat_view_of([p.data for p in params])
    flat_g = _flat_view_of([p.grad for p in params])
    if flat_p is None or flat_g is None:
        return None
    return _FlatTorchOptimizer(opt, params, flat_p, flat_g, cfg, clip)

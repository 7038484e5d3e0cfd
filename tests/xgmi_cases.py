"""The exchanges of several ranks on one GPU: the payloads and the exact CPU reference of the
stand-alone all-reduce (``csrc/xgmi_allreduce.hip``), and the rank function that one spawn per
world size runs for ``tests/test_xgmi_matrix_gpu.py`` (the cells themselves: ``tests/step_cases.py``).

**Stand-alone all-reduce.**  The kernel's contract: per element the fp32 sum of the ranks'
values in rank order from +0, then one multiply by ``scale`` -- no product feeds an addition,
so there is no fma to contract, and the CPU loop ``s = 0; for r: s = s + x_r; s * scale`` in fp32
(:func:`ar_reference`) gives the same bits.  One object of capacity ``AR_CAP`` = 4100 floats
(5 workgroups of 1024, the last of 4 floats) serves the calls of ``AR_SIZES`` in order: a short
call leaves the granules beyond its size at an older epoch of the same parity, which a later
long call has to read over; 11 calls use both parities in every workgroup's own count.

Payloads by call (:func:`ar_payload`): integer-valued floats in [-2^15, 2^15] with ``scale``
2^-3 (exact in any order; also compared with the int64 sum), normal draws scaled per element
by 2^-20 .. 2^20 with ``scale = 1 / W``, and one full-size call of the latter with +-inf, -0.0
and NaN planted at fixed positions (:func:`ar_specials`).  No denormal inputs: the kernels'
flush mode is not a contract.  On every other call one rank arrives late
(``torch.cuda._sleep``), a different one each time, the highest first.
"""
from __future__ import annotations

import os
import traceback

import torch

AR_CAP = 4100
AR_SIZES = [AR_CAP, 1, 3, 4, 5, AR_CAP, 1023, 1024, 1025, 4097, AR_CAP]
AR_SPECIAL_CALL = 5
AR_WORLDS = (3, 5, 8)
INT_SCALE = 2.0 ** -3


def ar_kind(call: int) -> str:
    return "int" if call % 2 == 0 else "normal"


def ar_scale(world: int, call: int) -> float:
    return INT_SCALE if ar_kind(call) == "int" else 1.0 / world


def ar_late_rank(world: int, call: int) -> int | None:
    """The rank that queues a delay before its call: on the even calls, the highest rank first."""
    return (world - 1 - call // 2) % world if call % 2 == 0 else None


def ar_specials(world: int) -> list[tuple[int, int, float]]:
    """(position, rank, value) of the planted values of call AR_SPECIAL_CALL."""
    inf, nan, top = float("inf"), float("nan"), world - 1
    out = [(0, 0, inf),                                  # inf + finite
           (1, 0, inf), (1, top, -inf),                  # inf - inf = NaN
           (3, 1, nan),                                  # NaN from a middle slot
           (7, top, -inf),                               # the highest slot (got[r][3], mask bit 4 r + 3)
           (1030, top, nan),                             # the second workgroup
           (AR_CAP - 1, 0, inf), (AR_CAP - 2, top, nan)]  # the last workgroup's 4 floats
    out += [(2, r, -0.0) for r in range(world)]          # +0 + -0 ... = +0, as in the CPU loop
    out += [(5, r, -0.0) for r in range(1, world)]       # -0 after a finite value
    return out


def ar_payload(world: int, rank: int, call: int) -> torch.Tensor:
    """Rank ``rank``'s input of call ``call`` (CPU fp32, AR_SIZES[call] floats)."""
    n = AR_SIZES[call]
    g = torch.Generator().manual_seed(7919 * call + 31 * rank + world)
    if ar_kind(call) == "int":
        return torch.randint(-(1 << 15), (1 << 15) + 1, (n,), generator=g).float()
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 21, (n,), generator=g).float())
    if call == AR_SPECIAL_CALL:
        for pos, r, v in ar_specials(world):
            if r == rank:
                x[pos] = v
    return x


def ar_reference(xs: list[torch.Tensor], scale: float) -> torch.Tensor:
    """``s = 0; for r: s = s + x_r; s * scale`` in fp32."""
    s = torch.zeros_like(xs[0])
    for x in xs:
        s = s + x
    return s * torch.tensor(scale, dtype=torch.float32)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal bit for bit outside NaN, and NaN at the same positions (a NaN's payload bits are
    not a contract)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)))


def ar_calls(rank: int, world: int, device) -> list[torch.Tensor]:
    """The calls of AR_SIZES on one XgmiAllReduce; the outputs as CPU tensors."""
    from distributed_training_pytorch_amd.parallel.xgmi import XgmiAllReduce

    ar = XgmiAllReduce(AR_CAP, device)
    outs = []
    try:
        for c in range(len(AR_SIZES)):
            t = ar_payload(world, rank, c).to(device)
            if ar_late_rank(world, c) == rank:
                torch.cuda._sleep(2_000_000)
            ar.all_reduce_(t, scale=ar_scale(world, c))
            outs.append(t.cpu())
        torch.cuda.synchronize(device)
        ar.check()
    finally:
        import torch.distributed as dist

        dist.barrier()  # no rank unmaps its buffer under a peer's stores
        ar.close()
    return outs


def graph_vs_persistent(cell, device, rank: int, steps: int = 7) -> dict:
    """``steps`` steps of the cell with launch="graph" and with launch="persistent"
    (steps_per_launch = 4: one captured graph of 4, then one-step launches): parameters and losses."""
    import torch.distributed as dist

    from . import step_cases as sc

    out = {}
    for launch in ("graph", "persistent"):
        tr = sc.make_trainer(cell, device, rank=rank, launch=launch, steps_per_launch=4)
        try:
            out[launch + "_comm"] = (tr.comm, tr.comm_fallback_reason, [tr.lanes, tr.kernel_waves, tr.groups])
            dist.barrier()
            tr.train(steps)
            tr.synchronize()
            out[launch] = (tr.params.detach().cpu().clone(), tr.losses(0, steps).clone())
        finally:
            tr.close()
    return out


def world_rank(rank: int, world: int, cell_ids: list[str], env: tuple = (), with_ar: bool = False,
               with_graph: bool = False) -> dict:
    """What one spawn runs on every rank, in order: the stand-alone all-reduce calls, the cells,
    the graph-replay check.  The first item that raises ends the spawn on every rank (the ranks
    agree after each item): it is recorded under "stopped", later items are absent.  Nothing is
    retried."""
    for k, v in env:  # read once per process, when the library first picks an instance
        os.environ[k] = v
    from . import step_cases as sc

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"ar": None, "cells": {}, "graph": None, "stopped": None}

    def item(name, fn):
        err = None
        try:
            fn()
        except Exception:
            err = f"{name} on rank {rank}:\n{traceback.format_exc()}"
        if not sc._all_ranks(err is None):
            out["stopped"] = err or f"{name}: a peer raised"
            return False
        return True

    def do_ar():
        out["ar"] = ar_calls(rank, world, dev)

    def do_graph():
        out["graph"] = graph_vs_persistent(sc.XGMI_GRAPH_CELL, dev, rank)

    if with_ar and not item("the stand-alone all-reduce", do_ar):
        return out
    for cid in cell_ids:
        def do_cell(cid=cid):
            o = out["cells"][cid] = sc.run_cell_rank(sc.BY_ID[cid], dev)
            if o["fails"] or o["comm"] != "xgmi" or tuple(o["pick"]) != sc.BY_ID[cid].expect:
                raise RuntimeError(f"{cid}: {o['fails'] or (o['comm'], o['fallback'], o['pick'])}")

        if not item(cid, do_cell):
            return out
    if with_graph:
        item("graph against persistent", do_graph)
    return out

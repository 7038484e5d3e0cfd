#!/usr/bin/env python3
"""Instruction counts of a kernel's step loop, per barrier-delimited segment and per class.

Usage: python scripts/step_loop_stats.py FILE.s KERNEL_SUBSTRING [--json]

FILE.s is what ``build.asm("mlp_train_lanes.hip")`` (or ``"mlp_train_one.hip"``) writes.  The step loop is the largest span
of the kernel closed by a backward branch (a branch whose target label stands above it).
A segment ends with its ``s_barrier``; what follows the last barrier is the tail.
Instructions are classified by mnemonic prefix only (first match wins):

    MFMA     v_mfma                         LDS      ds_
    lane     v_readlane / v_writelane /     VMEM     buffer_ / global_
             v_readfirstlane                wait     s_waitcnt
    AGPR     v_accvgpr                      nop      s_nop
    VALU     every other v_                 barrier  s_barrier
    branch   s_branch / s_cbranch           SALU     every other s_

The counts are static: a listing says nothing about how often a path runs.
"""
from __future__ import annotations

import collections
import json
import re
import sys

CLASSES = ("VALU", "MFMA", "lane", "AGPR", "LDS", "VMEM", "wait", "nop", "barrier", "branch", "SALU", "other")
_PREFIX = (("v_mfma", "MFMA"), ("v_readlane", "lane"), ("v_writelane", "lane"), ("v_readfirstlane", "lane"),
           ("v_accvgpr", "AGPR"), ("v_", "VALU"), ("ds_", "LDS"), ("buffer_", "VMEM"), ("global_", "VMEM"),
           ("s_waitcnt", "wait"), ("s_nop", "nop"), ("s_barrier", "barrier"), ("s_branch", "branch"),
           ("s_cbranch", "branch"), ("s_", "SALU"))
_LABEL = re.compile(r"^([.\w$]+):")
_KERNEL = re.compile(r"^(\S+):\s*; @", re.M)


def classify(op: str) -> str:
    for pre, cls in _PREFIX:
        if op.startswith(pre):
            return cls
    return "other"


def kernel_body(text: str, pat: str) -> tuple[str, list[str]]:
    """(symbol, lines) of the first kernel whose symbol contains ``pat``"""
    for m in _KERNEL.finditer(text):
        if pat in m.group(1):
            start = text.find("\n", m.end())
            end = text.find(".Lfunc_end", start)
            return m.group(1), text[start:end if end >= 0 else len(text)].split("\n")
    raise SystemExit(f"no kernel matching {pat!r}")


def parse(lines: list[str]) -> tuple[list[tuple[str, str]], dict[str, int]]:
    """instructions as (mnemonic, first operand) and label -> index of the next instruction"""
    ins, labels = [], {}
    for raw in lines:
        ln = raw.split(";", 1)[0].strip()
        if not ln:
            continue
        m = _LABEL.match(ln)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if ln.startswith("."):
            continue
        tok = ln.replace(",", " ").split()
        ins.append((tok[0], tok[1] if len(tok) > 1 else ""))
    return ins, labels


def step_loop(ins, labels) -> tuple[int, int]:
    """[first, last] instruction index of the largest span closed by a backward branch.  A
    span reaches to the last backward branch into it: a block the compiler laid out behind
    the loop's own back edge (a cold path that jumps back into the loop) belongs to it."""
    back = [(labels[arg], i) for i, (op, arg) in enumerate(ins)
            if classify(op) == "branch" and arg in labels and labels[arg] <= i]
    best = None
    for lo in sorted({t for t, _ in back}):
        hi = lo
        while True:
            ext = max((i for t, i in back if lo <= t <= hi and i > hi), default=hi)
            if ext == hi:
                break
            hi = ext
        if best is None or hi - lo > best[1] - best[0]:
            best = (lo, hi)
    if best is None:
        raise SystemExit("no backward branch: no loop in this kernel")
    return best


def stats(text: str, pat: str) -> dict:
    name, lines = kernel_body(text, pat)
    ins, labels = parse(lines)
    lo, hi = step_loop(ins, labels)
    segs = [collections.Counter()]
    for op, _ in ins[lo:hi + 1]:
        cls = classify(op)
        segs[-1][cls] += 1
        if cls == "barrier":
            segs.append(collections.Counter())
    total = collections.Counter()
    for s in segs:
        total.update(s)
    return {"kernel": name, "kernel_instructions": len(ins), "loop_instructions": hi - lo + 1,
            "segments": [{"instructions": sum(s.values()), **{c: s[c] for c in CLASSES if s[c]}} for s in segs],
            "classes": {c: total[c] for c in CLASSES if total[c]},
            "branches_seg2_4": sum(s["branch"] for s in segs[1:4])}


def main(argv: list[str]) -> int:
    args = [a for a in argv if a != "--json"]
    if len(args) != 2:
        print(__doc__)
        return 2
    st = stats(open(args[0]).read(), args[1])
    if "--json" in argv:
        print(json.dumps(st))
        return 0
    print(f"{st['kernel']}\n  kernel {st['kernel_instructions']} instructions, step loop {st['loop_instructions']}")
    n = len(st["segments"])
    print("  " + "segment".ljust(9) + "".join(c.rjust(8) for c in ("all",) + CLASSES))
    for i, s in enumerate(st["segments"]):
        tag = "tail" if i == n - 1 and n > 1 else str(i + 1)
        print("  " + tag.ljust(9) + str(s["instructions"]).rjust(8) + "".join(str(s.get(c, 0)).rjust(8) for c in CLASSES))
    print("  " + "loop".ljust(9) + str(st["loop_instructions"]).rjust(8)
          + "".join(str(st["classes"].get(c, 0)).rjust(8) for c in CLASSES))
    print(f"  branches in segments 2-4: {st['branches_seg2_4']}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

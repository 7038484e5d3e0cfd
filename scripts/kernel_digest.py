#!/usr/bin/env python3
"""Digests of the kernels in a device assembly listing, to tell whether two builds of a
source produced the same device code.

Usage: python scripts/kernel_digest.py [--mask-ordinals] FILE.s
       python scripts/kernel_digest.py --diff A.s B.s
       python scripts/kernel_digest.py --mask-ordinals --diff A1.s [A2.s ...] -- B1.s [B2.s ...]

FILE.s is what ``build.asm("mlp_train_one.hip")`` writes (``hipcc --cuda-device-only -S``).
The only thing masked is the ``__hip_cuid_<hex>`` symbol, a hash of the source file.  One
line ``sha256  symbol`` per kernel covers the text from the kernel's label through its
``.end_amdhsa_kernel`` (the body and the kernel descriptor: registers, LDS size); the last
line, symbol ``*``, covers the whole masked file (device functions, metadata and the order
of everything included).  ``--diff`` lists the kernels that stand in one listing only or
differ, and exits 1 if the masked files differ anywhere.

``--mask-ordinals`` also replaces N in the basic-block labels ``.LBB<N>_<k>``, and in the
loop comments that name them (``Header=BB<N>_<k>``), by a fixed token (and the padding between such a label and its comment, which
shrinks when N gains a digit, by one space): N is the ordinal of the function in its listing, so a kernel that moved to another
place or another source keeps its digest when no instruction changed.  In that mode
``--diff`` takes several listings per side and compares the kernels' digests only (the
whole-file digest means nothing across a split).

Text is hashed and compared; no instruction is looked at.
"""
from __future__ import annotations

import hashlib
import re
import sys

_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
_KERNEL = re.compile(r"^(\S+):\s*; @", re.M)
_END = ".end_amdhsa_kernel"
_LBB = re.compile(r"(\.L|\b)BB\d+_(?=\d)")
_LBB_PAD = re.compile(r"^(\.LBB\d+_\d+:)[ \t]+;", re.M)  # the comment column moves with the digits of N


def _sha(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()


def digests(text: str, mask_ordinals: bool = False) -> tuple[dict[str, str], str]:
    """({kernel symbol: sha256}, sha256 of the whole file), the cuid symbol masked"""
    text = _CUID.sub("__hip_cuid_", text)
    if mask_ordinals:
        text = _LBB.sub(r"\1BBN_", _LBB_PAD.sub(r"\1 ;", text))
    heads = list(_KERNEL.finditer(text))
    out = {}
    for m, nxt in zip(heads, heads[1:] + [None]):
        end = text.find(_END, m.start(), nxt.start() if nxt else len(text))
        if end >= 0 and f".amdhsa_kernel {m.group(1)}\n" in text[m.start():end]:  # a kernel, not a device function
            out[m.group(1)] = _sha(text[m.start():end + len(_END)])
    return out, _sha(text)


def diff(a: str, b: str) -> list[str]:
    """one line per kernel in one listing only or differing, one for a difference elsewhere"""
    (ka, fa), (kb, fb) = digests(a), digests(b)
    out = [f"only in A  {k}" for k in ka if k not in kb] + [f"only in B  {k}" for k in kb if k not in ka]
    out += [f"differs    {k}" for k in ka if k in kb and ka[k] != kb[k]]
    if fa != fb and not out:
        out.append("differs    * (outside the kernels)")
    return out


def diff_kernels(a: list[str], b: list[str]) -> list[str]:
    """diff() of the kernels of several listings per side, function ordinals masked"""
    ka, kb = ({k: h for t in side for k, h in digests(t, True)[0].items()} for side in (a, b))
    out = [f"only in A  {k}" for k in ka if k not in kb] + [f"only in B  {k}" for k in kb if k not in ka]
    return out + [f"differs    {k}" for k in ka if k in kb and ka[k] != kb[k]]


def main(argv: list[str]) -> int:
    mask = "--mask-ordinals" in argv
    argv = [x for x in argv if x != "--mask-ordinals"]
    if mask and argv[:1] == ["--diff"] and argv.count("--") == 1 and argv[1] != "--" and argv[-1] != "--":
        i = argv.index("--")
        lines = diff_kernels([open(f).read() for f in argv[1:i]], [open(f).read() for f in argv[i + 1:]])
        print("\n".join(lines) if lines else "identical")
        return 1 if lines else 0
    if mask and argv[:1] == ["--diff"]:
        print(__doc__)
        return 2
    if len(argv) == 3 and argv[0] == "--diff":
        lines = diff(open(argv[1]).read(), open(argv[2]).read())
        print("\n".join(lines) if lines else "identical")
        return 1 if lines else 0
    if len(argv) != 1 or argv[0].startswith("-"):
        print(__doc__)
        return 2
    kernels, whole = digests(open(argv[0]).read(), mask)
    for k, h in kernels.items():
        print(f"{h}  {k}")
    print(f"{whole}  *")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

#!/usr/bin/env python3
"""Digests of the kernels in a device assembly listing, to tell whether two builds of a
source produced the same device code.

Usage: python scripts/kernel_digest.py FILE.s
       python scripts/kernel_digest.py --diff A.s B.s

FILE.s is what ``build.asm("mlp_train.hip")`` writes (``hipcc --cuda-device-only -S``).
The only thing masked is the ``__hip_cuid_<hex>`` symbol, a hash of the source file.  One
line ``sha256  symbol`` per kernel covers the text from the kernel's label through its
``.end_amdhsa_kernel`` (the body and the kernel descriptor: registers, LDS size); the last
line, symbol ``*``, covers the whole masked file (device functions, metadata and the order
of everything included).  ``--diff`` lists the kernels that stand in one listing only or
differ, and exits 1 if the masked files differ anywhere.

Text is hashed and compared; no instruction is looked at.
"""
from __future__ import annotations

import hashlib
import re
import sys

_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
_KERNEL = re.compile(r"^(\S+):\s*; @", re.M)
_END = ".end_amdhsa_kernel"


def _sha(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()


def digests(text: str) -> tuple[dict[str, str], str]:
    """({kernel symbol: sha256}, sha256 of the whole file), the cuid symbol masked"""
    text = _CUID.sub("__hip_cuid_", text)
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


def main(argv: list[str]) -> int:
    if len(argv) == 3 and argv[0] == "--diff":
        lines = diff(open(argv[1]).read(), open(argv[2]).read())
        print("\n".join(lines) if lines else "identical")
        return 1 if lines else 0
    if len(argv) != 1 or argv[0].startswith("-"):
        print(__doc__)
        return 2
    kernels, whole = digests(open(argv[0]).read())
    for k, h in kernels.items():
        print(f"{h}  {k}")
    print(f"{whole}  *")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library, kernel by kernel.

    python tools/kernel_diff.py LIB_A LIB_B

For a refactor of host-side or template plumbing (csrc/conv_halo.h, conv_tiles.h): the embedded code
objects of both libraries are disassembled and split per symbol; the two builds must hold the same
symbols with the same instruction streams.  Addresses are not compared -- a change in instantiation
order moves functions within ``.text`` without changing any of them -- so branch targets are read as
symbol + offset, and the filler after a section's last function is dropped (``...``, or zero words
that disassemble as ``v_cndmask_b32_e32 v0, s0, v0, vcc``).

Prints the number of symbols compared and the number that differ (with the first differing line of
each); exit status 1 when the sets or any stream differ.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_dma_waits import LLVM, code_objects  # noqa: E402

_SYM = re.compile(r"^(?:[0-9a-f]+ )?<(.+)>:$")
_FILLER = ("v_cndmask_b32_e32 v0, s0, v0, vcc", "s_code_end", "s_nop 0")     # a zero word; the assembler's padding


def functions(lib: str) -> dict[str, list[tuple[str, ...]]]:
    """{symbol: its instruction streams, sorted} over every code object embedded in ``lib`` (a symbol local
    to several translation units has one stream per unit)."""
    out: dict[str, list[list[str]]] = {}
    for co in code_objects(lib):
        with tempfile.TemporaryDirectory() as d:
            f = os.path.join(d, "co")
            with open(f, "wb") as fh:
                fh.write(co)
            dis = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", f],
                                 check=True, capture_output=True, text=True).stdout
        cur = None
        for line in dis.splitlines():
            m = _SYM.match(line)
            if m:
                cur = []
                out.setdefault(m.group(1), []).append(cur)
                continue
            line = line.split("//")[0].strip()          # the address comment
            if cur is not None and line and line != "...":
                cur.append(line)
    for streams in out.values():
        for s in streams:
            while s and s[-1] in _FILLER:
                s.pop()
    return {name: sorted(tuple(s) for s in streams) for name, streams in out.items()}


def main(argv) -> int:
    if len(argv) != 2:
        print(__doc__)
        return 2
    a, b = functions(argv[0]), functions(argv[1])
    for name in sorted(set(a) ^ set(b)):
        print(f"only in {argv[0] if name in a else argv[1]}: {name}")
    common = sorted(set(a) & set(b))
    differing = [name for name in common if a[name] != b[name]]
    for name in differing:
        x, y = (" ; ".join(s) for s in (a[name][0], b[name][0])) if len(a[name]) == len(b[name]) == 1 else ("", "")
        i = next((k for k, (p, q) in enumerate(zip(x, y)) if p != q), 0)
        print(f"differs: {name} ({[len(s) for s in a[name]]} vs {[len(s) for s in b[name]]} instructions)"
              + (f"\n    {x[max(0, i - 60):i + 60]}\n    {y[max(0, i - 60):i + 60]}" if x else ""))
    kernels = sum(len(a[name]) for name in common)
    print(f"{kernels} kernels and device functions compared ({len(common)} symbols), {len(differing)} differ, "
          f"{len(set(a) ^ set(b))} in one library only")
    return 1 if differing or set(a) != set(b) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

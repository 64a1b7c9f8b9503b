#!/usr/bin/env python3
"""Kernel-for-kernel comparison of two builds' libraries (diagnostic): which kernels kept their instruction stream.

    python tools/compare_digests.py OLD_LIB_DIR [NEW_LIB_DIR]      # NEW defaults to pika-zoo_amd/lib

For every libpikazoo_*.so of either directory: every kernel's digest (tools/kernel_digest.py: the SHA-256 of its
disassembled instruction texts) in both builds, one line per kernel -- `same`, `MOVED` (with both digests and instruction
counts), `only old` or `only new` -- and a summary line per library.  Exit status 1 when a kernel of a library that both
builds hold moved or disappeared.
"""
import sys
from pathlib import Path

import kernel_digest

REPO = Path(__file__).resolve().parent.parent


def main():
    old = Path(sys.argv[1])
    new = Path(sys.argv[2]) if len(sys.argv) > 2 else REPO / "pika-zoo_amd" / "lib"
    names = sorted({p.name for d in (old, new) for p in d.glob("libpikazoo_*.so")})
    bad = 0
    for name in names:
        if not (old / name).exists() or not (new / name).exists():
            side = "new" if (new / name).exists() else "old"
            table = kernel_digest.kernels((new if side == "new" else old) / name)
            kernels = sorted(k for k in table if not k.endswith(".kd"))
            print(f"{name}: only in the {side} build, {len(kernels)} kernels")
            for k in kernels:
                print(f"    only {side}  {table[k][0]}  {table[k][1]:6d}  {k}")
            continue
        a, b = kernel_digest.kernels(old / name), kernel_digest.kernels(new / name)
        moved = 0
        lines = []
        for k in sorted(set(a) | set(b)):
            if k.endswith(".kd"):
                continue
            if k not in b:
                lines.append(f"    only old  {a[k][0]}  {a[k][1]:6d}  {k}")
                moved += 1
            elif k not in a:
                lines.append(f"    only new  {b[k][0]}  {b[k][1]:6d}  {k}")
                moved += 1
            elif a[k] != b[k]:
                lines.append(f"    MOVED     {a[k][0]} {a[k][1]:6d} -> {b[k][0]} {b[k][1]:6d}  {k}")
                moved += 1
            else:
                lines.append(f"    same      {a[k][0]}  {a[k][1]:6d}  {k}")
        print(f"{name}: {len(lines)} kernels, {len(lines) - moved} with the same digest, {moved} moved / added / removed")
        print("\n".join(lines))
        bad += moved
    print(f"kernels of shared libraries that moved: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

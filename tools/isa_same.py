#!/usr/bin/env python3
"""Did a source change leave the existing kernels alone?  Compares two `hipcc -S` listings of one .hip file (before / after)
kernel by kernel: every kernel of the first must have a kernel in the second with the same instructions, whatever it is called
now (labels, symbol names and assembler directives aside -- a template parameter or an appended empty argument renames a
kernel and changes its kernarg size without touching its code).  What remains is printed: for the RAGGED instantiations of
DESIGN.md 5.3e that is, in the kernels that read the grid size, the offset of one implicit-argument load.
  hipcc <the flags of rfnet_amd/build.py> --cuda-device-only -S rfnet_amd/csrc/X.hip -o after.s   (and the same at the parent)
  python tools/isa_same.py before.s after.s"""
import difflib
import re
import sys


def kernels(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
                continue
            code = ln.split(";")[0].rstrip()
            if not code.strip() or code.strip().startswith("."):
                continue
            out[cur].append(re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", code)))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bodies = {tuple(v) for v in b.values()}
    changed = 0
    for name, body in sorted(a.items()):
        if tuple(body) in bodies:
            continue
        changed += 1
        near = min((k for k in b if len(b[k]) == len(body)), default=None,
                   key=lambda k: sum(x != y for x, y in zip(b[k], body)))
        print("CHANGED", name)
        if near:
            for ln in difflib.unified_diff(body, b[near], lineterm="", n=0):
                if not ln.startswith(("---", "+++", "@@")):
                    print("   ", ln)
    print(f"{len(a)} kernels before, {len(b)} after, {changed} without an identical body")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())

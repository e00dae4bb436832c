#!/usr/bin/env python3
"""Are the kernels of two sets of gfx950 device assembly files the same code?

  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S x.hip -o x.s
  python tools/isa_diff.py old.s new.s [old2.s new2.s ...]

The files are taken in (old, new) pairs; a kernel is looked up by its mangled
name in the union of each side, so a kernel may move from one translation unit
to another (`-` stands for no file where one side has fewer). Per kernel it compares text only: the instruction lines after
stripping `;` comments and whitespace and replacing the translation-unit-local
label numbers (.LBB18_3 -> .LBB_3, .Ltmp / .LJTI likewise), and the kernel's
.amdhsa_* descriptor lines (registers, LDS, scratch). Reports missing and added
kernels and the kernels whose text or descriptor differs; exit status 1 if any.
"""
import re
import sys

from isa_count import kernels

_LABEL = re.compile(r"\.(LBB|Ltmp|LJTI|Lfunc_begin|Lfunc_end)\d+")


def normalize(body):
    out = []
    for line in body:
        s = line.split(";", 1)[0]
        s = " ".join(s.split())
        if s:
            out.append(_LABEL.sub(lambda m: "." + m.group(1), s))
    return out


def descriptors(path):
    """mangled name -> its .amdhsa_* lines"""
    out, cur = {}, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None and s.startswith(".amdhsa_"):
            cur.append(" ".join(s.split(";", 1)[0].split()))
    return out


def load(paths):
    text, desc = {}, {}
    for p in paths:
        if p == "-":
            continue
        for name, body in kernels(p):
            text[name] = normalize(body)
        desc.update(descriptors(p))
    return text, desc


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    n = min(len(a), len(b))
    return n, (a[n] if n < len(a) else "<end>"), (b[n] if n < len(b) else "<end>")


def compare(old_paths, new_paths):
    """-> (missing, added, differing) lists; differing holds (name, why) pairs"""
    ot, od = load(old_paths)
    nt, nd = load(new_paths)
    missing = sorted(set(ot) - set(nt))
    added = sorted(set(nt) - set(ot))
    differing = []
    for name in sorted(set(ot) & set(nt)):
        if ot[name] != nt[name]:
            i, x, y = first_diff(ot[name], nt[name])
            differing.append((name, f"text: {len(ot[name])} -> {len(nt[name])} lines, first at {i}: `{x}` -> `{y}`"))
        elif od.get(name) != nd.get(name):
            i, x, y = first_diff(od.get(name, []), nd.get(name, []))
            differing.append((name, f"descriptor: `{x}` -> `{y}`"))
    return missing, added, differing


def main():
    args = sys.argv[1:]
    if len(args) < 2 or len(args) % 2:
        sys.exit(__doc__)
    missing, added, differing = compare(args[0::2], args[1::2])
    for n in missing:
        print("missing  ", n)
    for n in added:
        print("added    ", n)
    for n, why in differing:
        print("differs  ", n, "--", why)
    print(f"{len(missing)} missing, {len(added)} added, {len(differing)} differing")
    return 1 if missing or added or differing else 0


if __name__ == "__main__":
    sys.exit(main())

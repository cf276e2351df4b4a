#!/usr/bin/env python3
"""Diff two device-assembly files (hipcc --cuda-device-only -S) kernel by kernel.

usage: compare_kernel_asm.py parent.s new.s [--map FILE] [--show N]

Kernels are the symbols with an .amdhsa_kernel block.  A kernel of the parent is compared with the kernel of the same symbol in
the new file, or with the one FILE names for it (lines "parent_symbol new_symbol": template arguments that changed their spelling).
Per pair: instruction count, whether the opcode histograms are equal, and the number of positions at which the normalised
instruction text differs - comments and directives stripped, labels kept (their function index removed, since it counts the
kernels before this one), the kernel's own symbol replaced by <self>.  Up to N differing positions are printed with both texts
and with whether an s_barrier lies on both sides of them (the body of a barrier-delimited loop step).
Exit status 1 when a pair differs in count or histogram, or a kernel has no counterpart that --map does not declare gone ("-")."""
import argparse
import collections
import re
import sys


def kernels(path):
    lines = open(path, errors="replace").read().splitlines()
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = collections.OrderedDict()
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        body = []
        for l in lines[start + 1:]:
            if re.match(r"^\.Lfunc_end\d+:", l):
                break
            l = l.split(";", 1)[0].strip()
            if not l or (l.startswith(".") and not l.endswith(":")):
                continue
            l = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", l).replace(name, "<self>")
            body.append(re.sub(r"\s+", " ", l))
        out[name] = body
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--map")
    ap.add_argument("--show", type=int, default=8)
    a = ap.parse_args()
    rename = {}
    if a.map:
        for l in open(a.map):
            if l.strip() and not l.startswith("#"):
                old, new = l.split()
                rename[old] = new
    pk, nk = kernels(a.parent), kernels(a.new)
    bad = 0
    seen = set()
    for name, pb in pk.items():
        other = rename.get(name, name)
        if other == "-":
            print(f"gone  {len(pb):6d} instr | {name}")
            continue
        if other not in nk:
            print(f"MISSING in new | {name}")
            bad = 1
            continue
        seen.add(other)
        nb = nk[other]
        is_op = lambda s: not s.endswith(":")
        hist_eq = collections.Counter(s.split()[0] for s in pb if is_op(s)) == collections.Counter(s.split()[0] for s in nb if is_op(s))
        diff = [i for i in range(min(len(pb), len(nb))) if pb[i] != nb[i]]
        ndiff = len(diff) + abs(len(pb) - len(nb))
        ok = len(pb) == len(nb) and hist_eq
        bad |= not ok
        print(f"{'same ' if ok and not ndiff else ('order' if ok else 'DIFF ')} instr {len(pb):6d} / {len(nb):6d}  histogram {'=' if hist_eq else '!='}  "
              f"positions differing {ndiff:5d} | {name}" + (f" -> {other}" if other != name else ""))
        bar = [i for i, s in enumerate(pb) if s.startswith("s_barrier")]
        for i in diff[:a.show]:
            inside = bool(bar) and bar[0] < i < bar[-1]
            print(f"        @{i}{' (between barriers)' if inside else ''}: {pb[i]}   |   {nb[i]}")
    for name in nk:
        if name not in seen:
            print(f"ONLY in new | {name}")
            bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main())

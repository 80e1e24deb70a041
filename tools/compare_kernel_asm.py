#!/usr/bin/env python3
"""Compares two gfx950 assembly files of one translation unit function by function:

    hipcc $(GPUFLAGS) --cuda-device-only -S csrc/pg_kernels.hip -o a.s      (at two commits)
    python tools/compare_kernel_asm.py a.s b.s

A function's text runs from `.type <sym>,@function` to its `.Lfunc_end`; a kernel's includes its `.amdhsa_kernel` block (registers, LDS,
scratch).  Comments are stripped and the numbers in labels that count functions or temporaries are rewritten, so that functions may
change places in the file.  Exits 0 when both files hold the same symbols with equal text."""
import re
import sys


def functions(path):
    out, name = {}, None
    for line in open(path):
        line = re.sub(r"\.L(func_begin|func_end|tmp)\d+", r".L\1", re.sub(r"\bL?BB\d+_", "BB_", line.split(";")[0])).rstrip()
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m: name = m.group(1); out[name] = []
        if name is not None: out[name].append(line)
        if line.startswith(".Lfunc_end:"): name = None
    return out


a, b = functions(sys.argv[1]), functions(sys.argv[2])
kernels = sum(any(l.lstrip().startswith(".amdhsa_kernel") for l in body) for body in a.values())
differing = sorted(k for k in set(a) & set(b) if a[k] != b[k])
print(f"{len(a)} and {len(b)} function symbols ({kernels} kernels in the first file), {len(set(a) & set(b))} in both, {len(set(a) & set(b)) - len(differing)} with identical text")
for k in sorted(set(a) ^ set(b)): print("only in one file:", k)
for k in differing: print("differs:", k)
sys.exit(1 if differing or set(a) != set(b) else 0)

#!/usr/bin/env python3
"""Compare two assemblies of one unit of csrc/ kernel by kernel -- what a refactor of the host side has to leave alone:

    scratch/isa_compare.py BEFORE.s AFTER.s

Each file is the unit compiled with `-S --cuda-device-only` and the flags `_native.UNITS` gives it (tests/test_kernel_isa.py::_asm does
the same).  Kernels are paired by their symbol.  Printed: the number of kernels on each side, the symbols only one side has, and for
the pairs whether the instruction streams (labels renumbered) and the resource lines (registers, scratch, occupancy, LDS, code
length) are the same.  Exit status 0 when nothing differs.  A one-off tool, not a test: a checkout has no parent to compare against."""
import re
import sys

RESOURCES = re.compile(r"NumSgprs|NumVgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte")


def kernels(path):
    """symbol -> (instructions, resource lines)"""
    lines = open(path).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m:
            j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            body = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip()) for l in lines[i + 1:j]]
            out[m.group(1)] = ([l for l in body if l.strip()], [l for l in lines[j:j + 80] if RESOURCES.search(l)])
            i = j
        i += 1
    return out


before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
only_before, only_after = sorted(set(before) - set(after)), sorted(set(after) - set(before))
differ = sorted(n for n in set(before) & set(after) if before[n] != after[n])
print("kernels:", len(before), len(after))
for what, names in (("only in BEFORE", only_before), ("only in AFTER", only_after), ("differ", differ)):
    print(f"{what}: {len(names)}", *[n[:110] for n in names[:5]])
sys.exit(1 if only_before or only_after or differ else 0)

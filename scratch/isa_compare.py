#!/usr/bin/env python3
"""Compare two assemblies of csrc/step_rollout.hip kernel by kernel (folding the plant kernels into their templates):

    scratch/isa_compare.py BEFORE.s AFTER.s

Each file is the unit compiled with `-S --cuda-device-only` and the flags `_native.UNITS[0]` gives it (tests/test_kernel_isa.py::_asm
does the same).  BEFORE has the twin templates `gpd_X_plant_kernel<a...>`, AFTER has `gpd_X_kernel<a..., defaults..., PLANT = true>`; the
two are paired, every other kernel is paired with its namesake (whose name gained a trailing `PLANT = false`).  Printed: the number of
kernels on each side, the unpaired ones, and for the pairs whether the instruction streams (labels renumbered) and the resource lines
(registers, scratch, occupancy, LDS, code length) are the same; the differences that an argument block 8 bytes longer explains --
`.amdhsa_kernarg_size`, the offset of a scalar load of a hidden argument behind the new pointer -- are counted apart from any OTHER.
A one-off tool, not a test: a checkout has no parent to compare against."""
import collections
import re
import sys

TEMPLATES = ("gpd_step_kernel", "gpd_rollout_kernel", "gpd_rollout1_kernel")
TWINS = tuple(t.replace("_kernel", "_plant_kernel") for t in TEMPLATES)
NAME = re.compile(r"_ZN12_GLOBAL__N_1\d+(gpd_\w+?_kernel)I((?:L[bi]n?\d+E)+)E")
RESOURCES = re.compile(r"NumSgprs|NumVgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte")
KERNARG_LOAD = re.compile(r"\ts_load_dword\w* s\S+, s\[\d+:\d+\], 0x[0-9a-f]+$")


def kernels(path):
    """symbol -> (body lines, resource lines)"""
    lines = open(path).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m:
            j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            out[m.group(1)] = (lines[i + 1:j], [l for l in lines[j:j + 80] if RESOURCES.search(l)])
            i = j
        i += 1
    return out


def normalised(name, body):
    res = []
    for l in body:
        s = l.split(";")[0].rstrip()
        if s.strip():
            res.append(re.sub(r"\.LBB\d+_", ".LBB_", s).replace(name, "K"))
    return res


def key(symbol, after):
    """what pairs a kernel of BEFORE with one of AFTER: (template or twin, the twin's six arguments / all arguments but PLANT)"""
    m = NAME.match(symbol)
    if not m or m.group(1) not in TEMPLATES + TWINS:
        return symbol
    base, args = m.group(1), re.findall(r"L[bi](n?\d+)E", m.group(2))
    if after:
        plant, args = args[-1], args[:-1]
        if plant == "1":
            base, args = base.replace("_kernel", "_plant_kernel"), args[:6]
    return (base, tuple(args))


before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
print("kernels:", len(before), len(after))
by_key = {key(n, True): n for n in after}
assert len(by_key) == len(after)
pairs, kinds = collections.Counter(), collections.Counter()
for nb, (body_b, res_b) in before.items():
    na = by_key.pop(key(nb, False), None)
    if na is None:
        pairs["missing in AFTER"] += 1
        print("missing", nb[:110])
        continue
    x, y = normalised(nb, body_b), normalised(na, after[na][0])
    if res_b != after[na][1]:
        pairs["resource lines differ"] += 1
    if len(x) != len(y):
        pairs["length differs"] += 1
        print("LEN", nb[:110])
        continue
    other = False
    for p, q in zip(x, y):
        if p != q:
            if "kernarg_size" in p:
                kinds["kernarg_size"] += 1
            elif KERNARG_LOAD.match(p) and re.sub(r"0x[0-9a-f]+$", "", p) == re.sub(r"0x[0-9a-f]+$", "", q):
                kinds["kernarg-offset load"] += 1
            else:
                kinds["OTHER"] += 1
                other = True
    pairs["other differences" if other else "same, or kernarg only"] += 1
print("unpaired in AFTER:", len(by_key), list(by_key)[:3])
print(dict(pairs), dict(kinds))

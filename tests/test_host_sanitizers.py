""""-fsanitize=address host build".  The HOST side of libgpd -- argument checks, error strings, struct plumbing,
launch arithmetic, the choice of the kernel -- compiled from the five product units (step_rollout.hip, policy.hip, swarm.hip, abi.hip,
mrac.hip) with AddressSanitizer + UndefinedBehaviorSanitizer (`hipcc --cuda-host-only`: no device code, seconds), linked against a HIP
runtime that launches nothing and names what it was asked to launch (tests/stubs/hip_stub.c), and driven through every entry of
include/gpd.h by a plain C program (tests/c/asan_host.c); tests/c/launch_trace.c then lists which kernel serves which call over the
shapes at which a launch path decides something, and tests/c/arg_errors.c what every entry refuses, one broken argument at a time, against
the recorded table tests/c/arg_errors.expected.  No GPU needed."""
import os
import re
import subprocess

import pytest

from conftest import REPO


def test_host_side_of_the_c_abi_under_asan_and_ubsan(tmp_path):
    from gym_pybullet_drones_amd import _native
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    clang = "/opt/rocm/lib/llvm/bin/clang"
    if not (os.path.exists(hipcc) and os.path.exists(clang)):
        pytest.skip("no hipcc / clang")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    objs, procs = [], []
    for unit, _ in _native.UNITS:
        obj = str(tmp_path / unit.replace(".hip", ".host.o"))
        cmd = [hipcc, "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-fPIC"] + san + ["-I", _native.INCLUDE, "-c", os.path.join(_native.CSRC, unit), "-o", obj]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        objs.append(obj)
    for p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, out[-3000:]
    # the device images the host objects expect to be linked against: empty stand-ins (nothing is ever launched)
    undefined = subprocess.run(["nm", "-u"] + objs, capture_output=True, text=True, check=True).stdout
    fatbins = sorted(set(re.findall(r"__hip_fatbin_\w+", undefined)))
    assert len(fatbins) == len(_native.UNITS), fatbins
    stub_c = str(tmp_path / "fatbin_stubs.c")
    open(stub_c, "w").write("".join(f"const char {s}[16] = {{0}};\n" for s in fatbins))
    lib = str(tmp_path / "libgpd_asan.so")
    link = [clang + "++", "-shared", "-fPIC"] + san + objs + ["-x", "c", stub_c, os.path.join(REPO, "tests", "stubs", "hip_stub.c"), "-o", lib, "-ldl"]
    res = subprocess.run(link, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    exes = {}
    for name in ("asan_host", "launch_trace", "arg_errors"):
        exes[name] = str(tmp_path / name)
        res = subprocess.run([clang] + san + ["-std=c11", "-I", _native.INCLUDE, os.path.join(REPO, "tests", "c", name + ".c"), lib, f"-Wl,-rpath,{tmp_path}", "-o", exes[name]],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("GPD_ROLLOUT_SIZED", None)
    run = subprocess.run([exes["asan_host"]], capture_output=True, text=True, env=env, timeout=120)
    print(run.stdout[-3000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and " 0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") >= 86

    # which kernel serves which call, with the sized variants and under the hook that leaves the generic kernels only
    traces = []
    for hook in ({}, {"GPD_ROLLOUT_SIZED": "0"}):
        run = subprocess.run([exes["launch_trace"]], capture_output=True, text=True, env=dict(env, **hook), timeout=120)
        assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
        assert run.returncode == 0, run.stderr[-2000:]
        lines = run.stdout.splitlines()
        assert len(lines) > 10000
        assert not [l for l in lines if l.endswith("-> nothing")][:5]                 # every accepted call launched
        assert not [l for l in lines if l.split(" -> ")[1].startswith("?")][:5]       # ... kernels the stub can name
        traces.append(lines)
    sized, generic = traces
    assert len(sized) == len(generic)
    rollout_kernels = ("gpd_step_kernel", "gpd_rollout_kernel", "gpd_rollout1_kernel")
    changed = [(a, b) for a, b in zip(sized, generic) if a != b]
    assert changed                                                                     # (the hook does something)
    assert not [(a, b) for a, b in changed if not (any(k in a for k in rollout_kernels) and any(k in b for k in rollout_kernels))][:5]

    # what every entry refuses: the recorded codes, and a message that names the entry, row by row
    run = subprocess.run([exes["arg_errors"]], capture_output=True, text=True, env=env, timeout=120)
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, run.stderr[-2000:]
    row = re.compile(r"(\w+) (.+) -> rc (-?\d+) \| (.*)")
    rows = [row.fullmatch(l).groups() for l in run.stdout.splitlines()]
    recorded = [row.fullmatch(l).groups() for l in open(os.path.join(REPO, "tests", "c", "arg_errors.expected")).read().splitlines()]
    assert len(recorded) > 700
    assert [r[:3] for r in rows] == [r[:3] for r in recorded], [(a, b) for a, b in zip(rows, recorded) if a[:3] != b[:3]][:5]
    assert not [r for r in rows if int(r[2]) == 0 or not r[3].startswith(r[0] + ": ") or len(r[3]) <= len(r[0]) + 2][:5]

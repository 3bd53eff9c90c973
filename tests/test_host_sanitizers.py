""""-fsanitize=address host build".  The HOST side of libgpd -- argument checks, error strings, struct plumbing,
launch arithmetic, the choice of the kernel -- compiled from the five product units (step_rollout.hip, policy.hip, swarm.hip, abi.hip,
mrac.hip) with AddressSanitizer + UndefinedBehaviorSanitizer (host-only: no device code, seconds), linked against a HIP runtime that
launches nothing and names what it was asked to launch (tests/stubs/hip_stub.c) -- the build is tests/helpers/host_lib.py's --, and
driven through every entry of include/gpd.h by a plain C program (tests/c/asan_host.c); tests/c/launch_trace.c then lists which kernel
serves which call over the shapes at which a launch path decides something, and tests/c/arg_errors.c what every entry refuses, one
broken argument at a time, against the recorded table tests/c/arg_errors.expected.  No GPU needed."""
import os
import re
import sys

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import host_lib  # noqa: E402


def test_host_side_of_the_c_abi_under_asan_and_ubsan():
    exes = {name: host_lib.program(name) for name in ("asan_host", "launch_trace", "arg_errors")}          # (the library: host_lib.library)
    env = host_lib.environment()
    env.pop("GPD_ROLLOUT_SIZED", None)
    run = host_lib.run(exes["asan_host"], env=env)
    print(run.stdout[-3000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and " 0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") >= 86

    # which kernel serves which call, with the sized variants and under the hook that leaves the generic kernels only
    traces = []
    for hook in ({}, {"GPD_ROLLOUT_SIZED": "0"}):
        run = host_lib.run(exes["launch_trace"], env=dict(env, **hook))
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
    run = host_lib.run(exes["arg_errors"], env=env)
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0, run.stderr[-2000:]
    row = re.compile(r"(\w+) (.+) -> rc (-?\d+) \| (.*)")
    rows = [row.fullmatch(l).groups() for l in run.stdout.splitlines()]
    recorded = [row.fullmatch(l).groups() for l in open(os.path.join(REPO, "tests", "c", "arg_errors.expected")).read().splitlines()]
    assert len(recorded) > 700
    assert [r[:3] for r in rows] == [r[:3] for r in recorded], [(a, b) for a, b in zip(rows, recorded) if a[:3] != b[:3]][:5]
    assert not [r for r in rows if int(r[2]) == 0 or not r[3].startswith(r[0] + ": ") or len(r[3]) <= len(r[0]) + 2][:5]


def test_lanes_per_wave_is_refused_or_sizes_the_single_step_grid():
    """`GpdStepCfg.lanes_per_wave` (tests/c/lanes_per_wave.c): 8, 48, -1 and four more values are refused with GPD_EINVAL and "<entry>:
    lanes_per_wave must be 0, 16, 32 or 64" by the five entries that read it, nothing launched; 0 launches what 64 launches; 16 and 32
    make the single-step grid (also of a one-step rollout) four and two times as large, and change neither a longer rollout's nor a
    multi-drone aviary's."""
    exe = host_lib.program("lanes_per_wave")
    run = host_lib.run(exe)
    print(run.stdout[-3000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") == 5 * 11 + 4 * 3 + 4
    for value in (8, 48, -1):
        assert f"ok   gpd_step refuses lanes_per_wave = {value}\n" in run.stdout

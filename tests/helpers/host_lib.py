"""The HOST side of libgpd under AddressSanitizer + UndefinedBehaviorSanitizer, built once per test session: the five product units
compiled with `hipcc --cuda-host-only` (no device code), empty stand-ins for the device images they expect, and tests/stubs/hip_stub.c
as the HIP runtime (launches are counted and named, nothing runs).  tests/test_host_sanitizers.py, tests/test_host_diff.py and
tests/test_host_sysid.py compile their stand-alone C programs (tests/c/) against it and run them here; the last two also share what
their ctypes calls into the product library start from (`params`, `step_cfg`, `REJECTED`).  No GPU needed.  Test infrastructure."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@functools.lru_cache(maxsize=None)
def library() -> str:
    """path of libgpd_asan.so, in a directory of its own that goes when the process does; skips the test without hipcc / clang"""
    from gym_pybullet_drones_amd import _native
    if not (os.path.exists(HIPCC) and os.path.exists(CLANG)):
        pytest.skip("no hipcc / clang")
    tmp = tempfile.mkdtemp(prefix="gpd_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    objs, procs = [], []
    for unit, _ in _native.UNITS:          # the units compile side by side
        obj = os.path.join(tmp, unit.replace(".hip", ".host.o"))
        cmd = [HIPCC, "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-fPIC"] + SAN + ["-I", _native.INCLUDE, "-c", os.path.join(_native.CSRC, unit), "-o", obj]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        objs.append(obj)
    for p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, out[-3000:]
    # the device images the host objects expect to be linked against: empty stand-ins (nothing is ever launched)
    undefined = subprocess.run(["nm", "-u"] + objs, capture_output=True, text=True, check=True).stdout
    fatbins = sorted(set(re.findall(r"__hip_fatbin_\w+", undefined)))
    assert len(fatbins) == len(_native.UNITS), fatbins
    stub_c = os.path.join(tmp, "fatbin_stubs.c")
    with open(stub_c, "w") as f:
        f.write("".join(f"const char {s}[16] = {{0}};\n" for s in fatbins))
    lib = os.path.join(tmp, "libgpd_asan.so")
    link = [CLANG + "++", "-shared", "-fPIC"] + SAN + objs + ["-x", "c", stub_c, os.path.join(REPO, "tests", "stubs", "hip_stub.c"), "-o", lib, "-ldl"]
    res = subprocess.run(link, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return lib


def program(name: str, include=()) -> str:
    """tests/c/<name>.c compiled with the sanitisers against the library (include/ and `include` on its -I path): the executable"""
    from gym_pybullet_drones_amd import _native
    lib = library()
    exe = os.path.join(os.path.dirname(lib), name)
    dirs = [x for d in (_native.INCLUDE, *include) for x in ("-I", d)]
    res = subprocess.run([CLANG] + SAN + ["-std=c11"] + dirs + [os.path.join(REPO, "tests", "c", name + ".c"), lib, f"-Wl,-rpath,{os.path.dirname(lib)}", "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    return exe


def environment() -> dict:
    """this process's environment with the sanitisers' options of the host tests: leaks and undefined behaviour are fatal"""
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def run(exe: str, *args, env: dict = None):
    """the finished process of `exe args` under `env` (`environment()` by default)"""
    return subprocess.run([exe, *args], capture_output=True, text=True, env=environment() if env is None else env, timeout=120)


@functools.lru_cache(maxsize=None)
def diff_host():
    """tests/c/diff_host.c -- the host side of the five entries of the differentiable rollout -- built and run once:
    (the finished process, the file of formula values it wrote)"""
    from gym_pybullet_drones_amd import _native
    exe = program("diff_host", include=(_native.CSRC,))
    values = os.path.join(os.path.dirname(exe), "formulas.txt")
    return run(exe, values), values


# ---- the entries of the differentiable rollout through ctypes: a supported configuration, and every change that is refused ---------
def params(model):
    from gym_pybullet_drones_amd.params import DroneParams
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    from diff_f64 import MODELS
    return DroneParams(getattr(DroneModel, MODELS[model]))


def step_cfg(**kw):
    from gym_pybullet_drones_amd import _native
    d = dict(num_envs=70, drones_per_env=1, act_type=0, substeps=8, physics_flags=0, pyb_dt=1 / 240, ctrl_dt=1 / 30, inv_ctrl_dt=30.0,
             lanes_per_wave=64, task=1, xy_bound=1.5, z_bound=2.0, tilt_bound=0.4, term_dist=1e-4, trunc_counter=1920, target_per_env=0,
             init_per_env=0, auto_reset=0)
    d.update(kw)
    return _native.GpdStepCfg(**d)


REJECTED = [(dict(act_type=1), "DSLPID"), (dict(act_type=2), "DSLPID"), (dict(act_type=4), "DSLPID"),
            (dict(physics_flags=1), "physics_flags"), (dict(physics_flags=4), "physics_flags"), (dict(physics_flags=8), "physics_flags"),
            (dict(physics_flags=16), "physics_flags"), (dict(physics_flags=3), "physics_flags"),
            (dict(drones_per_env=2, num_envs=35), "drones_per_env"), (dict(task=2), "task"), (dict(auto_reset=1), "auto_reset")]

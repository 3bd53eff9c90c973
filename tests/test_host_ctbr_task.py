"""CTBR as a task (`gpd_task_eval`, `gpd_rollout_ctbr_task`, `envs.VectorCTBRAviary`), the part that needs no GPU: the binding and the
header, the one sub-step helper both CTBR kernels call, what the class constructs and refuses, the inputs of the device test against
their float64 prediction (tests/helpers/ctbr_task_cases.py), every refusal of the two launching entries against the launch stub under
ASan + UBSan (tests/c/ctbr_task_host.c), and the new kernels' resource remarks.  The sanitizers run in the stand-alone program only,
never in this process."""
import ctypes
import functools
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import ctbr_task_cases as T  # noqa: E402


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_three_entries_and_the_abi_stays():
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    P = ctypes.POINTER
    for name in ("gpd_task_eval", "gpd_sizeof_ctbr_task", "gpd_rollout_ctbr_task"):
        res, args = _native._SIGNATURES[name]
        assert name in _native.exported_symbols() and getattr(L, name).argtypes == args and res is ctypes.c_int
    _, ev = _native._SIGNATURES["gpd_task_eval"]
    assert len(ev) == 8 and ev[0] == P(_native.GpdStepCfg) and all(a is ctypes.c_void_p for a in ev[1:])
    _, ro = _native._SIGNATURES["gpd_rollout_ctbr_task"]
    assert len(ro) == 20 and ro[:5] == [P(t) for t in (_native.GpdParams, _native.GpdCtbr, _native.GpdState, _native.GpdStepCfg, _native.GpdCtbrTask)]
    assert ro[5] is ctypes.c_int32 and [i for i, a in enumerate(ro) if a is ctypes.c_int64] == [7, 13, 17] and ro[19] is ctypes.c_void_p
    size = ctypes.c_int32(0)
    assert L.gpd_sizeof_ctbr_task(ctypes.byref(size)) == 0 and size.value == ctypes.sizeof(_native.GpdCtbrTask) == 48
    assert L.gpd_sizeof_ctbr_task(None) == _native.GPD_EINVAL and L.gpd_last_error().decode().startswith("gpd_sizeof_ctbr_task: ")
    assert [(n, ctypes.sizeof(t)) for n, t in _native.GpdCtbrTask._fields_] == [("act_scale", 16), ("act_bias", 16), ("normalized", 4), ("pad_", 12)]
    assert L.gpd_abi_version() == 9 and _native.ABI_VERSION == 9 and len(_native.UNITS) == 5
    assert "ctbr_task.inc" in _native.HEADERS and os.path.exists(os.path.join(_native.CSRC, "ctbr_task.inc"))
    abi = open(os.path.join(_native.CSRC, "abi.hip")).read()
    assert abi.index('#include "ctbr.inc"') < abi.index('#include "ctbr_task.inc"') < abi.index('#include "mppi_ctbr.inc"')


def test_header_and_mirror_agree():
    from gym_pybullet_drones_amd import _native
    hdr = open(os.path.join(_native.INCLUDE, "gpd.h")).read()
    assert "#define GPD_ABI_VERSION 9" in hdr
    body = re.search(r"typedef struct GpdCtbrTask \{(.*?)\} GpdCtbrTask;", hdr, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+)(?:\[(\d+)\])?;", body, flags=re.M)
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32}
    want = [(name, ctype[t] * int(n) if n else ctype[t]) for t, name, n in fields]
    assert [(n, ctypes.sizeof(t)) for n, t in want] == [(n, ctypes.sizeof(t)) for n, t in _native.GpdCtbrTask._fields_] and len(want) == 4
    assert re.search(r"^int gpd_task_eval\(const GpdStepCfg\* cfg, const float\* obs12, const int32_t\* counter, const float\* target_pos, float\* reward,", hdr, flags=re.M)
    assert re.search(r"^int gpd_sizeof_ctbr_task\(int32_t\* size_out\);", hdr, flags=re.M)
    decl = re.search(r"^int gpd_rollout_ctbr_task\((.*?)\);", hdr, flags=re.M | re.S).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    assert len(params) == len(_native._SIGNATURES["gpd_rollout_ctbr_task"][1]) == 20
    for p, a in zip(params, _native._SIGNATURES["gpd_rollout_ctbr_task"][1]):
        assert ("int64_t" in p) == (a is ctypes.c_int64) and ("int32_t num_steps" in p) == (a is ctypes.c_int32), p
    assert params[4] == "const GpdCtbrTask* task" and params[-1] == "void* stream"


def test_both_kernels_fly_their_sub_steps_through_one_helper():
    """the rate loop inside the sub-steps is stated once (ctbr.inc: ctbr_substep / ctbr_substeps) and called by both kernels; the task
    is gpd_common.inc's task_single, called, not restated"""
    from gym_pybullet_drones_amd import _native
    plain = open(os.path.join(_native.CSRC, "ctbr.inc")).read()
    fused = open(os.path.join(_native.CSRC, "ctbr_task.inc")).read()
    assert plain.count("void ctbr_substep(") == 1 and plain.count("void ctbr_substeps(") == 1 and plain.count("gpd_ctbr_rate_loop(") == 1
    assert plain.count("ctbr_substeps<EXT>(P, B, Q, C, flags, drag, cmd, c, avx, avy, avz);") == 1
    assert fused.count("ctbr_substeps<EXT>(P, B, Q, C, flags, drag, cmd, c, avx, avy, avz);") == 1
    assert "gpd_ctbr_rate_loop" not in fused and "substep<" not in fused.replace("ctbr_substeps<", "")
    assert fused.count("task_single(C, ") == 2 and "fast_sqrt" not in fused and "tilt_bound" not in fused


# ---- the class ----------------------------------------------------------------------------------------------------------------------------
def test_class_refuses_what_the_entry_does_not_serve_and_defaults_are_hover_centred():
    from gym_pybullet_drones_amd.control.CTBRControl import G_Z, RATE_MAX
    from gym_pybullet_drones_amd.envs import VectorAviary, VectorCTBRAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    assert issubclass(VectorCTBRAviary, VectorAviary)
    # everything below is refused before any device work: no GPU is touched
    for kw in (dict(num_drones=2), dict(full_obs=True), dict(full_obs="lazy"), dict(task="multihover"), dict(physics=Physics.PYB_DW), dict(physics=4)):
        with pytest.raises(NotImplementedError):
            VectorCTBRAviary(4, **kw)
    for kw in (dict(k_rate=(40.0, 0.0, 20.0)), dict(rate_max=float("nan")), dict(thrust_max=-1.0), dict(thrust_span=float("inf")), dict(randomize={"weight": 0.1})):
        with pytest.raises(ValueError):
            VectorCTBRAviary(4, **kw)
    sig = inspect.signature(VectorCTBRAviary.__init__).parameters
    assert sig["normalized"].default is True and sig["ctrl_freq"].default == 48 and sig["task"].default == "hover"
    assert all(sig[n].default is None for n in ("thrust_center", "thrust_span", "rate_span", "k_rate"))
    assert all(n in sig for n in ("num_envs", "randomize", "keep_terminal_obs", "nan_guard", "target_pos", "episode_len_sec"))
    t = VectorCTBRAviary.task_struct(G_Z, RATE_MAX)
    g, r = np.float32(G_Z), np.float32(RATE_MAX)
    assert t.normalized == 1 and list(t.act_scale) == [g, r, r, r] and list(t.act_bias) == [g, 0.0, 0.0, 0.0]

    def cmd(task, a):            # the kernel's map: one fused multiply-add per component, in float32
        return [np.float32(np.float64(x) * np.float64(s) + np.float64(b)) for x, s, b in zip(a, task.act_scale, task.act_bias)]
    assert cmd(t, [0.0, 0.0, 0.0, 0.0]) == [g, 0.0, 0.0, 0.0]                       # a = 0: the hover command
    assert cmd(t, [-1.0, 0.0, 0.0, 0.0])[0] == 0.0                                    # a = -1: zero thrust
    assert cmd(t, [1.0, 1.0, -1.0, 1.0]) == [2 * g, r, -r, r]
    u = VectorCTBRAviary.task_struct(G_Z, RATE_MAX, thrust_center=12.0, thrust_span=4.0, rate_span=3.0, normalized=False)
    assert u.normalized == 0 and list(u.act_scale) == [4.0, 3.0, 3.0, 3.0] and list(u.act_bias) == [12.0, 0.0, 0.0, 0.0]


# ---- the inputs of the device test --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("N", [70, 257])
def test_inputs_end_episodes_by_every_cause_in_float64(N, S):
    """the float64 yardstick flown through the composition's steps: at least 20 % of the drones end before the last of six steps,
    through the clock, the box and the tilt, and some terminate -- with and without the flags and the +-25 % masses the device cases
    use.  Every group ends at step 2, where it was placed; the `none` group never does."""
    for flags, mass in ((0, None), (T.EVERY, np.where(np.arange(N) % 2 == 0, 1.25, 0.75))):
        s = T.scene(N, 6, S, target_per_env=1, init_per_env=1)
        first, why = T.predict(s, flags, mass)
        share, kinds, near = T.condition(first, why, 6)
        assert share >= 0.2 and kinds == 3 and near >= 1, (share, kinds, near)
        for g, name in enumerate(T.GROUPS):
            assert set(first[s.group == g]) == ({6} if name == "none" else {2}), name
        assert why[0][s.group == 3].all() and why[1][s.group == 1].all() and why[2][(s.group == 0) | (s.group == 5)].all() and why[3][s.group == 2].all()
    assert s.kin.shape == (13, N) and s.kin.dtype == np.float32 and s.cmd.shape == (6, N, 4) and s.counter.dtype == np.int32
    assert (s.cmd[..., 0] > 40.9).any() and (s.cmd[..., 0] < 0).any() and (np.abs(s.cmd[..., 1:]) > 2 * np.pi).any()       # beyond both clips


def test_ten_steps_end_episodes_in_both_parts_of_a_split_launch():
    s = T.scene(70, 10, 5, target_per_env=1, init_per_env=1)
    T.predict(s, T.EVERY)
    assert T.predict.ends[:4].any() and T.predict.ends[4:].any()


# ---- the two launching entries against the launch stub, under ASan + UBSan -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program():
    import host_lib
    return host_lib.program("ctbr_task_host")


def test_host_side_of_the_entries_under_asan_and_ubsan():
    """tests/c/ctbr_task_host.c linked to the host-only build of the units and the launch stub under -fsanitize=address,undefined: a
    good call launches the instantiation <EXT, PLANT> that the arguments select, one drone per lane; every refusal has its code, the
    entry's name and the reason, and launches nothing"""
    import host_lib
    run = host_lib.run(host_program())
    print(run.stdout[-8000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") == 84 and "FAIL" not in run.stdout
    for piece in ("ILb1ELb1EE", "ILb1ELb0EE", "ILb0ELb1EE", "ILb0ELb0EE"):
        assert f"\n{piece}\n" in run.stdout, piece


# ---- the kernels' resources -----------------------------------------------------------------------------------------------------------------
def test_every_new_instantiation_runs_without_scratch():
    """The unit that ships -- csrc/abi.hip with its own flags, device side only -- under -Rpass-analysis=kernel-resource-usage: the four
    instantiations of ctbr_task_kernel and gpd_task_eval_kernel use zero bytes of scratch and spill no VGPR (DESIGN.md section 3.23
    states the figures); gpd_rollout_ctbr_kernel, whose sub-steps now go through the shared helper, keeps zero scratch too."""
    from gym_pybullet_drones_amd import _native
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    flags = dict(_native.UNITS)["abi.hip"]
    cmd = [hipcc] + _native.COMMON_FLAGS + flags + ["-I", _native.INCLUDE, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                   "-c", os.path.join(_native.CSRC, "abi.hip"), "-o", os.devnull]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    blocks = re.split(r"remark: Function Name: ", res.stderr)[1:]
    for kernel, count, min_occ in (("ctbr_task_kernel", 4, 4), ("gpd_task_eval_kernel", 1, 8), ("gpd_rollout_ctbr_kernel", 8, 4)):
        mine = [b for b in blocks if kernel in b.split("\n", 1)[0]]
        assert len(mine) == count, (kernel, [b.split("\n", 1)[0] for b in blocks])
        for b in mine:
            name = b.split(" ", 1)[0]
            scratch, spill = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b), re.search(r"VGPRs Spill: (\d+)", b)
            vgprs, sgprs, occ = re.search(r" VGPRs: (\d+)", b), re.search(r"TotalSGPRs: (\d+)", b), re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b)
            print(name, "VGPRs", vgprs.group(1), "SGPRs", sgprs.group(1), "occupancy", occ.group(1), "scratch", scratch.group(1))
            assert scratch.group(1) == "0" and spill.group(1) == "0" and "Dynamic Stack: False" in b, b[:1500]
            assert int(occ.group(1)) >= min_occ and int(vgprs.group(1)) <= 128, b[:1500]


# ---- the recorded cost --------------------------------------------------------------------------------------------------------------------
def test_recorded_profile_shows_the_fused_launch_faster_at_every_shape():
    """profiles/ctbr_task_mi355x.json, as profiles/ctbr_task_bench.py wrote it on an MI355X: the four shapes, fused and composed bit for bit
    before the timing, and the one condition fixed in advance -- the eager fused launch faster than the composition in one hipGraph"""
    import json
    res = json.load(open(os.path.join(REPO, "profiles", "ctbr_task_mi355x.json")))
    assert sorted(res["shapes"]) == ["N4096_K1", "N4096_K20", "N65536_K1", "N65536_K20"] and res["condition_met"] is True
    for v in res["shapes"].values():
        us = v["us_per_env_step"]
        assert v["bit_for_bit"] is True and 0 < us["fused"] < us["composed_graph"] and set(us) >= {"fused_graph", "ctbr_no_task", "pid_task"}

"""The obstacle task (`gpd_rollout_obst`, `envs.VectorObstacleAviary`), the part that needs no GPU: the binding and the header, what the
class constructs and refuses, the table of device cases against the paths of the kernel, csrc/obst_task_math.inc compiled for the host
against its float64 restatement (tests/helpers/obst_task_f64.py), every refusal of the entry against the launch stub under ASan + UBSan
(tests/c/obst_task_host.c), and the kernel's resource remarks.  The sanitizers run in the stand-alone program only, never in this
process."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import obst_task_f64 as yo  # noqa: E402


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry_and_pins_nothing_else():
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    res, args = _native._SIGNATURES["gpd_rollout_obst"]
    assert "gpd_rollout_obst" in _native.exported_symbols() and "gpd_sizeof_obst_task" in _native.exported_symbols()
    assert L.gpd_rollout_obst.argtypes == args and len(args) == 22 and res is ctypes.c_int
    assert args[:4] == [ctypes.POINTER(t) for t in (_native.GpdParams, _native.GpdState, _native.GpdStepCfg, _native.GpdObstTask)]
    assert args[4] is ctypes.c_int32 and args[6] is ctypes.c_int64 and args[10] is ctypes.c_int32 and args[11] is ctypes.c_int64
    assert args[14] is ctypes.c_int64 and args[15] is ctypes.c_int64 and args[20] is ctypes.c_int64 and args[21] is ctypes.c_void_p
    size = ctypes.c_int32(0)
    assert L.gpd_sizeof_obst_task(ctypes.byref(size)) == 0 and size.value == ctypes.sizeof(_native.GpdObstTask) == 32
    assert [n for n, _ in _native.GpdObstTask._fields_] == ["collision_radius", "hit_terminates", "hit_reward", "prox_margin", "prox_weight",
                                                           "n_rays", "ray_frame", "max_range"]
    assert L.gpd_abi_version() == 9 and _native.ABI_VERSION == 9 and len(_native.UNITS) == 5
    for inc in ("obst_task.inc", "obst_task_math.inc"):
        assert inc in _native.HEADERS and os.path.exists(os.path.join(_native.CSRC, inc))
    abi = open(os.path.join(_native.CSRC, "abi.hip")).read()
    assert abi.index('#include "obstacles.inc"') < abi.index('#include "obst_task.inc"') < abi.index('#include "mppi.inc"')
    hdr = open(os.path.join(_native.INCLUDE, "gpd.h")).read()
    assert re.search(r"^int gpd_rollout_obst\(const GpdParams\* params, const GpdState\* state, const GpdStepCfg\* cfg, const GpdObstTask\* task, int32_t num_steps,",
                     hdr, flags=re.M)
    assert re.search(r"^int gpd_sizeof_obst_task\(int32_t\* size_out\);", hdr, flags=re.M) and "typedef struct GpdObstTask {" in hdr
    assert "#define GPD_ABI_VERSION 9" in hdr


def test_both_kernels_turn_their_rays_with_one_helper():
    from gym_pybullet_drones_amd import _native
    scan = open(os.path.join(_native.CSRC, "obstacles.inc")).read()
    fused = open(os.path.join(_native.CSRC, "obst_task.inc")).read()
    assert scan.count("void obst_turn_ray(") == 1 and scan.count("obst_turn_ray(frame, q.x") == 1 and "obst_turn_ray(Q.ray_frame" in fused
    assert "sinf(yaw)" not in fused and scan.count("sinf(yaw)") == 1


# ---- the class ----------------------------------------------------------------------------------------------------------------------------
def test_class_constructs_its_task_and_refuses_what_the_entry_does_not_serve():
    from gym_pybullet_drones_amd import obstacles as ob
    from gym_pybullet_drones_amd.envs import VectorAviary, VectorObstacleAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType, Physics
    assert issubclass(VectorObstacleAviary, VectorAviary)
    t = VectorObstacleAviary.task_struct(0.06, True, -5.0, 0.5, 2.0, 16, "body", 1.5)
    assert (t.hit_terminates, t.n_rays, t.ray_frame) == (1, 16, 2) and t.collision_radius == np.float32(0.06) and t.max_range == 1.5
    assert VectorObstacleAviary.task_struct(0.06, False, 0.0, 0.0, 0.0, 0, "world", 5.0).hit_terminates == 0
    for bad in (dict(collision_radius=0.0), dict(collision_radius=float("nan")), dict(hit_reward=float("inf")), dict(prox_margin=-0.1),
                dict(prox_weight=-1.0), dict(max_range=0.0), dict(frame="sideways")):
        kw = dict(collision_radius=0.06, hit_terminates=True, hit_reward=-1.0, prox_margin=0.1, prox_weight=1.0, n_rays=4, frame="body", max_range=2.0)
        with pytest.raises(ValueError):
            VectorObstacleAviary.task_struct(**{**kw, **bad})
    assert VectorObstacleAviary.check_rays(None) is None
    rays = VectorObstacleAviary.check_rays(ob.fan(16, 1.0))
    assert rays.shape == (16, 3) and rays.dtype == np.float32 and rays.flags["C_CONTIGUOUS"]
    for bad in (np.zeros((65, 3)), np.zeros((0, 3)), np.zeros((4, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            VectorObstacleAviary.check_rays(bad)
    field = ob.ObstacleField().sphere((0, 0, 1), 0.1)
    # everything below is refused before any device work: no GPU is touched
    for kw in (dict(randomize={"mass": 0.1}), dict(full_obs=True), dict(full_obs="lazy"), dict(keep_terminal_obs=True), dict(nan_guard=True),
               dict(num_drones=2), dict(act=ActionType.ONE_D_RPM), dict(act="raw_rpm"), dict(task="multihover"), dict(physics=Physics.PYB_DW),
               dict(physics=4)):
        with pytest.raises(NotImplementedError):
            VectorObstacleAviary(4, field, **kw)
    with pytest.raises(ValueError, match="aviaries"):
        VectorObstacleAviary(4, ob.ObstacleField(3).sphere((0, 0, 1), 0.1))
    import inspect
    sig = inspect.signature(VectorObstacleAviary.__init__).parameters
    assert sig["hit_terminates"].default is True and sig["collision_radius"].default is None and sig["act"].default == ActionType.VEL
    assert all(n in sig for n in ("num_envs", "field", "rays", "max_range", "frame", "hit_reward", "prox_margin", "prox_weight", "task", "target_pos"))


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
def test_cases_cover_the_paths_of_the_kernel():
    """one drone, a partial wave, two workgroups at G = 1; one step and five; one sub-step and five; the three action types; no flag and
    every flag; n_rays 0, 1, 5, 16, 64, so G = 1, 1, 8, 16, 64; the three frames; shared lists of 1, 7 and 65 records with NONE records
    between, and per-aviary planes with a pitch above E and NaN beyond E; both tasks, with and without auto-reset"""
    C = yo.CASES
    for field, values in (("N", {1, 70, 257}), ("K", {1, 5}), ("S", {1, 5}), ("act", {"rpm", "vel", "pid"}), ("flags", {0, yo.EVERY}),
                          ("rays", {0, 1, 5, 16, 64}), ("frame", {"world", "level", "body"}), ("task", {"hover", "none"}), ("auto_reset", {0, 1}),
                          ("obst", {("shared", 1), ("shared", 7), ("shared", 65), ("lists", 5)})):
        assert {getattr(c, field) for c in C} == values, field
    assert {yo.group_lanes(c.rays) for c in C} == {1, 8, 16, 64} and [yo.group_lanes(r) for r in (0, 1, 5, 16, 17, 64)] == [1, 1, 8, 16, 32, 64]
    assert len({c.name for c in C}) == len(C) and 8 <= len(C) <= 10
    for act in ("rpm", "vel", "pid"):
        assert {c.flags for c in C if c.act == act} == {0, yo.EVERY}, act
        assert {c.obst[0] for c in C if c.act == act} == {"shared", "lists"}, act
    assert any(c.N == 257 and yo.group_lanes(c.rays) == 16 for c in C)        # many workgroups at G = 16
    assert any(c.N == 257 and yo.group_lanes(c.rays) == 1 for c in C)         # two workgroups at G = 1, the second one ragged
    for c in C:
        s = yo.scene(c)
        mode, M = c.obst
        assert s.kin.shape == (13, c.N) and s.kin.dtype == np.float32 and s.pid.shape == (9, c.N) and s.actions.shape == (c.K, c.N, yo.ACT_DIM[c.act])
        assert np.abs(s.pid).min() > 0 and np.abs(s.kin[10:13]).min() > 0                     # controller members and rates that are not zero
        kinds = s.records[..., 3]
        assert (kinds == yo.NONE).any() == (M > 1) and (kinds[:, 0] != yo.NONE).all()
        if mode == "lists":
            assert s.obst_ld > c.N and s.table.shape == (M * 8, s.obst_ld) and np.isnan(s.table[:, c.N:]).all() and not np.isnan(s.table[:, :c.N]).any()
        else:
            assert s.obst_ld == 1 and s.table.shape == (M, 8)
        if c.rays:
            np.testing.assert_allclose(np.linalg.norm(s.rays.astype(np.float64), axis=1), 1.0, atol=2e-7)
        # a third of the drones on a collision course: the gap is 10-60 % of what the start speed covers in K - 1 steps
        assert s.hitter[0] and (c.N == 1 or 0.25 <= s.hitter.mean() <= 0.45)
        ratio = s.gap[s.hitter] / s.travel[s.hitter]
        assert (ratio >= 0.1).all() and (ratio <= 0.6).all() and (s.gap[~s.hitter] > s.travel[~s.hitter] + 0.04).all()
        assert (s.gap[~s.hitter] < yo.PROX_MARGIN).all()                                        # ... the others inside the margin
        far = yo.scene(c, far=True)
        assert np.array_equal(far.kin, s.kin) and np.array_equal(far.actions, s.actions)


# ---- csrc/obst_task_math.inc on the host against the float64 restatement; the entry's refusals -------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program():
    import host_lib
    from gym_pybullet_drones_amd import _native
    return host_lib.program("obst_task_host", include=(_native.CSRC,))


def test_host_compiled_formula_agrees_with_the_float64_restatement(tmp_path):
    """The text the kernel compiles, built as a stand-alone program under ASan + UBSan: reward, hinge and hit of 4096 rows -- inside and
    outside the margin, in contact, exactly at contact, d = +inf -- within 4 ulp (fp32) of |task_reward| + |hit_reward| + prox_weight
    (prox_margin + |d - r|) of the float64 formula; the hit flags are the float64 ones exactly."""
    import host_lib
    x = yo.math_inputs()
    src, dst = str(tmp_path / "rows.bin"), str(tmp_path / "values.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(x)], dtype=np.int32).tobytes())
        f.write(x.tobytes())
    res = host_lib.run(host_program(), "math", src, dst)
    assert res.returncode == 0 and "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stdout[-2000:] + res.stderr[-4000:]
    raw = np.frombuffer(open(dst, "rb").read(), dtype=np.float32).reshape(len(x), 3)
    got_r, got_h, got_hit = raw[:, 0].astype(np.float64), raw[:, 1].astype(np.float64), raw[:, 2].view(np.int32)
    a = x.astype(np.float64)
    want = yo.reward(a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5])
    lim = yo.bound(a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5])
    err = np.abs(got_r - want)
    print(f"MEASURED host obstacle-task formula: worst error / bound {float((err / lim).max()):.3f}; hits {int(got_hit.sum())} of {len(x)}")
    assert np.isfinite(got_r).all() and (err <= lim).all()
    assert np.array_equal(got_hit != 0, yo.hit(a[:, 1], a[:, 2])) and 0.1 < got_hit.mean() < 0.5
    assert (got_h[np.isinf(a[:, 1])] == 0).all() and (got_h >= 0).all() and (got_h > 0).mean() > 0.3


def test_host_side_of_the_entry_under_asan_and_ubsan():
    """tests/c/obst_task_host.c linked to the host-only build of the units and the launch stub under -fsanitize=address,undefined: a good
    call launches the instantiation action type x flags x list that the arguments select, with 256 / G drones per workgroup and a shared
    list's bytes of LDS; every refusal has its code, the entry's name and the reason, and launches nothing"""
    import host_lib
    run = host_lib.run(host_program())
    print(run.stdout[-8000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") >= 85 and "FAIL" not in run.stdout
    for piece in ("ILi2ELb1ELb1EE", "ILi2ELb0ELb0EE", "ILi0ELb1ELb1EE", "ILi0ELb0ELb0EE", "ILi1ELb1ELb1EE", "ILi1ELb1ELb0EE"):
        assert f"\n{piece}\n" in run.stdout, piece


# ---- the kernel's resources -----------------------------------------------------------------------------------------------------------------
def test_every_instantiation_of_the_kernel_runs_without_scratch():
    """The unit that ships -- csrc/abi.hip with its own flags, device side only -- under -Rpass-analysis=kernel-resource-usage: the
    twelve instantiations of obst_task_kernel (three action types x flags x list) use zero bytes of scratch, spill no VGPR and keep at
    least three waves per SIMD (DESIGN.md section 3.22 states the figures).  The kernel compiled on its own, outside the unit, comes out
    with other register counts: only the unit's own code generation is what libgpd.so holds."""
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
    mine = [b for b in blocks if "obst_task_kernel" in b.split("\n", 1)[0]]
    assert len(mine) == 12, [b.split("\n", 1)[0] for b in blocks]
    for b in mine:
        name = b.split(" ", 1)[0]
        scratch, spill = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b), re.search(r"VGPRs Spill: (\d+)", b)
        vgprs, occ = re.search(r" VGPRs: (\d+)", b), re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b)
        print(name, "VGPRs", vgprs.group(1), "occupancy", occ.group(1), "scratch", scratch.group(1))
        assert scratch.group(1) == "0" and spill.group(1) == "0" and "Dynamic Stack: False" in b, b[:1500]
        assert int(occ.group(1)) >= 3 and int(vgprs.group(1)) <= 160, b[:1500]

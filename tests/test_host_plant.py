"""The per-drone plant (domain randomisation, include/gpd.h GPD_SCALE_* / GPD_PLANT_*) on the host side: the ABI mirror, the argument
checks of its two entries (nothing is launched) and the compiled plant kernels.  No GPU needed."""
import ctypes
import math
import os
import re

import pytest

from conftest import REPO


def _enum(hdr, prefix):
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(" + prefix + r"\w*)\s*=\s*(\d+)", hdr)}


def test_header_scale_enum_and_row_layout_match_the_python_mirror():
    from gym_pybullet_drones_amd import _native
    hdr = open(os.path.join(REPO, "include", "gpd.h")).read()
    scales = _enum(hdr, "GPD_SCALE_")
    assert _enum(hdr, "GPD_NUM_SCALES")["GPD_NUM_SCALES"] == len(_native.SCALE_FIELDS) == 9
    assert [f"GPD_SCALE_{f.upper()}" for f in _native.SCALE_FIELDS] == sorted(scales, key=scales.get)
    assert sorted(scales.values()) == list(range(9))
    rows = _enum(hdr, "GPD_PLANT_")
    assert rows.pop("GPD_PLANT_ROWS") == _native.PLANT_ROWS == len(_native.PLANT_ROW_FIELDS) == 19
    # every enumerator names where its field starts; the three-float fields take three rows
    starts = {"M": "GPD_PLANT_M", "inv_M": "GPD_PLANT_INV_M", "KF": "GPD_PLANT_KF", "GRAVITY": "GPD_PLANT_GRAVITY", "J[0]": "GPD_PLANT_J",
              "J_INV[0]": "GPD_PLANT_J_INV", "km_over_kf": "GPD_PLANT_KM_OVER_KF", "gnd_eff_coeff": "GPD_PLANT_GND_EFF",
              "drag_coeff[0]": "GPD_PLANT_DRAG", "hover_thrust": "GPD_PLANT_HOVER_THRUST", "hover_resid": "GPD_PLANT_HOVER_RESID",
              "norm_thrust": "GPD_PLANT_NORM_THRUST", "norm_gap": "GPD_PLANT_NORM_GAP"}
    assert set(starts.values()) == set(rows)
    for field, name in starts.items():
        assert _native.PLANT_ROW_FIELDS[rows[name]] == field, name
    # ... and every row that replaces a GpdParams field names one that exists
    from gym_pybullet_drones_amd.params import GpdParams
    members = {f for f, _ in GpdParams._fields_}
    assert {f.split("[")[0] for f in _native.PLANT_ROW_FIELDS[:17]} <= members


@pytest.fixture(scope="module")
def lib():
    from gym_pybullet_drones_amd import _native
    return _native.lib()


def _host_state(n, ld):
    """A GpdState over host buffers (never dereferenced: every call below fails its checks first)"""
    from gym_pybullet_drones_amd import _native
    buf = (ctypes.c_float * (64 * (ld + 64)))()
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 255) // 256 * 256
    st = _native.GpdState(kin=base, last_rpm=base, pid=base, step_counter=base, ld=ld)
    return buf, base, st


def _nominal():
    from gym_pybullet_drones_amd.params import DroneParams
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    return DroneParams(DroneModel.CF2X).to_struct(pid_model=DroneModel.CF2X)


def test_plant_derive_rejects_bad_arguments_before_device_work(lib):
    from gym_pybullet_drones_amd import _native
    P = _nominal()
    buf, base, _ = _host_state(128, 128)

    def derive(scales=base, rows=base, E=2, D=64, ld=128):
        rc = lib.gpd_plant_derive(ctypes.byref(P), scales, None, E, D, ld, rows, None)
        return rc, lib.gpd_last_error().decode()

    for kw in ({"rows": None}, {"scales": None}):
        rc, msg = derive(**kw)
        assert rc == _native.GPD_EINVAL and msg.startswith("gpd_plant_derive") and "NULL" in msg
    rc, msg = derive(ld=127)
    assert rc == _native.GPD_EINVAL and "ld <" in msg
    rc, msg = derive(rows=base + 4)
    assert rc == _native.GPD_EINVAL and "16-byte" in msg
    rc, msg = derive(E=0)
    assert rc == _native.GPD_EINVAL and msg.startswith("gpd_plant_derive")
    assert lib.gpd_plant_derive(None, base, None, 2, 64, 128, base, None) == _native.GPD_EINVAL


def test_rollout_plant_rejects_bad_arguments_before_device_work(lib):
    from gym_pybullet_drones_amd import _native
    P = _nominal()
    buf, base, st = _host_state(128, 128)
    cfg = _native.GpdStepCfg(num_envs=128, drones_per_env=1, act_type=0, substeps=1, physics_flags=0, pyb_dt=1 / 240, ctrl_dt=1 / 240,
                             inv_ctrl_dt=240.0, lanes_per_wave=64, task=0, trunc_counter=1920)

    def run(state, rows, K=20):
        rc = lib.gpd_rollout_plant(ctypes.byref(P), ctypes.byref(state), ctypes.byref(cfg), K, base, 0, None, None, base, 0, base, base,
                                   base, 0, None, rows, None)
        return rc, lib.gpd_last_error().decode()

    for K in (1, 20):                                       # one entry for step() and rollout(): the checks are the same
        rc, msg = run(st, None, K)
        assert rc == _native.GPD_EINVAL and msg == "gpd_rollout_plant: NULL plant_rows"
        rc, msg = run(st, base + 4, K)
        assert rc == _native.GPD_EINVAL and msg.startswith("gpd_rollout_plant") and "16-byte" in msg
        short = _native.GpdState(kin=base, last_rpm=base, pid=base, step_counter=base, ld=127)
        rc, msg = run(short, base, K)
        assert rc == _native.GPD_EINVAL and msg.startswith("gpd_rollout_plant") and "ld" in msg
        # a shape it does not serve: downwash computed outside the kernel (the one-world path)
        dw = _native.GpdState(kin=base, last_rpm=base, pid=base, step_counter=base, ld=128, dw_force=base)
        rc, msg = run(dw, base, K)
        assert rc == _native.GPD_ENOTSUP and msg.startswith("gpd_rollout_plant") and "dw_force" in msg
    rc, msg = run(st, base, 0)
    assert rc == _native.GPD_EINVAL and msg.startswith("gpd_rollout_plant")


@pytest.mark.parametrize("bad", [{"mass": 1.5}, {"mass": 1.0}, {"kf": -0.1}, {"ixx": math.nan}, {"km": math.inf}, {"arm": 0.1}])
def test_vector_aviary_rejects_bad_randomisation_ranges(bad):
    """0 <= r < 1 for a known field, before any device work (so it also raises on a machine without a GPU)."""
    from gym_pybullet_drones_amd.envs import VectorHoverAviary
    with pytest.raises(ValueError, match="randomize"):
        VectorHoverAviary(4, randomize=bad)


def test_compiled_unit_holds_the_plant_kernels_without_scratch():
    """The PLANT = true instantiations of the three kernel templates exist, 20 of each, built from the generic entries only (ACT from the
    argument block, the sub-step loop), and need no scratch memory; the derive kernel too.  No lookup the ISA tests make for a uniform
    kernel matches one of them."""
    from test_kernel_isa import UNIFORM_LOOKUPS, _kernel, _unit_asm
    lines = _unit_asm(0)
    labels = [m.group(1) for m in (re.match(r"^(_Z\w+):", l) for l in lines) if m]

    def targs(sym, template):         # the template arguments of an instantiation of `template`, or None
        m = re.search(r"\d+" + template + r"I((?:L[bi]n?\d+E)+)E", sym)
        return [int(a.replace("n", "-")) for a in re.findall(r"L[bi](n?\d+)E", m.group(1))] if m else None

    # template -> (number of parameters, index of ACT, index of S1); PLANT is the last parameter of each
    templates = {"gpd_step_kernel": (10, 4, 5), "gpd_rollout1_kernel": (12, 3, 4), "gpd_rollout_kernel": (7, 4, 5)}
    plant = []
    for template, (count, act, s1) in templates.items():
        found = [(l, targs(l, template)) for l in labels if targs(l, template)]
        assert found and all(len(a) == count for _, a in found), template
        mine = [(l, a) for l, a in found if a[-1] == 1]
        assert len(mine) == 20, (template, len(mine))         # 10 <PID, EXT, AW> x {single, multi}
        for sym, a in mine:
            assert a[act] == -1 and a[s1] == 0, sym
        plant += [l for l, _ in mine]
    assert len(plant) == 60, len(plant)
    derive = [l for l in labels if "gpd_plant_derive_kernel" in l]
    assert derive
    for sym in plant + derive:
        _, meta = _kernel(lines, sym[2:])          # (the helper matches `_Z\w*` + a name)
        assert re.search(r"ScratchSize: 0\b", meta), sym
    for name in UNIFORM_LOOKUPS:
        assert not [l for l in plant if re.match(r"^_Z\w*" + name + r"\w*$", l)], name

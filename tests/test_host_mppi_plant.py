"""MPPI on the aviary's own model, the part that needs no GPU: the conditions the device cases have to meet, checked on the float64
yardstick alone (tests/helpers/mppi_plant_f64.py); the binding; what the `MPPI` / `CTBRMPPI` classes construct and refuse with `model=`
and `plant=`; and the host side of `gpd_mppi_plant` against the launch stub under ASan + UBSan (tests/c/mppi_plant_host.c).  The
sanitizers run in the stand-alone program only, never in this process."""
import ctypes
import functools
import os
import re
import sys
import types

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import mppi_plant_f64 as yq  # noqa: E402

IDS = [c.name for c in yq.CASES]
#: the flags whose force acts all along a flight (GPD_PHYS_GROUND acts only on contact, which the parity cases stay clear of: the device
#: test at sigma 0 against the project's own rollout covers it)
ACTING = {"GND": yq.GND, "DRAG": yq.DRAG, "DAMP": yq.DAMP}


def test_cases_cover_the_paths_of_the_kernel():
    """a lone wave, a partial block, two blocks; one sample per lane and the sample loop; one step and five; one sub-step and five; the
    three action types; no list, a shared one, per-aviary ones; the three flag sets; with and without a table -- and every flag set and
    every table state with every action type"""
    C = yq.CASES
    both = yq.GND | yq.DRAG
    every = both | yq.GROUND | yq.DAMP
    for field, values in (("N", {1, 3, 6}), ("M", {64, 192}), ("H", {1, 5}), ("S", {1, 5}), ("act", {"rpm", "vel", "ctbr"}),
                          ("obst", {"none", "shared", "lists"}), ("flags", {0, both, every}), ("table", {False, True})):
        assert {getattr(c, field) for c in C} == values, field
    assert len({c.name for c in C}) == len(C) and 9 <= len(C) <= 12
    for act in ("rpm", "vel", "ctbr"):
        assert {c.flags for c in C if c.act == act} == {0, both, every}, act
        assert {c.table for c in C if c.act == act} == {False, True}, act
    for c in C:
        inp = yq.make_inputs(c)
        assert (inp.pos[:, 2] >= 0.10).all() and (inp.pos[:, 2] <= 0.55).all()
        assert inp.last_rpm.shape == (c.N, 4) and inp.last_rpm.dtype == np.float32
        if c.table:
            s = inp.scales
            assert s.shape == (9, c.N) and s.dtype == np.float32 and (s >= 0.8).all() and (s <= 1.25).all()
            assert c.N == 1 or all(len(set(row)) == c.N for row in s.tolist()), "the drones' rows differ in every field"
        else:
            assert inp.scales is None


@functools.lru_cache(maxsize=None)
def planned(name):
    case = next(c for c in yq.CASES if c.name == name)
    inp = yq.make_inputs(case)
    return inp, yq.plan(case, inp)


def moved(a, b):
    """the median over the samples of |a - b| / max(1, |b|)"""
    return float(np.median(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("case", yq.CASES, ids=IDS)
def test_conditions_of_the_device_cases_on_the_yardstick(case):
    """On the yardstick alone: every sample finite; no sample within 0.02 m of the ground plane (the parity cases hold no
    discontinuity); the effective sample size strictly between 2 and M / 2 (the weights are neither one sample's alone nor all equal:
    an error of the costs shows in u_out); and every acting flag the case sets, and its table, moves the float64 costs by a median
    relative difference of at least ten times the bound against the same case without it -- otherwise the device comparison could pass
    with the flag or the table never read"""
    inp, ref = planned(case.name)
    S = ref["costs"]
    assert np.isfinite(S).all() and (ref["stats"][:, 3] == case.M).all()
    z0 = yq.ground_z()
    low = float(ref["lowest"].min())
    ess = ref["stats"][:, 2]
    lo, hi = inp.lo.astype(np.float64), inp.hi.astype(np.float64)
    a = ref["a"]
    moves = {}
    for name, bit in ACTING.items():
        if case.flags & bit:
            moves[name] = moved(S, yq.rollout_costs(case, inp, a, flags=case.flags & ~bit)[0])
    if case.table:
        moves["table"] = moved(S, yq.rollout_costs(case, inp, a, scales=None)[0])
    print(f"{case.name}: costs {S.min():.3g} .. {S.max():.3g}  lowest height {low:.3f} (plane {z0:.3f})  ess {ess.round(1)}  moved "
          + "  ".join(f"{k} {v:.2e}" for k, v in moves.items()))
    assert low > z0 + 0.02
    assert (ess > 2.0).all() and (ess < case.M / 2).all(), ess
    assert all(v >= 10.0 * yq.CEILING for v in moves.values()), moves
    assert ((ref["u_out"] >= lo) & (ref["u_out"] <= hi)).all()


def test_yardstick_without_flags_and_table_is_the_models_own_yardstick():
    """flags 0 and no table: the per-drone oracles give the costs of mppi_f64 / mppi_ctbr_f64 on the same (lowered) inputs"""
    import mppi_ctbr_f64 as yc
    import mppi_f64 as y
    for case in (yq.CASES[3], yq.CASES[5], yq.CASES[8]):
        inp = yq.make_inputs(case)
        mine = yq.plan(case, inp, flags=0, scales=None)
        if case.act == "ctbr":
            b = yc.Case(case.name, "cf2x", case.N, case.M, case.H, case.S, case.obst, case.goal_per_step, case.iteration, False)
            own = yc.rollout_costs(b, inp, mine["a"])[0]
        else:
            b = y.Case(case.name, case.N, case.M, case.H, case.S, case.act, case.obst, case.goal_per_step, case.iteration)
            own = y.rollout_costs(b, inp, mine["a"])
        np.testing.assert_allclose(mine["costs"], own, rtol=1e-12)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry_and_pins_nothing_else():
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    res, args = _native._SIGNATURES["gpd_mppi_plant"]
    assert "gpd_mppi_plant" in _native.exported_symbols() and L.gpd_mppi_plant.argtypes == args and len(args) == 17 and res is ctypes.c_int
    assert args[:5] == [ctypes.POINTER(t) for t in (_native.GpdParams, _native.GpdCtbr, _native.GpdState, _native.GpdStepCfg, _native.GpdMppi)]
    assert args[5] is ctypes.c_void_p
    assert L.gpd_abi_version() == 9 and _native.ABI_VERSION == 9 and len(_native.UNITS) == 5
    assert ctypes.sizeof(_native.GpdMppi) == 104
    assert "mppi_plant.inc" in _native.HEADERS and os.path.exists(os.path.join(_native.CSRC, "mppi_plant.inc"))
    abi = open(os.path.join(_native.CSRC, "abi.hip")).read()
    assert abi.index('#include "mppi_peers.inc"') < abi.index('#include "mppi_plant.inc"')
    hdr = open(os.path.join(_native.INCLUDE, "gpd.h")).read()
    assert re.search(r"^int gpd_mppi_plant\(const GpdParams\* params, const struct GpdCtbr\* ctbr", hdr, flags=re.M)


def fake_core(act_code, physics_flags=0, dw_force=None):
    """what `_Planner._bind` reads of a core, on the CPU"""
    import torch
    from gym_pybullet_drones_amd import _native
    return types.SimpleNamespace(D=1, act_code=act_code, N=4, E=4, S=5, ld=4, device=torch.device("cpu"), physics_flags=physics_flags,
                                 P=types.SimpleNamespace(COLLISION_R=0.06),
                                 _cfg=types.SimpleNamespace(pyb_dt=1 / 240, ctrl_dt=1 / 48, inv_ctrl_dt=48.0, lanes_per_wave=64),
                                 _state=_native.GpdState(dw_force=dw_force), _params=object())


def test_classes_construct_the_nominal_model_as_before_and_refuse_what_the_aviary_model_cannot_be():
    import torch
    from gym_pybullet_drones_amd import mppi
    ctrl = types.SimpleNamespace(n=4, device=torch.device("cpu"), thrust_max=40.9, rate_max=6.28, struct=lambda: types.SimpleNamespace(g=9.8))
    every = yq.GND | yq.DRAG | yq.GROUND | yq.DAMP
    for make, entry, act in ((lambda core, **kw: mppi.MPPI(core, 5, 64, 0.3, 1.0, seed=7, **kw), "gpd_mppi", 2),
                             (lambda core, **kw: mppi.CTBRMPPI(core, ctrl, 5, 64, 0.3, 1.0, seed=7, **kw), "gpd_mppi_ctbr", 6)):
        core = fake_core(act, physics_flags=every)
        default, nominal, aviary = make(core), make(core, model="nominal"), make(core, model="aviary")
        for p in (default, nominal):
            assert p.model == "nominal" and p._ENTRY == entry and p._cfg.physics_flags == 0 and p.plant_rows is None
        assert bytes(default._q) == bytes(nominal._q) == bytes(aviary._q) and ctypes.sizeof(default._q) == 104
        assert bytes(default._cfg) == bytes(nominal._cfg)
        assert aviary.model == "aviary" and aviary._cfg.physics_flags == every and aviary.plant_rows is None
        assert (aviary._ctbr() is None) == (act == 2)
        with pytest.raises(ValueError, match="downwash"):
            make(fake_core(act, physics_flags=yq.GND | yq.DW), model="aviary")
        with pytest.raises(ValueError, match="downwash"):
            make(fake_core(act, dw_force=64), model="aviary")
        make(fake_core(act, physics_flags=yq.GND | yq.DW))                   # (the nominal model does not look at the core's flags)
        for kw in (dict(plant={"mass": 1.2}), dict(plant={"mass": 1.2}, model="nominal")):
            with pytest.raises(ValueError, match="aviary"):
                make(core, **kw)
        with pytest.raises(ValueError, match="model must be"):
            make(core, model="identified")
        with pytest.raises(ValueError, match="aviary"):
            default.set_plant({"mass": 1.2})
    import inspect
    from gym_pybullet_drones_amd.envs.VectorAviary import VectorAviary
    for f in (VectorAviary.mppi, VectorAviary.mppi_ctbr, mppi.MPPI.__init__, mppi.CTBRMPPI.__init__):
        sig = inspect.signature(f).parameters
        assert sig["model"].default == "nominal" and sig["plant"].default is None
    assert "model" not in inspect.signature(mppi.SwarmMPPI.__init__).parameters and "plant" not in inspect.signature(VectorAviary.mppi_swarm).parameters


# ---- the host side of the entry -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_run():
    import host_lib
    from gym_pybullet_drones_amd import _native
    return host_lib.run(host_lib.program("mppi_plant_host", include=(_native.CSRC,)))


def test_host_side_of_the_entry_under_asan_and_ubsan():
    """tests/c/mppi_plant_host.c linked to the host-only build of the units and the launch stub under -fsanitize=address,undefined: a good
    call launches the instantiation model x list x flags x table that the arguments select, every refusal -- the entry's own (downwash,
    a misaligned table, drag without the last RPMs) and everything gpd_mppi / gpd_mppi_ctbr refuse -- has its code, the entry's name and
    the reason, and launches nothing"""
    run = host_run()
    print(run.stdout[-8000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") >= 80 and "FAIL" not in run.stdout
    for piece in ("<VEL, OBST, EXT, PLANT>", "<VEL, no OBST, EXT, no PLANT>", "<VEL, OBST, no EXT, PLANT>", "<RPM, OBST, EXT, PLANT>",
                  "<RPM, no OBST, no EXT, no PLANT>", "<CTBR, OBST, EXT, PLANT>", "<CTBR, no OBST, EXT, no PLANT>", "<CTBR, OBST, no EXT, PLANT>"):
        assert f"{piece}\n" in run.stdout, piece

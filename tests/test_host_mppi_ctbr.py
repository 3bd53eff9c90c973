"""MPPI over thrust and body-rate commands, the part that needs no GPU: the conditions every device case has to meet, checked on the
float64 yardstick alone (tests/helpers/mppi_ctbr_f64.py); every refusal of `gpd_mppi_ctbr` with its code and message (all before the
first device call); the binding; the `CTBRMPPI` class's own refusals; and the host side of the entry against the launch stub under
ASan + UBSan (tests/c/mppi_ctbr_host.c).  The sanitizers run in the stand-alone program only, never in this process."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import mppi_ctbr_f64 as yc  # noqa: E402
import mppi_f64 as y  # noqa: E402

IDS = [c.name for c in yc.CASES]


# ---- the device cases on the yardstick: are they worth running, and what may float32 cost on them? ----------------------------------
@pytest.fixture(scope="module")
def plans():
    return {c.name: (yc.make_inputs(c), yc.plan(c)) for c in yc.CASES}


def test_cases_cover_the_paths_of_the_kernel():
    """a lone wave, a partial block and two blocks; one sample per lane and the sample loop; one step and five; one sub-step and five;
    no list, a shared one, per-aviary ones; one goal and one per step; two iteration words; both kinds of bounds; the three airframes"""
    C = yc.CASES
    for field, values in (("N", {1, 3, 6}), ("M", {64, 192}), ("H", {1, 5}), ("S", {1, 5}), ("obst", {"none", "shared", "lists"}),
                          ("goal_per_step", {False, True}), ("iteration", {0, 7}), ("wide", {False, True}), ("model", {"cf2x", "cf2p", "racer"})):
        assert {getattr(c, field) for c in C} == values, field
    assert len({c.name for c in C}) == len(C)
    outside = [c for c in C if ((yc.make_inputs(c).u_in < yc.make_inputs(c).lo) | (yc.make_inputs(c).u_in > yc.make_inputs(c).hi)).any()]
    assert outside, "no nominal row outside the bounds"
    import ctbr_f64
    for c in C:
        inp = yc.make_inputs(c)
        beyond = inp.hi[0] > ctbr_f64.THRUST_MAX and (inp.hi[1:] > ctbr_f64.RATE_MAX).all() and (inp.lo[1:] < -ctbr_f64.RATE_MAX).all()
        within = 0.0 <= inp.lo[0] and inp.hi[0] <= ctbr_f64.THRUST_MAX and (np.abs(inp.lo[1:]) <= ctbr_f64.RATE_MAX).all() and (inp.hi[1:] <= ctbr_f64.RATE_MAX).all()
        assert beyond if c.wide else within, c.name


@pytest.mark.parametrize("case", yc.CASES, ids=IDS)
def test_device_cases_meet_their_conditions_on_the_yardstick(plans, case):
    """Every case: finite costs, all M samples counted; an effective sample size above 1.5 for every drone and below 0.95 M for some (the
    weights do something); clamped and unclamped action components; where the bounds are wider than the controller's clips, samples
    with a rotor held at 0, samples with one at f_max, and samples without (the rate loop's clips and the rotor limits act, and not
    everywhere); with a list, samples inside the hinge.  And the conditioning: a relative error of 1e-6 in every cost moves u_out by
    less than 1e-5, so that a device result within the project's 1e-4 is a statement about the kernel and not about the softmax."""
    inp, ref = plans[case.name]
    S, ess = ref["costs"], ref["stats"][:, 2]
    assert np.isfinite(S).all() and (ref["stats"][:, 3] == case.M).all()
    assert (ess > 1.5).all() and (ess < 0.95 * case.M).any()
    at_bound = (ref["a"] == inp.lo) | (ref["a"] == inp.hi)
    assert 0.005 < at_bound.mean() < 0.5
    if case.wide:
        for flag in (ref["at_zero"], ref["at_max"]):
            assert flag.any() and not flag.all()
    touched = None
    if inp.obst is not None:
        without = yc.plan(case, inp._replace(obst=None))["costs"]
        touched = float(((S - without) > 1e-9).mean())
        assert touched > 0.05 and (S >= without - 1e-12).all()
    rng = np.random.default_rng(1)
    worst = 0.0
    lo, hi = inp.lo.astype(np.float64), inp.hi.astype(np.float64)
    for _ in range(4):
        moved, _ = y.update(inp.u_in, ref["a"], S * (1.0 + 1e-6 * rng.uniform(-1.0, 1.0, size=S.shape)), inp.lam, lo, hi)
        worst = max(worst, float(y.rel_err(moved, ref["u_out"]).max()))
    print(f"{case.name}: lambda {inp.lam:.3g} costs {S.min():.3g} .. {S.max():.3g} ess {ess.round(1)} at a bound {at_bound.mean():.3f} "
          f"rotor at 0 {ref['at_zero'].mean():.3f} at f_max {ref['at_max'].mean():.3f} hinge {touched} d u_out for 1e-6 of the costs {worst:.2e}")
    assert worst < 1e-5


@pytest.mark.parametrize("case", yc.CASES, ids=IDS)
def test_float32_storage_run_follows_the_float64_one_on_the_device_cases(plans, case):
    """The yardstick run again with everything it carries from step to step, its actions and every cost term rounded to float32: u_out
    and the costs stay within 1e-5 of the float64 run"""
    inp, ref = plans[case.name]
    got = yc.plan(case, inp, store32=True)
    eu, ec = float(y.rel_err(got["u_out"], ref["u_out"]).max()), float((np.abs(got["costs"] - ref["costs"]) / np.abs(ref["costs"])).max())
    print(f"{case.name}: float32 storage against float64: u_out {eu:.2e} costs {ec:.2e}")
    assert eu < 1e-5 and ec < 1e-5


def test_yardstick_without_noise_flies_the_clamped_nominal():
    """sigma = 0: every sample's cost is one value, that of CtbrF64 flying clamp(u_in) and scored from its observations -- the
    composition adds nothing of its own (1e-7: cos(roll) cos(pitch) is R22 of the NORMALISED quaternion, and the float32 start
    quaternion is off unit length by 6e-8)"""
    import ctbr_f64
    case = yc.CASES[2]
    inp = yc.make_inputs(case)._replace(sigma=np.zeros(4, dtype=np.float32), obst=None)
    ref = yc.plan(case, inp)
    assert (ref["costs"] == ref["costs"][:, :1]).all() and (ref["stats"][:, 2] == case.M).all()
    np.testing.assert_array_equal(ref["u_out"], np.clip(inp.u_in.astype(np.float64), inp.lo, inp.hi))
    sim = ctbr_f64.CtbrF64(case.model, case.N, pos=inp.pos, quat=inp.quat, vel=inp.vel, w=inp.rates, pyb_freq=240, ctrl_freq=240 // case.S)
    obs = sim.run(np.clip(inp.u_in.astype(np.float64), inp.lo, inp.hi), case.H)
    np.testing.assert_allclose(yc.nominal_costs(case, inp, obs), ref["costs"][:, 0], rtol=1e-7)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry_and_pins_nothing_else():
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    res, args = _native._SIGNATURES["gpd_mppi_ctbr"]
    assert "gpd_mppi_ctbr" in _native.exported_symbols() and L.gpd_mppi_ctbr.argtypes == args and len(args) == 16 and res is ctypes.c_int
    assert args[:5] == [ctypes.POINTER(t) for t in (_native.GpdParams, _native.GpdCtbr, _native.GpdState, _native.GpdStepCfg, _native.GpdMppi)]
    assert L.gpd_abi_version() == 9 and _native.ABI_VERSION == 9 and len(_native.UNITS) == 5
    assert "mppi_ctbr.inc" in _native.HEADERS and os.path.exists(os.path.join(_native.CSRC, "mppi_ctbr.inc"))
    assert ctypes.sizeof(_native.GpdMppi) == 104 and ctypes.sizeof(_native.GpdCtbr) == 128
    hdr = open(os.path.join(_native.INCLUDE, "gpd.h")).read()
    assert "int gpd_mppi_ctbr(const GpdParams* params, const struct GpdCtbr* ctbr, const GpdState* state, const GpdStepCfg* cfg, const GpdMppi* mppi," in hdr
    abi = open(os.path.join(_native.CSRC, "abi.hip")).read()
    assert abi.index('#include "mppi.inc"') < abi.index('#include "ctbr.inc"') < abi.index('#include "mppi_ctbr.inc"')


# ---- the entry's refusals ---------------------------------------------------------------------------------------------------------------
def test_entry_rejects_bad_arguments_before_touching_a_device():
    """Every argument error of gpd_mppi_ctbr is found before the first HIP call: the code include/gpd.h states and a message that starts
    with the entry's name (host buffers stand in for device memory: nothing is launched)"""
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.control.CTBRControl import to_struct as ctbr_struct
    from gym_pybullet_drones_amd.params import DroneParams
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    L = _native.lib()
    buf = (ctypes.c_float * 65536)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    F4 = ctypes.c_float * 4
    cfg0 = dict(num_envs=70, drones_per_env=1, act_type=6, substeps=5, physics_flags=0, pyb_dt=1 / 240, ctrl_dt=1 / 48, inv_ctrl_dt=48.0,
                lanes_per_wave=64, task=0, auto_reset=0)
    q0 = dict(horizon=5, samples=192, sigma=(2.0,) * 4, act_lo=(0.0, -6.0, -6.0, -6.0), act_hi=(40.0, 6.0, 6.0, 6.0), lam=0.5, w_pos=1.0, w_term=2.0,
              seed=(1, 2), iteration=0)
    st0 = dict(kin=base, step_counter=base + 8192, ld=128)
    arg0 = dict(u_in=base + 32768, u_stride=280, goal=base + 49152, goal_stride=0, obst=base + 65536, n_obst=7, obst_ld=70, u_out=base + 81920,
                costs=base + 98304, stats=base + 114688)
    dp = DroneParams(DroneModel.CF2X)
    P, B = dp.to_struct(), ctbr_struct(dp)

    def rc(cfg=None, q=None, st=None, null=None, **args):
        qq = {**q0, **(q or {})}
        Q = _native.GpdMppi(**{**qq, "sigma": F4(*qq["sigma"]), "act_lo": F4(*qq["act_lo"]), "act_hi": F4(*qq["act_hi"]), "seed": (ctypes.c_uint32 * 2)(*qq["seed"])})
        a = {**arg0, **args}
        lead = dict(params=ctypes.byref(P), ctbr=ctypes.byref(B), state=ctypes.byref(_native.GpdState(**{**st0, **(st or {})})),
                    cfg=ctypes.byref(_native.GpdStepCfg(**{**cfg0, **(cfg or {})})), mppi=ctypes.byref(Q))
        if null:
            lead[null] = None
        return L.gpd_mppi_ctbr(*lead.values(), *[a[k] for k in arg0], None)

    def rejected(code, reason, **change):
        assert rc(**change) == code, change
        msg = L.gpd_last_error().decode()
        assert msg.startswith("gpd_mppi_ctbr: ") and reason in msg, (change, msg)

    EINVAL, ERANGE, ENOTSUP = _native.GPD_EINVAL, _native.GPD_ERANGE, _native.GPD_ENOTSUP
    for name in ("params", "ctbr", "state", "cfg", "mppi"):
        rejected(EINVAL, "NULL", null=name)
    for name in ("u_in", "goal", "u_out", "costs", "stats"):
        rejected(EINVAL, "NULL", **{name: None})
    rejected(EINVAL, "NULL", st=dict(kin=None))
    rejected(EINVAL, "NULL", st=dict(step_counter=None))
    rejected(EINVAL, "aligned", st=dict(kin=base + 4))
    rejected(EINVAL, "state.ld", st=dict(ld=64))
    for m in (0, 32, 100, 1088, -64):
        rejected(EINVAL, "samples", q=dict(samples=m))
    for h in (0, -1):
        rejected(EINVAL, "horizon", q=dict(horizon=h))
    for lam in (0.0, -1.0, float("inf"), float("nan")):
        rejected(EINVAL, "lambda", q=dict(lam=lam))
    for s in (-0.1, float("inf"), float("nan")):
        rejected(EINVAL, "sigma", q=dict(sigma=(2.0, 2.0, s, 2.0)))
    rejected(EINVAL, "act_lo", q=dict(act_lo=(0.0, 0.5, -1.0, -1.0), act_hi=(40.0, 0.25, 1.0, 1.0)))
    rejected(EINVAL, "act_lo", q=dict(act_lo=(float("nan"),) * 4))
    rejected(EINVAL, "alias", u_out=arg0["u_in"])
    for name in ("u_in", "u_out", "goal", "stats"):
        rejected(EINVAL, "aligned", **{name: arg0[name] + 4})
    for s in (276, 282, -280):
        rejected(EINVAL, "stride", u_stride=s)
    for s in (-4, 8, 281):
        rejected(EINVAL, "stride", goal_stride=s)
    for m in (-1, 1025):
        rejected(EINVAL, "n_obst", n_obst=m)
    for ld in (69, 1, -1):
        rejected(EINVAL, "obst_ld", obst_ld=ld)
    rejected(EINVAL, "positive", cfg=dict(substeps=0))
    rejected(EINVAL, "positive", cfg=dict(num_envs=0))
    rejected(EINVAL, "act_type", cfg=dict(act_type=9))
    rejected(EINVAL, "task", cfg=dict(task=9))
    rejected(EINVAL, "unknown physics flag", cfg=dict(physics_flags=32))
    rejected(ERANGE, "2^26", cfg=dict(num_envs=2 ** 26 + 1), st=dict(ld=2 ** 26 + 64))
    rejected(ENOTSUP, "drones_per_env", cfg=dict(drones_per_env=2, num_envs=35))
    for flag in (1, 2, 4, 8, 16, 3):
        rejected(ENOTSUP, "physics_flags", cfg=dict(physics_flags=flag))
    rejected(ENOTSUP, "episode", cfg=dict(task=1))
    rejected(ENOTSUP, "episode", cfg=dict(auto_reset=1))
    for act in (0, 1, 2, 3, 4):
        rejected(ENOTSUP, "act_type", cfg=dict(act_type=act))


def test_python_class_rejects_what_the_entry_would_before_any_device_work():
    from gym_pybullet_drones_amd import mppi

    class Core:
        D, act_code, N, device = 2, 6, 4, "cpu"

    class Ctrl:
        n, device, thrust_max, rate_max = 4, "cpu", 40.9, 6.28
    with pytest.raises(ValueError, match="one drone"):
        mppi.CTBRMPPI(Core(), Ctrl(), 5, 64, 1.0, 1.0)
    Core.D = 1
    for act in (0, 1, 2, 3, 4):
        Core.act_code = act
        with pytest.raises(ValueError, match="RAW_RPM or DIRECT_RPM"):
            mppi.CTBRMPPI(Core(), Ctrl(), 5, 64, 1.0, 1.0)
    Core.act_code = 5
    for change in (dict(n=3), dict(device="cuda:0")):
        with pytest.raises(ValueError, match="VectorCTBR of 4 controllers"):
            mppi.CTBRMPPI(Core(), type("Other", (Ctrl,), change)(), 5, 64, 1.0, 1.0)
    with pytest.raises(ValueError, match="VectorCTBR of 4 controllers"):
        mppi.CTBRMPPI(Core(), object(), 5, 64, 1.0, 1.0)
    for bad in (dict(horizon=0), dict(samples=100), dict(samples=2048), dict(lam=0.0), dict(lam=float("inf")), dict(sigma=(1.0, 1.0))):
        kw = {**dict(horizon=5, samples=64, sigma=1.0, lam=1.0), **bad}
        with pytest.raises(ValueError):
            mppi.CTBRMPPI(Core(), Ctrl(), **kw)
    assert issubclass(mppi.CTBRMPPI, mppi._Planner) and issubclass(mppi.MPPI, mppi._Planner)
    for name in ("plan", "advance", "reset", "nominal"):                # shared, not copied
        assert getattr(mppi.CTBRMPPI, name) is getattr(mppi.MPPI, name)
    from gym_pybullet_drones_amd.envs.VectorAviary import VectorCtrlAviary
    assert callable(VectorCtrlAviary.mppi_ctbr)


# ---- the host side of the entry ---------------------------------------------------------------------------------------------------------
def test_host_side_of_the_entry_under_asan_and_ubsan():
    """tests/c/mppi_ctbr_host.c linked to the host-only build of the units and the launch stub under -fsanitize=address,undefined: the
    accepted calls launch the variant the list selects, every refusal has its code, the entry's name and the reason, and launches
    nothing"""
    import host_lib
    from gym_pybullet_drones_amd import _native
    run = host_lib.run(host_lib.program("mppi_ctbr_host", include=(_native.CSRC,)))
    print(run.stdout[-6000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") >= 65 and "FAIL" not in run.stdout

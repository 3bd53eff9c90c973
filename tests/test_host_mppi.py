"""Sampling-based MPC, the part that needs no GPU: the float64 yardstick (tests/helpers/mppi_f64.py) pinned by known answers -- the
Philox vectors, the update's limits --, csrc/mppi_math.inc compiled for the host under ASan + UBSan (tests/c/mppi_host.c) against it:
the generator bit for bit, the normals within a measured bound, their moments; the conditioning of the device cases; every refusal of
`gpd_mppi` with its code and message (all before the first device call); and the host side of the entry against the launch stub.
The sanitizers run in the stand-alone program only, never in this process."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import mppi_f64 as y  # noqa: E402

#: counter / key -> output of Philox4x32-10 (the first two are Random123's own known answers)
PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


# ---- the noise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,out", PHILOX_KAT)
def test_yardstick_philox_known_answers(ctr, key, out):
    assert tuple(int(v) for v in y.philox(np.array(ctr), np.array(key))) == out


def test_uniforms_are_the_float32_values_and_never_zero():
    """((x >> 8) + 0.5) 2^-24 needs 25 significant bits from 2^23 on: the float32 sum rounds to even there, so the top word gives
    exactly 1 (whose logarithm is 0); the yardstick uses those float32 values, which float64 holds exactly"""
    u = y.uniforms(np.array([0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0x800001ff, 0xffffffff], dtype=np.uint64))
    assert list(u) == [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, (2 ** 23 - 0.5) * 2.0 ** -24, 0.5, (2 ** 23 + 2) * 2.0 ** -24, 1.0]
    z = y.box_muller(np.array([[0xffffffff, 0x40000000, 0, 0]], dtype=np.uint64))
    assert np.isfinite(z).all() and z[0, 0] == 0 and z[0, 1] == 0


@pytest.fixture(scope="module")
def host_exe():
    import host_lib
    from gym_pybullet_drones_amd import _native
    return host_lib.program("mppi_host", include=(_native.CSRC,))


def test_host_compiled_philox_is_the_yardsticks_bit_for_bit(host_exe, tmp_path):
    import host_lib
    rng = np.random.default_rng(11)
    words = rng.integers(0, 2 ** 32, size=(10000, 6), dtype=np.uint64)
    words[:3] = [list(c) + list(k) for c, k, _ in PHILOX_KAT]
    src, dst = str(tmp_path / "counters.bin"), str(tmp_path / "words.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(words)], dtype=np.int32).tobytes())
        f.write(words.astype(np.uint32).tobytes())
    res = host_lib.run(host_exe, "philox", src, dst)
    assert res.returncode == 0 and "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    got = np.fromfile(dst, dtype=np.uint32).reshape(-1, 4)
    np.testing.assert_array_equal(got, y.philox(words[:, :4], words[:, 4:]))
    assert [tuple(int(v) for v in r) for r in got[:3]] == [o for _, _, o in PHILOX_KAT]


#: 3 x the largest |z32 - z64| the host-compiled normals show against the float64 ones over the 10^6 below (1.6e-6: the float32
#: rounding of 2 pi u2 and of r, both times a value up to ~5): DESIGN.md 3.15
NORMALS_BOUND = 4.8e-6


@pytest.fixture(scope="module")
def host_normals(host_exe, tmp_path_factory):
    """10^6 normals of the host-compiled generator -- counters (n < 5, m < 1000, h < 50), iteration 3 -- and the yardstick's"""
    import host_lib
    dst = str(tmp_path_factory.mktemp("mppi") / "normals.bin")
    seed = (0xDEADBEEF, 0x12345678)
    res = host_lib.run(host_exe, "normals", "5", "1000", "50", "3", str(seed[0]), str(seed[1]), dst)
    assert res.returncode == 0 and "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    return np.fromfile(dst, dtype=np.float32).reshape(5, 1000, 50, 4), y.normals(5, 1000, 50, 3, seed)


def test_host_compiled_normals_follow_the_float64_ones(host_normals):
    z32, z64 = host_normals
    err = float(np.abs(z32.astype(np.float64) - z64).max())
    print(f"MEASURED host normals: max |z32 - z64| = {err:.3e} over {z64.size} values, max |z| = {np.abs(z64).max():.2f}")
    assert NORMALS_BOUND <= y.CEILING and err <= NORMALS_BOUND


def test_moments_of_a_million_normals(host_normals):
    """mean, variance and kurtosis within 5 standard errors of a standard normal's (n = 10^6: 1/sqrt(n), sqrt(2/n), sqrt(96/n) for the
    fourth moment), per component too: the two members of a Box-Muller pair are not favoured"""
    for z in host_normals:
        z = z.astype(np.float64).reshape(-1, 4)
        for col in (z.reshape(-1), z[:, 0], z[:, 1], z[:, 2], z[:, 3]):
            n = col.size
            assert abs(col.mean()) < 5.0 / np.sqrt(n)
            assert abs(col.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
            assert abs((col ** 4).mean() - 3.0) < 5.0 * np.sqrt(96.0 / n)
        assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 5.0 / np.sqrt(len(z))


# ---- the update on the yardstick: known answers ---------------------------------------------------------------------------------------
def _samples(seed=0, N=2, M=64, H=3, sigma=(0.5, 0.4, 0.3, 0.2)):
    rng = np.random.default_rng(seed)
    u_in = rng.uniform(-0.9, 0.9, size=(H, N, 4)).astype(np.float32)
    u_in[0, 0] = [1.5, -1.25, 0.25, 1.5]
    lo, hi = np.full(4, -1.0), np.full(4, 1.0)
    a = y.perturbed(u_in, sigma, lo, hi, M, 5, (1, 2))
    return u_in, a, rng.uniform(1.0, 3.0, size=(N, M)), lo, hi


def test_update_without_noise_returns_the_clamped_nominal():
    u_in, a, S, lo, hi = _samples(sigma=(0, 0, 0, 0))
    u_out, stats = y.update(u_in, a, np.ones_like(S), 0.7, lo, hi)
    np.testing.assert_array_equal(u_out, np.clip(u_in.astype(np.float64), lo, hi))
    assert list(stats[:, 2]) == [64.0, 64.0] and list(stats[:, 3]) == [64.0, 64.0]


def test_update_limits_of_the_temperature():
    u_in, a, S, lo, hi = _samples()
    u64 = u_in.astype(np.float64).transpose(1, 0, 2)
    hot, stats = y.update(u_in, a, S, 1e12, lo, hi)                 # every weight 1: the plain mean of the clamped perturbations
    np.testing.assert_allclose(hot.transpose(1, 0, 2) - u64, (a - u64[:, None]).mean(axis=1), atol=1e-10)
    np.testing.assert_allclose(stats[:, 2], 64.0, rtol=1e-9)
    cold, stats = y.update(u_in, a, S, 1e-6, lo, hi)                # one weight 1: the argmin sample's sequence
    best = S.argmin(axis=1)
    np.testing.assert_allclose(cold.transpose(1, 0, 2), a[np.arange(len(S)), best], atol=1e-12)
    np.testing.assert_allclose(stats[:, 2], 1.0, rtol=1e-9)
    np.testing.assert_allclose(stats[:, 0], S.min(axis=1))
    np.testing.assert_allclose(stats[:, 1], S.min(axis=1))


def test_update_gives_a_cost_that_is_not_finite_no_weight():
    u_in, a, S, lo, hi = _samples()
    ref, _ = y.update(u_in, np.delete(a, 7, axis=1), np.delete(S, 7, axis=1), 0.5, lo, hi)
    for bad in (np.nan, np.inf):
        S2 = S.copy()
        S2[:, 7] = bad
        u_out, stats = y.update(u_in, a, S2, 0.5, lo, hi)
        np.testing.assert_allclose(u_out, ref, atol=1e-14)
        assert list(stats[:, 3]) == [63.0, 63.0] and np.isfinite(stats).all()
    S2 = S.copy()
    S2[1] = np.nan                                                    # a drone with no finite sample: its nominal, clamped
    u_out, stats = y.update(u_in, a, S2, 0.5, lo, hi)
    np.testing.assert_array_equal(u_out[:, 1], np.clip(u_in[:, 1].astype(np.float64), lo, hi))
    assert list(stats[1]) == [np.inf, np.inf, 0.0, 0.0] and stats[0, 3] == 64


# ---- the device cases on the yardstick: are they worth running, and what may float32 cost on them? -----------------------------------------
@pytest.fixture(scope="module")
def plans():
    return {c.name: (y.make_inputs(c), y.plan(c)) for c in y.CASES}


@pytest.mark.parametrize("case", y.CASES, ids=[c.name for c in y.CASES])
def test_device_cases_have_softmax_weights_that_matter_and_are_well_conditioned(plans, case):
    """Every case: finite costs; drones whose effective sample size is neither 1 nor M (the weights do something); clamped and
    unclamped samples; with a list, samples inside and outside the hinge.  And the conditioning: a relative error of 1e-6 in every
    cost -- what float32 leaves of a sum of a few squares -- moves u_out by less than 1e-5, so that a device result within the project's
    1e-4 is a statement about the kernel and not about the softmax"""
    inp, ref = plans[case.name]
    S, ess = ref["costs"], ref["stats"][:, 2]
    assert np.isfinite(S).all() and (ref["stats"][:, 3] == case.M).all()
    assert (ess > 1.5).all() and (ess < 0.95 * case.M).any()
    at_bound = (ref["a"] == inp.lo) | (ref["a"] == inp.hi)
    assert 0.005 < at_bound.mean() < 0.5
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(4):
        moved, _ = y.update(inp.u_in, ref["a"], S * (1.0 + 1e-6 * rng.uniform(-1.0, 1.0, size=S.shape)), inp.lam, inp.lo.astype(np.float64), inp.hi.astype(np.float64))
        worst = max(worst, float(y.rel_err(moved, ref["u_out"]).max()))
    print(f"{case.name}: lambda {inp.lam:.3g} costs {S.min():.3g} .. {S.max():.3g} ess {ess.round(1)} d u_out for 1e-6 of the costs {worst:.2e}")
    assert worst < 1e-5


@pytest.mark.parametrize("case", y.CASES, ids=[c.name for c in y.CASES])
def test_float32_storage_run_follows_the_float64_one_on_the_device_cases(plans, case):
    """The restatement run again with everything it carries from step to step, its actions and every cost term rounded to float32 (the
    oracle's arithmetic inside a step has no float32 form, so this is float32 STORAGE, not float32 arithmetic): u_out and the costs stay
    within 1e-5 of the float64 run -- the rule of tests/test_host_diff.py for choosing lambda and the weights"""
    inp, ref = plans[case.name]
    got = y.plan(case, inp, store32=True)
    eu, ec = float(y.rel_err(got["u_out"], ref["u_out"]).max()), float((np.abs(got["costs"] - ref["costs"]) / np.abs(ref["costs"])).max())
    print(f"{case.name}: float32 storage against float64: u_out {eu:.2e} costs {ec:.2e}")
    assert eu < 1e-5 and ec < 1e-5


def test_the_hinge_is_active_for_some_samples_and_not_for_others():
    case = y.CASES[2]
    inp = y.make_inputs(case)
    with_list = y.plan(case, inp)["costs"]
    without = y.plan(case, inp._replace(obst=None))["costs"]
    touched = (with_list - without) > 1e-9
    assert 0.05 < touched.mean() and (with_list >= without - 1e-12).all()


# ---- the entry's refusals ---------------------------------------------------------------------------------------------------------------
def test_entry_rejects_bad_arguments_before_touching_a_device():
    """Every argument error of gpd_mppi is found before the first HIP call: the code include/gpd.h states and a message that starts
    with the entry's name (host buffers stand in for device memory: nothing is launched)"""
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.params import DroneParams
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    L = _native.lib()
    assert "gpd_mppi" in _native.exported_symbols() and L.gpd_abi_version() == 9 and {"mppi.inc", "mppi_math.inc"} <= set(_native.HEADERS)
    buf = (ctypes.c_float * 65536)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    F4 = ctypes.c_float * 4
    cfg0 = dict(num_envs=70, drones_per_env=1, act_type=2, substeps=5, physics_flags=0, pyb_dt=1 / 240, ctrl_dt=1 / 48, inv_ctrl_dt=48.0,
                lanes_per_wave=64, task=0, auto_reset=0)
    q0 = dict(horizon=5, samples=192, sigma=(0.3,) * 4, act_lo=(-1.0,) * 4, act_hi=(1.0,) * 4, lam=0.5, w_pos=1.0, w_term=2.0, seed=(1, 2), iteration=0)
    st0 = dict(kin=base, step_counter=base + 8192, pid=base + 16384, ld=128)
    arg0 = dict(u_in=base + 32768, u_stride=280, goal=base + 49152, goal_stride=0, obst=base + 65536, n_obst=7, obst_ld=70, u_out=base + 81920,
                costs=base + 98304, stats=base + 114688)

    def rc(cfg=None, q=None, st=None, no_pid=False, **args):
        P = DroneParams(DroneModel.CF2X).to_struct(pid_model=DroneModel.CF2X)
        if no_pid:
            P.pid_kf = 0.0
        qq = {**q0, **(q or {})}
        Q = _native.GpdMppi(**{**qq, "sigma": F4(*qq["sigma"]), "act_lo": F4(*qq["act_lo"]), "act_hi": F4(*qq["act_hi"]), "seed": (ctypes.c_uint32 * 2)(*qq["seed"])})
        a = {**arg0, **args}
        return L.gpd_mppi(ctypes.byref(P), ctypes.byref(_native.GpdState(**{**st0, **(st or {})})), ctypes.byref(_native.GpdStepCfg(**{**cfg0, **(cfg or {})})),
                          ctypes.byref(Q), *[a[k] for k in arg0], None)

    def rejected(code, reason, **change):
        assert rc(**change) == code, change
        msg = L.gpd_last_error().decode()
        assert msg.startswith("gpd_mppi: ") and reason in msg, (change, msg)

    EINVAL, ERANGE, ENOTSUP = _native.GPD_EINVAL, _native.GPD_ERANGE, _native.GPD_ENOTSUP
    for name in ("u_in", "goal", "u_out", "costs", "stats"):
        rejected(EINVAL, "NULL", **{name: None})
    rejected(EINVAL, "NULL", st=dict(kin=None))
    rejected(EINVAL, "aligned", st=dict(kin=base + 4))
    rejected(EINVAL, "state.ld", st=dict(ld=64))
    for m in (0, 32, 100, 1088, -64):
        rejected(EINVAL, "samples", q=dict(samples=m))
    for h in (0, -1):
        rejected(EINVAL, "horizon", q=dict(horizon=h))
    for lam in (0.0, -1.0, float("inf"), float("nan")):
        rejected(EINVAL, "lambda", q=dict(lam=lam))
    for s in (-0.1, float("inf"), float("nan")):
        rejected(EINVAL, "sigma", q=dict(sigma=(0.3, 0.3, s, 0.3)))
    rejected(EINVAL, "act_lo", q=dict(act_lo=(-1.0, 0.5, -1.0, -1.0), act_hi=(1.0, 0.25, 1.0, 1.0)))
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
    rejected(EINVAL, "state.pid", st=dict(pid=None))
    rejected(EINVAL, "positive", cfg=dict(substeps=0))
    rejected(EINVAL, "act_type", cfg=dict(act_type=9))
    rejected(ERANGE, "2^26", cfg=dict(num_envs=2 ** 26 + 1), st=dict(ld=2 ** 26 + 64))
    rejected(ENOTSUP, "drones_per_env", cfg=dict(drones_per_env=2, num_envs=35))
    for flag in (1, 2, 4, 8, 16, 3):
        rejected(ENOTSUP, "physics_flags", cfg=dict(physics_flags=flag))
    rejected(ENOTSUP, "episode", cfg=dict(task=1))
    rejected(ENOTSUP, "episode", cfg=dict(auto_reset=1))
    for act in (1, 3, 4, 5, 6):
        rejected(ENOTSUP, "act_type", cfg=dict(act_type=act))
    rejected(ENOTSUP, "DSLPID", no_pid=True)


def test_python_class_rejects_what_the_entry_would_before_any_device_work():
    from gym_pybullet_drones_amd import mppi

    class Core:
        D, act_code = 2, 2
    with pytest.raises(ValueError, match="one drone"):
        mppi.MPPI(Core(), 5, 64, 0.3, 1.0)
    Core.D, Core.act_code = 1, 1
    with pytest.raises(ValueError, match="RPM or VEL"):
        mppi.MPPI(Core(), 5, 64, 0.3, 1.0)
    assert mppi.DEFAULT_BOUNDS[mppi.ACT_RPM] == ((-1.0,) * 4, (1.0,) * 4) and mppi.DEFAULT_BOUNDS[mppi.ACT_VEL] == ((-1.0, -1.0, -1.0, 0.0), (1.0,) * 4)
    assert ctypes.sizeof(__import__("gym_pybullet_drones_amd")._native.GpdMppi) == 104


def test_host_side_of_the_entry_under_asan_and_ubsan(host_exe):
    """tests/c/mppi_host.c linked to the host-only build of the units and the launch stub under -fsanitize=address,undefined: the
    accepted calls launch the variant the action type and the list select, every refusal has its code, the entry's name and the
    reason, and launches nothing; the corner values of mppi_math.inc"""
    import host_lib
    run = host_lib.run(host_exe)
    print(run.stdout[-6000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") >= 60 and "FAIL" not in run.stdout

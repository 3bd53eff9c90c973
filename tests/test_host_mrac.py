"""MRAC, the parts that need no GPU: the float64 restatement against the reference's recorded calls, the product's design against
the reference's, the argument checks of the three entries, the ISA fences on the cross-compiled `mrac.hip`, and the package's
independence from scipy.  Fixtures: tests/golden/make_golden_mrac.py (the reference's unmodified `control/MRAC.py` + `CtrlAviary`)."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, golden

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
from mrac_f64 import MracF64, rel_err  # noqa: E402

MODELS = ("cf2x", "cf2p")
#: float64 rounding of the same statements evaluated through other library routes (numpy instead of pybullet / scipy Rotation):
#: measured <= 4.5e-14 over every recorded call and all 3 x 720 steps of the closed loops
F64_BOUND = 1e-12


# ---- 1. the float64 restatement is the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", ["calls", "calls_wide"])
@pytest.mark.parametrize("model", MODELS)
def test_restatement_reproduces_the_recorded_calls(model, calls):
    """`calls`: 72 calls of the recorded flight + 64 random near level; `calls_wide`: 64 calls with roll and yaw in every quadrant"""
    d, c = golden(f"mrac_design_{model}"), golden(f"mrac_{calls}_{model}")
    if calls == "calls_wide":
        rpy = c["target_rpy"] - c["rpy_e"]
        assert np.abs(rpy[:, 0]).max() > 3.0 and np.abs(rpy[:, 2]).max() > 3.0 and np.abs(rpy[:, 1]).max() > 1.4
        assert len(set(np.rint(rpy[:, 0] * 2 / np.pi).astype(int))) == 5 and len(set(np.rint(rpy[:, 2] * 2 / np.pi).astype(int))) == 5
    n = len(c["dt"])
    assert n == int(c["n_hover"]) + 64 and (c["counter_in"] == 0).sum() >= 8      # (calls that re-seed Xm are among them)
    worst = {}
    for i in range(n):
        k = MracF64(d)
        k.Kx, k.Kr, k.Xm = c["Kx_in"][i].copy(), c["Kr_in"][i].copy(), c["Xm_in"][i].reshape(12, 1).copy()
        k.control_counter = int(c["counter_in"][i])
        rpm, pos_e, rpy_e = k.computeControl(float(c["dt"][i]), c["cur_pos"][i], c["cur_quat"][i], c["cur_vel"][i], c["cur_ang_vel"][i],
                                             c["target_pos"][i], c["target_rpy"][i], c["target_vel"][i], c["target_rpy_rates"][i])
        for name, got, want in (("rpm", rpm, c["rpm"][i]), ("pos_e", pos_e, c["pos_e"][i]), ("rpy_e", rpy_e, c["rpy_e"][i]),
                                ("Kx", k.Kx, c["Kx_out"][i]), ("Kr", k.Kr, c["Kr_out"][i]), ("Xm", k.Xm.reshape(12), c["Xm_out"][i])):
            worst[name] = max(worst.get(name, 0.0), rel_err(got, want))
    print(model, worst)
    assert max(worst.values()) < F64_BOUND, worst


@pytest.mark.parametrize("run", ["mrac_hover_cf2x", "mrac_hover_cf2p", "mrac_hover_cf2x_mass120"])
def test_restatement_reproduces_the_recorded_closed_loops(run):
    """The restated controller along the reference's trajectory: fed the recorded state of every step, it returns the recorded RPMs
    and carries the recorded Kx, Kr, Xm -- 720 steps, adaptation included."""
    h, d = golden(run), golden("mrac_design_" + run.split("_")[2])
    k, worst = MracF64(d), {}
    assert h["rpm"].shape == (720, 4) and np.linalg.norm(h["state20"][-1, 0:3] - h["target"]) < 0.02      # (the reference flies it)
    for i in range(720):
        s = h["state20"][i]
        rpm, _, _ = k.computeControl(1.0 / float(h["ctrl_freq"]), s[0:3], s[3:7], s[10:13], s[13:16], h["target"])
        for name, got, want in (("rpm", rpm, h["rpm"][i]), ("Kx", k.Kx, h["Kx"][i]), ("Kr", k.Kr, h["Kr"][i]), ("Xm", k.Xm.reshape(12), h["Xm"][i])):
            worst[name] = max(worst.get(name, 0.0), rel_err(got, want))
    print(run, worst)
    assert max(worst.values()) < F64_BOUND, worst


# ---- 2. the product's design ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_design_equals_the_reference_and_satisfies_its_equations(model):
    M = importlib.import_module("gym_pybullet_drones_amd.control.MRAC")
    from gym_pybullet_drones_amd.params import DroneParams
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    P = DroneParams(DroneModel(model))
    ref = golden(f"mrac_design_{model}")
    d = M.design(P.M, P.J[0, 0], P.J[1, 1], P.J[2, 2])
    again = M.design(P.M, P.J[0, 0], P.J[1, 1], P.J[2, 2])
    for k in ("A", "B", "K", "Am", "Bm", "P", "Kr_ref_gain", "Kx0"):
        assert np.array_equal(d[k], again[k]), k                     # deterministic: two constructions, identical bits
        assert rel_err(d[k], ref[k]) < 1e-9, (k, rel_err(d[k], ref[k]))   # (the same scipy calls: equal to rounding of the solver's route)
    assert np.array_equal(d["Kr0"], np.eye(4)) and np.array_equal(d["Kx0"], -d["K"].T)
    # ... and independently of the fixture: the poles are -1 .. -12 and P solves the Lyapunov equation
    eig = np.sort(np.linalg.eigvals(d["Am"]).real)
    assert np.allclose(eig, -np.arange(12, 0, -1), rtol=0, atol=1e-6), eig
    assert np.abs(np.linalg.eigvals(d["Am"]).imag).max() < 1e-6
    res = d["Am"].T @ d["P"] + d["P"] @ d["Am"] + 600 * np.eye(12)
    assert np.abs(res).max() < 1e-7 * np.abs(d["P"]).max(), np.abs(res).max()
    # the compact form of the struct loses nothing: rebuilt from its fields, Am and Bm are the float32 roundings of the design's
    s = M.to_struct(d, 5e-3, 5e-3, M.mixer_matrix(DroneModel(model)), P.KF)
    Am = np.zeros((12, 12))
    Am[:6, 6:] = np.eye(6)
    Am[6:8, 3:5] = np.array(list(s.A_grav)).reshape(2, 2)
    Am[8:] = np.array(list(s.Am_lo)).reshape(4, 12)
    Bm = np.zeros((12, 4))
    Bm[8:] = np.diag(list(s.B_diag))
    assert np.array_equal(Am, d["Am"].astype(np.float32).astype(np.float64)) and np.array_equal(Bm, d["Bm"].astype(np.float32).astype(np.float64))
    assert np.array_equal(np.array(list(s.PB)).reshape(12, 4), (d["P"] @ d["Bm"]).astype(np.float32).astype(np.float64))
    bad = dict(d, Am=d["Am"] + np.eye(12))
    with pytest.raises(ValueError):
        M.to_struct(bad, 5e-3, 5e-3, M.mixer_matrix(DroneModel(model)), P.KF)


def test_constructor_check_and_gamma_setter_need_no_device():
    M = importlib.import_module("gym_pybullet_drones_amd.control.MRAC")
    assert M._scalar_of_identity(np.eye(12) * 0.01, 12, "Gamma_x") == 0.01 and M._scalar_of_identity(0.0, 4, "Gamma_r") == 0.0
    for wrong in (np.diag(np.arange(1.0, 13.0)), np.ones((12, 12)), np.eye(4)):
        with pytest.raises(ValueError):
            M._scalar_of_identity(wrong, 12, "Gamma_x")


# ---- 3. argument errors are found before the first HIP call ---------------------------------------------------------------------
def _entries():
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.params import DroneParams
    L = _native.lib()
    size = ctypes.c_int32(0)
    assert L.gpd_sizeof_mrac(ctypes.byref(size)) == 0 and size.value == ctypes.sizeof(_native.GpdMrac) == 4 * (176 + 64)
    assert L.gpd_sizeof_mrac(None) == _native.GPD_EINVAL and L.gpd_abi_version() == 9
    return _native, L, DroneParams().to_struct()


def _expect(L, rc, code, text):
    msg = L.gpd_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_gpd_mrac_and_reset_reject_bad_arguments_without_a_device():
    _native, L, _ = _entries()
    m = _native.GpdMrac()
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    odd = ctypes.c_void_p(0x1004)

    def call(mrac=ctypes.byref(m), state=p, counter=p, ld=64, dt=1 / 120, pos=p, quat=p, vel=p, angv=p, tpos=p, rpm=p, n=64):
        return L.gpd_mrac(mrac, state, counter, ld, dt, pos, quat, vel, angv, tpos, None, None, None, rpm, None, None, n, None)
    for kw in (dict(mrac=None), dict(state=None), dict(counter=None), dict(pos=None), dict(quat=None), dict(vel=None), dict(angv=None),
               dict(tpos=None), dict(rpm=None)):
        _expect(L, call(**kw), _native.GPD_EINVAL, "gpd_mrac: NULL")
    _expect(L, call(n=0), _native.GPD_EINVAL, "gpd_mrac: need 0 < n <= ld")
    _expect(L, call(n=65), _native.GPD_EINVAL, "gpd_mrac: need 0 < n <= ld")
    _expect(L, call(n=(1 << 26) + 1, ld=1 << 27), _native.GPD_ERANGE, "gpd_mrac: more than 2^26")
    _expect(L, call(dt=0.0), _native.GPD_EINVAL, "ctrl_dt must be positive")
    _expect(L, call(quat=odd), _native.GPD_EINVAL, "16-byte aligned")
    _expect(L, call(rpm=odd), _native.GPD_EINVAL, "16-byte aligned")
    _expect(L, L.gpd_mrac_reset(None, p, 64, ctypes.byref(m), None, 64, 0, None), _native.GPD_EINVAL, "gpd_mrac_reset: NULL")
    _expect(L, L.gpd_mrac_reset(p, None, 64, ctypes.byref(m), None, 64, 0, None), _native.GPD_EINVAL, "gpd_mrac_reset: NULL")
    _expect(L, L.gpd_mrac_reset(p, p, 64, None, None, 64, 1, None), _native.GPD_EINVAL, "restore_gains needs the design")
    _expect(L, L.gpd_mrac_reset(p, p, 63, ctypes.byref(m), None, 64, 0, None), _native.GPD_EINVAL, "need 0 < n <= ld")
    _expect(L, L.gpd_mrac_reset(p, p, 64, ctypes.byref(m), None, -1, 0, None), _native.GPD_EINVAL, "need 0 < n <= ld")


def test_gpd_rollout_mrac_rejects_bad_arguments_without_a_device():
    _native, L, params = _entries()
    m = _native.GpdMrac()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)

    def call(state_kw=None, cfg_kw=None, mrac=ctypes.byref(m), mst=p, counter=p, mld=128, targets=p, ts=0, rpm=p, plant=None, obs=p, os_=0, K=4):
        st = _native.GpdState(kin=0x1000, last_rpm=0x1000, step_counter=0x1000, ld=128)
        for k, v in (state_kw or {}).items():
            setattr(st, k, v)
        cfg = _native.GpdStepCfg(num_envs=100, drones_per_env=1, act_type=5, substeps=2, physics_flags=0, pyb_dt=1 / 240, ctrl_dt=1 / 120,
                                 inv_ctrl_dt=120.0, task=0)
        for k, v in (cfg_kw or {}).items():
            setattr(cfg, k, v)
        return L.gpd_rollout_mrac(ctypes.byref(params), mrac, ctypes.byref(st), ctypes.byref(cfg), mst, counter, mld, targets, ts, rpm,
                                  plant, obs, os_, K, None)
    E, R, U = _native.GPD_EINVAL, _native.GPD_ERANGE, _native.GPD_ENOTSUP
    _expect(L, L.gpd_rollout_mrac(None, None, None, None, None, None, 0, None, 0, None, None, None, 0, 0, None), E, "gpd_rollout_mrac: NULL")
    _expect(L, call(mrac=None), E, "NULL params/mrac/state/cfg")
    _expect(L, call(state_kw=dict(kin=None)), E, "NULL state.kin")
    for kw in (dict(mst=None), dict(counter=None), dict(targets=None), dict(rpm=None), dict(obs=None)):
        _expect(L, call(**kw), E, "NULL mrac_state/counter/targets/rpm_carry/obs12")
    _expect(L, call(state_kw=dict(kin=0x1004)), E, "16-byte aligned")
    _expect(L, call(K=0), E, "num_steps must be positive")
    _expect(L, call(cfg_kw=dict(num_envs=0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(substeps=0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(physics_flags=32)), E, "unknown physics flag")
    _expect(L, call(cfg_kw=dict(drones_per_env=2)), U, "aviaries of one drone")
    _expect(L, call(cfg_kw=dict(task=1)), U, "GPD_TASK_NONE")
    _expect(L, call(cfg_kw=dict(auto_reset=1)), U, "GPD_TASK_NONE")
    _expect(L, call(cfg_kw=dict(act_type=1)), U, "act_type")
    _expect(L, call(cfg_kw=dict(physics_flags=4)), U, "downwash")
    _expect(L, call(state_kw=dict(dw_force=0x1000)), U, "downwash")
    _expect(L, call(state_kw=dict(ld=99)), E, "state.ld / mrac_ld < num_envs")
    _expect(L, call(mld=99), E, "state.ld / mrac_ld < num_envs")
    _expect(L, call(cfg_kw=dict(num_envs=(1 << 26) + 1), state_kw=dict(ld=1 << 27), mld=1 << 27), R, "2^26")
    _expect(L, call(cfg_kw=dict(physics_flags=2), state_kw=dict(last_rpm=None)), E, "GPD_PHYS_DRAG needs state.last_rpm")
    _expect(L, call(ts=-1), E, "non-negative")
    _expect(L, call(os_=100), E, "at least 12*num_envs")
    _expect(L, call(ts=1202), E, "multiples of 4")
    for kw in (dict(targets=odd), dict(rpm=odd), dict(obs=odd), dict(plant=odd)):
        _expect(L, call(**kw), E, "16-byte aligned")
    _expect(L, call(cfg_kw=dict(ctrl_dt=0.0)), E, "must be positive")


# ---- 4. the ISA fences of tests/test_kernel_isa.py, on the fifth unit ------------------------------------------------------------
@pytest.fixture(scope="module")
def mrac_asm():
    from gym_pybullet_drones_amd import _native
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    assert _native.UNITS[4][0] == "mrac.hip" and len(_native.UNITS) == 5
    import tempfile
    flags = [f for f in _native.COMMON_FLAGS if f != "-fPIC"] + _native.UNITS[4][1]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "mrac.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(REPO, "include"),
                                          os.path.join(_native.CSRC, "mrac.hip"), "-o", out], check=True, capture_output=True)
        return open(out).read()


def test_mrac_unit_needs_no_scratch_reads_no_dispatch_packet_and_tears_no_argument_tuple(mrac_asm):
    import isa_spill_check as chk
    scratch = re.findall(r"; ScratchSize: (\d+)", mrac_asm)
    assert len(scratch) == 7 and all(v == "0" for v in scratch), scratch        # gpd_mrac, reset, restore, four rollout variants
    assert ".amdhsa_user_sgpr_dispatch_ptr 1" not in mrac_asm
    assert not re.search(r"^\s*scratch_(load|store)", mrac_asm, flags=re.M)
    names = []
    for name, body in chk.kernels(mrac_asm):
        names.append(name)
        found = chk.torn_spills(body)
        assert not found, (name, [(l, dead, run["lanes"]) for _, l, dead, run in found])
        meta = mrac_asm[mrac_asm.index(name + ":"):]
        vgprs, agprs = (int(re.search(rf"; Num{k}gprs: (\d+)", meta).group(1)) for k in ("V", "A"))
        print(name, "VGPRs", vgprs, "AGPRs", agprs)
        # one wave per SIMD: 256 VGPRs + 256 AGPRs.  The largest variant, <EXT, PLANT>, needs 217 AGPRs today; the ceiling leaves 24
        # registers before scratch memory, so that a compiler that moves the allocation is announced here first
        assert vgprs <= 256 and agprs <= 232, (name, vgprs, agprs)
        spills = int(re.search(r"\.sgpr_spill_count:\s*(\d+)", meta).group(1))
        print(name, "SGPR spills to VGPR lanes", spills)
        assert spills <= 100, (name, spills)          # (16 .. 86 today: GpdParams / GpdStepCfg words next to the loop's addresses)
        ops = [l.split()[0] for l in body if l.strip() and not l.strip().startswith((";", ".")) and not l.strip().endswith(":")]
        if "reset" not in name and "restore" not in name:
            # the design's constants come from LDS as 16-byte broadcasts: 44 rows per call; the rollout reads the 12 rows of
            # Kr_ref_gain once per target row (before the loop, and in the branch of a per-step target) and the other 32 per step
            want = 56 if "rollout" in name else 44
            assert ops.count("ds_read_b128") == want and not [o for o in ops if o.startswith("v_mfma")], ops.count("ds_read_b128")
    assert sum("gpd_rollout_mrac_kernel" in n for n in names) == 4 and any("gpd_mrac_kernel" in n for n in names)


# ---- 5. scipy stays optional --------------------------------------------------------------------------------------------------
def test_package_and_dslpid_import_without_scipy():
    code = ("import sys\n"
            "sys.modules['scipy'] = None\n"
            "import gym_pybullet_drones_amd\n"
            "from gym_pybullet_drones_amd.control import DSLPIDControl, DSLPIDControlBatch, MRAC, VectorMRAC\n"
            "from gym_pybullet_drones_amd.envs import CtrlAviary, VectorCtrlAviary\n"
            "import importlib; module = importlib.import_module('gym_pybullet_drones_amd.control.MRAC')\n"
            "assert not [m for m in sys.modules if m.startswith('scipy.')], 'scipy was imported'\n"
            "try:\n"
            "    module.design(0.027, 1.4e-5, 1.4e-5, 2.17e-5)\n"
            "except ImportError:\n"
            "    print('design needs scipy: ok')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO))
    assert res.returncode == 0 and "design needs scipy: ok" in res.stdout, res.stdout + res.stderr

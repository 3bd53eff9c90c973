"""Thrust and body-rate commands, the parts that need no GPU: the drop-in class and the float64 yardstick against the reference's
recorded calls, csrc/ctbr_math.inc compiled into a stand-alone C program (fp32, under ASan + UBSan) against both, the rotor
allocation as an exact inverse, the float64 closed loop, and the argument checks of the three entries and of the Python layer.
Fixture: tests/golden/make_golden_ctbr.py (the reference's unmodified `control/CTBRControl.py`)."""
import ctypes
import os
import struct
import sys
import types

import numpy as np
import pytest

from conftest import REPO, golden

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import ctbr_f64 as H  # noqa: E402
import host_lib  # noqa: E402

#: the same arithmetic in float64, only the matrix -> quaternion route differs (the reference: an eigenvector; the class: Shepperd; the
#: yardstick: none, it works on the rotation matrices)
F64_BOUND = 1e-9
#: fp32 against float64: the project's tolerance (tests/test_gpu_mrac.py), norm-relative
TOL = 1e-4
MODELS = ("cf2x", "cf2p", "racer")


def _model(name):
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    return DroneModel(name)


# ---- 1. float64: the drop-in class and the yardstick are the reference ------------------------------------------------------------
def test_fixture_is_what_the_generator_promises():
    c = golden("ctbr_calls")
    assert c["cmd"].shape == (256, 4) and c["via_state"].sum() == 128
    assert c["angle"][:128].max() <= 0.5 and c["angle"][128:].max() > 2.9 and np.abs(c["q_err_w"]).min() >= 1e-3
    assert (c["q_err_w"] < 0).any() and (c["q_err_w"] > 0).any()            # (both signs: the final negation is exercised)
    assert np.abs(c["target_rpy"]).min() > 0 and (c["target_vel"] == 0).all(axis=1).sum() == 128


def test_dropin_class_reproduces_the_recorded_calls():
    from gym_pybullet_drones_amd.control import CTBRControl
    c = golden("ctbr_calls")
    k = CTBRControl(_model("cf2x"))
    got = []
    for i in range(256):
        q = c["cur_quat"][i]
        if c["via_state"][i]:
            state = np.concatenate([c["cur_pos"][i], q, np.zeros(3), c["cur_vel"][i], c["cur_ang_vel"][i], np.zeros(4)])
            out = k.computeControlFromState(control_timestep=1 / 48, state=state, target_pos=c["target_pos"][i], target_rpy=c["target_rpy"][i],
                                            target_vel=c["target_vel"][i], target_rpy_rates=c["target_rpy_rates"][i])
        else:      # (the method's own convention: w, x, y, z)
            out = k.computeControl(1 / 48, c["cur_pos"][i], np.array([q[3], q[0], q[1], q[2]]), c["cur_vel"][i], c["cur_ang_vel"][i],
                                   c["target_pos"][i], c["target_rpy"][i], c["target_vel"][i], c["target_rpy_rates"][i])
        assert isinstance(out, tuple) and len(out) == 4
        got.append(out)
    err = {name: H.rel_err(np.array(got)[:, cols], c["cmd"][:, cols]) for name, cols in (("thrust", [0]), ("rates", [1, 2, 3]))}
    print(err)
    assert max(err.values()) < F64_BOUND, err
    # the defaults are the reference's: no target velocity = zeros
    i = int(np.flatnonzero((c["target_vel"] == 0).all(axis=1) & ~c["via_state"])[0])
    q = c["cur_quat"][i]
    out = k.computeControl(1 / 48, c["cur_pos"][i], np.array([q[3], q[0], q[1], q[2]]), c["cur_vel"][i], c["cur_ang_vel"][i], c["target_pos"][i])
    assert H.rel_err(out, c["cmd"][i]) < F64_BOUND


def test_dropin_class_keeps_the_reference_surface():
    from gym_pybullet_drones_amd.control import CTBRControl
    k = CTBRControl(_model("cf2p"), g=9.8)
    assert k.control_counter == 0 and k.KF > 0 and k.KM > 0 and abs(k.GRAVITY - 9.8 * k._getURDFParameter("m")) < 1e-15
    k.control_counter = 5
    k.reset()
    assert k.control_counter == 0
    with pytest.raises(AttributeError):            # (no PID coefficients to set: BaseControl's refusal)
        k.setPIDCoefficients(p_coeff_pos=np.ones(3))
    with pytest.raises(AssertionError):            # (the reference asserts its operands' shapes)
        k.computeControl(1 / 48, np.zeros(4), np.array([1.0, 0, 0, 0]), np.zeros(3), np.zeros(3), np.zeros(3))


def test_yardstick_reproduces_the_recorded_calls():
    c = golden("ctbr_calls")
    got = H.outer(c["cur_pos"], c["cur_quat"], c["cur_vel"], c["target_pos"], c["target_vel"])
    err = {name: H.rel_err(got[:, cols], c["cmd"][:, cols]) for name, cols in (("thrust", [0]), ("rates", [1, 2, 3]))}
    print(err)
    assert max(err.values()) < F64_BOUND, err


# ---- 2. the allocation is an exact inverse; the closed loop converges ---------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_allocation_inverts_the_integrators_torque_rows(model):
    from gym_pybullet_drones_amd.control.CTBRControl import allocation, to_struct
    from gym_pybullet_drones_amd.params import DroneParams
    P = DroneParams(_model(model))
    C = H.UrdfConstants(H.URDF[model], model)
    rows, alloc = H.torque_rows(C), allocation(P)
    rng = np.random.default_rng(4)
    for _ in range(32):
        T, tau = rng.uniform(0.0, 0.6), rng.normal(0.0, 1e-3, 3)
        f = T / 4 + alloc @ tau
        back = rows @ f
        assert abs(back[0] - T) < 1e-12 and np.abs(back[1:] - tau).max() < 1e-12, (model, back, T, tau)
    s = to_struct(P)
    assert np.array_equal(np.array(list(s.alloc)), alloc.reshape(-1).astype(np.float32).astype(np.float64))
    assert ctypes.sizeof(s) == 128 and s.g == np.float32(9.8) and list(s.k_rate) == [40.0, 40.0, 20.0] and s.thrust_max == np.float32(40.9)
    assert s.rate_max == np.float32(2 * np.pi) and s.f_max == np.float32(P.KF * P.MAX_RPM ** 2) and s.inv_kf == np.float32(1 / P.KF)
    for bad in (dict(k_rate=(40.0, 40.0)), dict(k_rate=(40.0, -1.0, 20.0)), dict(k_rate=(np.nan, 1.0, 1.0)), dict(thrust_max=0.0), dict(rate_max=np.inf)):
        with pytest.raises(ValueError):
            to_struct(P, **bad)


@pytest.mark.parametrize("ctrl_freq", [48, 30])
def test_float64_closed_loop_reaches_the_target(ctrl_freq):
    """outer loop at `ctrl_freq` over the rate loop at 240 Hz, CF2X, (0, 0, 0.5) -> (0.3, -0.2, 1.0): within 1e-3 m after 6 s (measured
    4.1e-5 m at 48 Hz, 3.8e-5 m at 30 Hz), no rotor ever clipped"""
    sim = H.CtbrF64("cf2x", 1, pos=[[0.0, 0.0, 0.5]], ctrl_freq=ctrl_freq)
    obs = sim.run(np.array([[0.3, -0.2, 1.0]]), 6 * ctrl_freq, "pos")
    err = float(np.linalg.norm(obs[-1, 0, 0:3] - [0.3, -0.2, 1.0]))
    print(ctrl_freq, "Hz:", err, "m; steps with a clipped rotor:", sim.clipped_steps)
    assert err < 1e-3 and sim.clipped_steps[0] == 0


def test_steady_state_error_of_a_heavier_drone_is_the_predicted_one():
    sim = H.CtbrF64("cf2x", 2, pos=[[0.0, 0.0, 0.5]] * 2, ctrl_freq=48, mass_scale=[1.2, 0.9])
    obs = sim.run(np.array([[0.3, -0.2, 1.0]] * 2), 6 * 48, "pos")
    err = np.linalg.norm(obs[-1, :, 0:3] - [0.3, -0.2, 1.0], axis=1)
    want = H.steady_state_error([1.2, 0.9])
    print(err, want)
    assert abs(want[0] - 0.245) < 1e-12 and np.abs(err - want).max() < 1e-4


# ---- 3. ctbr_math.inc in fp32, and the host side of the entries, under the sanitizers ---------------------------------------------
@pytest.fixture(scope="module")
def ctbr_host():
    from gym_pybullet_drones_amd import _native
    return host_lib.program("ctbr_host", include=(_native.CSRC,))


def _clean(run):
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]


def test_host_side_of_the_entries_under_asan_and_ubsan(ctbr_host):
    run = host_lib.run(ctbr_host)
    print(run.stdout[-3000:])
    _clean(run)
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") == 68          # (every check of the program ran)


def _run_math(exe, what, tmp_path, head: bytes, rows: np.ndarray) -> np.ndarray:
    src, dst = os.path.join(str(tmp_path), what + ".in"), os.path.join(str(tmp_path), what + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(rows)) + head + np.ascontiguousarray(rows, dtype=np.float32).tobytes())
    run = host_lib.run(exe, what, src, dst)
    _clean(run)
    assert run.returncode == 0, run.stdout + run.stderr
    return np.fromfile(dst, dtype=np.float32).reshape(len(rows), 4).astype(np.float64)


def test_outer_loop_in_fp32_against_the_recorded_calls(ctbr_host, tmp_path):
    from gym_pybullet_drones_amd.control.CTBRControl import to_struct
    from gym_pybullet_drones_amd.params import DroneParams
    c = golden("ctbr_calls")
    rows = np.hstack([c["cur_pos"], c["cur_quat"], c["cur_vel"], c["target_pos"], c["target_vel"]])
    got = _run_math(ctbr_host, "outer", tmp_path, bytes(to_struct(DroneParams(_model("cf2x")))), rows)
    err = {name: H.rel_err(got[:, cols], c["cmd"][:, cols]) for name, cols in (("thrust", [0]), ("rates", [1, 2, 3]))}
    print(err)
    assert max(err.values()) < TOL, err


@pytest.mark.parametrize("model", MODELS)
def test_rate_loop_in_fp32_against_the_yardstick(ctbr_host, tmp_path, model):
    """4 096 seeded (command, body rates) pairs: thrust commands from below 0 to beyond thrust_max, rate commands beyond +-rate_max,
    rate errors large enough to drive rotors to 0 and to f_max"""
    from gym_pybullet_drones_amd.control.CTBRControl import to_struct
    from gym_pybullet_drones_amd.params import DroneParams
    P, C = DroneParams(_model(model)), H.UrdfConstants(H.URDF[model], model)
    rng = np.random.default_rng(17)
    n = 4096
    cmd = np.hstack([rng.uniform(-5.0, 60.0, (n, 1)), rng.normal(0.0, 4.0, (n, 3))])
    cmd[::16, 1:] *= 10.0
    w = rng.normal(0.0, 3.0, (n, 3))
    assert (cmd[:, 0] < 0).any() and (cmd[:, 0] > H.THRUST_MAX).any() and (np.abs(cmd[:, 1:]) > H.RATE_MAX).any()
    want = H.rate_loop(C, cmd, w)
    at_max = np.isclose(want, C.MAX_RPM, rtol=1e-12, atol=0)
    assert (want == 0).any() and at_max.any() and ((want > 0) & ~at_max).any()
    head = bytes(to_struct(P)) + np.array([P.M, P.J[0, 0], P.J[1, 1], P.J[2, 2]], dtype=np.float32).tobytes()
    got = _run_math(ctbr_host, "rate", tmp_path, head, np.hstack([cmd, w]))
    err = H.rel_err(got, want)
    print(model, "rpm", err, "rotors at 0:", int((want == 0).sum()), "at f_max:", int(at_max.sum()))
    assert err < TOL


# ---- 4. refusals through ctypes, one broken argument at a time -------------------------------------------------------------------
def _entries():
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.params import DroneParams
    L = _native.lib()
    size = ctypes.c_int32(0)
    assert L.gpd_sizeof_ctbr(ctypes.byref(size)) == 0 and size.value == ctypes.sizeof(_native.GpdCtbr) == 128
    assert L.gpd_sizeof_ctbr(None) == _native.GPD_EINVAL and L.gpd_last_error().decode().startswith("gpd_sizeof_ctbr: ")
    return _native, L, DroneParams().to_struct()


def _expect(L, rc, code, text):
    msg = L.gpd_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_entries_are_bound_and_the_new_sources_are_tracked():
    _native, L, _ = _entries()
    assert L.gpd_abi_version() == 9 == _native.ABI_VERSION and len(_native.UNITS) == 5
    for name in ("gpd_sizeof_ctbr", "gpd_ctbr", "gpd_rollout_ctbr"):
        assert name in _native.exported_symbols() and getattr(L, name).argtypes is not None
    for inc in ("ctbr_math.inc", "ctbr.inc"):
        assert inc in _native.HEADERS and os.path.exists(os.path.join(_native.CSRC, inc))
    assert _native.CTBR_MODES == {"cmd": 0, "pos": 1}
    hdr = open(os.path.join(REPO, "include", "gpd.h")).read()
    assert "#define GPD_CTBR_CMD 0" in hdr and "#define GPD_CTBR_POS 1" in hdr


def test_gpd_ctbr_rejects_bad_arguments_without_a_device():
    _native, L, _ = _entries()
    b = _native.GpdCtbr()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)      # never dereferenced: every call below fails its checks first

    def call(ctbr=ctypes.byref(b), pos=p, quat=p, vel=p, tpos=p, tvel=None, cmd=p, n=64):
        return L.gpd_ctbr(ctbr, pos, quat, vel, tpos, tvel, cmd, n, None)
    for kw in (dict(ctbr=None), dict(pos=None), dict(quat=None), dict(vel=None), dict(tpos=None), dict(cmd=None)):
        _expect(L, call(**kw), _native.GPD_EINVAL, "gpd_ctbr: NULL")
    _expect(L, call(n=0), _native.GPD_EINVAL, "gpd_ctbr: n must be positive")
    _expect(L, call(n=-1), _native.GPD_EINVAL, "gpd_ctbr: n must be positive")
    _expect(L, call(n=(1 << 26) + 1), _native.GPD_ERANGE, "gpd_ctbr: more than 2^26")
    _expect(L, call(quat=odd), _native.GPD_EINVAL, "gpd_ctbr: cur_quat and cmd must be 16-byte aligned")
    _expect(L, call(cmd=odd), _native.GPD_EINVAL, "gpd_ctbr: cur_quat and cmd must be 16-byte aligned")


def test_gpd_rollout_ctbr_rejects_bad_arguments_without_a_device():
    _native, L, params = _entries()
    b = _native.GpdCtbr()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)

    def call(state_kw=None, cfg_kw=None, ctbr=ctypes.byref(b), mode=0, rows=p, rs=0, plant=None, obs=p, os_=0, cmd=None, K=4):
        st = _native.GpdState(kin=0x1000, last_rpm=0x1000, step_counter=0x1000, ld=128)
        for k, v in (state_kw or {}).items():
            setattr(st, k, v)
        cfg = _native.GpdStepCfg(num_envs=100, drones_per_env=1, act_type=5, substeps=5, physics_flags=0, pyb_dt=1 / 240, ctrl_dt=1 / 48,
                                 inv_ctrl_dt=48.0, task=0)
        for k, v in (cfg_kw or {}).items():
            setattr(cfg, k, v)
        return L.gpd_rollout_ctbr(ctypes.byref(params), ctbr, ctypes.byref(st), ctypes.byref(cfg), mode, rows, rs, plant, obs, os_, cmd, K, None)
    E, R, U = _native.GPD_EINVAL, _native.GPD_ERANGE, _native.GPD_ENOTSUP
    _expect(L, L.gpd_rollout_ctbr(None, None, None, None, 0, None, 0, None, None, 0, None, 0, None), E, "gpd_rollout_ctbr: NULL")
    _expect(L, call(ctbr=None), E, "gpd_rollout_ctbr: NULL params/ctbr/state/cfg")
    _expect(L, call(state_kw=dict(kin=None)), E, "gpd_rollout_ctbr: NULL state.kin")
    _expect(L, call(rows=None), E, "gpd_rollout_ctbr: NULL rows/obs12")
    _expect(L, call(obs=None), E, "gpd_rollout_ctbr: NULL rows/obs12")
    _expect(L, call(state_kw=dict(kin=0x1004)), E, "16-byte aligned")
    _expect(L, call(mode=2), E, "gpd_rollout_ctbr: unknown mode")
    _expect(L, call(K=0), E, "num_steps must be positive")
    _expect(L, call(rs=-4), E, "non-negative")
    _expect(L, call(cfg_kw=dict(num_envs=0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(substeps=0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(physics_flags=32)), E, "unknown physics flag")
    _expect(L, call(cfg_kw=dict(drones_per_env=2)), U, "gpd_rollout_ctbr: aviaries of one drone")
    _expect(L, call(cfg_kw=dict(task=1)), U, "GPD_TASK_NONE")
    _expect(L, call(cfg_kw=dict(auto_reset=1)), U, "GPD_TASK_NONE")
    for act in (0, 1, 2, 3, 4):
        _expect(L, call(cfg_kw=dict(act_type=act)), U, "act_type")
    _expect(L, call(cfg_kw=dict(physics_flags=4)), U, "downwash")
    _expect(L, call(state_kw=dict(dw_force=0x1000)), U, "downwash")
    _expect(L, call(state_kw=dict(ld=99)), E, "state.ld")
    _expect(L, call(cfg_kw=dict(num_envs=(1 << 26) + 1), state_kw=dict(ld=1 << 27)), R, "2^26")
    _expect(L, call(cfg_kw=dict(physics_flags=2), state_kw=dict(last_rpm=None)), E, "GPD_PHYS_DRAG needs state.last_rpm")
    _expect(L, call(rs=396), E, "step stride")                 # CMD: 4 * 100 floats per step
    _expect(L, call(mode=1, rs=400), E, "step stride")         # POS: 12 * 100
    _expect(L, call(os_=400), E, "step stride")
    _expect(L, call(rs=402), E, "multiples of 4")
    _expect(L, call(os_=1201), E, "multiples of 4")
    for kw in (dict(rows=odd), dict(obs=odd), dict(plant=odd), dict(cmd=odd)):
        _expect(L, call(**kw), E, "16-byte aligned")
    _expect(L, call(cmd=p), E, "must not alias")
    _expect(L, call(cfg_kw=dict(ctrl_dt=0.0)), E, "must be positive")
    _expect(L, call(cfg_kw=dict(pyb_dt=0.0)), E, "must be positive")


# ---- 5. the Python layer refuses the same shapes before any device work ----------------------------------------------------------
def test_vector_ctbr_and_rollout_ctbr_refuse_before_any_device_work():
    import torch
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.control import VectorCTBR
    cpu = torch.device("cpu")
    for bad in (dict(num=0), dict(num=4, drone_model=None), dict(num=4, k_rate=(1.0, 2.0)), dict(num=4, thrust_max=-1.0), dict(num=4, rate_max=0.0)):
        with pytest.raises(ValueError):
            VectorCTBR(**{"device": cpu, **bad})
    ctrl = VectorCTBR(4, _model("cf2x"), device=cpu, k_rate=(30.0, 30.0, 10.0))
    assert ctrl.struct().k_rate[2] == 10.0 and ctrl.n == 4 and ctrl.control_counter == 0
    z3, z4 = np.zeros((4, 3)), np.zeros((4, 4))
    for bad in (dict(pos=np.zeros((3, 3))), dict(quat=z3), dict(vel=z4), dict(target_pos=np.zeros(3)), dict(target_vel=z4)):
        with pytest.raises(ValueError):
            ctrl.compute(**{"pos": z3, "quat": z4, "vel": z3, "target_pos": z3, **bad})

    def core(**kw):         # what rollout_ctbr reads of a SimCore before its launch
        return types.SimpleNamespace(**{"N": 4, "device": cpu, "host_visible": False, "act_ring": None, **kw})
    roll = engine.SimCore.rollout_ctbr
    cmd = torch.zeros((4, 4))
    for who, args, kw in ((core(), (ctrl, cmd, 0), {}), (core(), (ctrl, cmd, 3), dict(mode="rates")), (core(host_visible=True), (ctrl, cmd, 3), {}),
                          (core(act_ring=cmd), (ctrl, cmd, 3), {}), (core(N=5), (ctrl, torch.zeros((5, 4)), 3), {}),
                          (core(), (object(), cmd, 3), {}), (core(), (ctrl, torch.zeros((4, 12)), 3), {}),
                          (core(), (ctrl, torch.zeros((2, 4, 4)), 3), {}), (core(), (ctrl, cmd, 3), dict(mode="pos")),
                          (core(), (ctrl, torch.zeros((3, 4, 5)), 3), dict(mode="pos"))):
        with pytest.raises((ValueError, AttributeError)) as e:
            roll(who, *args, **kw)
        assert e.type is ValueError, (args[1:], kw, e.value)

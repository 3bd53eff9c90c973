"""The differentiable rollout through the DSLPID loop without a GPU: the float64 yardstick (tests/helpers/diff_pid_f64.py) held against the
batched oracle and against finite differences, its float32 run against its float64 run on the GPU tests' inputs (the size sweep's
included), those inputs' distance to every select threshold (the drones of the far case: beyond the reward clamp at every step), csrc/dslpid_vjp.inc evaluated on the host against float64 autograd of the restatement's controller, and the
host side of the three entries (include/gpd.h `gpd_rollout_tape_pid_floats` / `gpd_rollout_tape_pid` / `gpd_rollout_vjp_pid`):
tests/c/diff_pid_host.c under AddressSanitizer + UBSan against the launch stub."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, urdf

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import diff_f64 as ref  # noqa: E402
import diff_pid_f64 as pref  # noqa: E402
import host_lib  # noqa: E402
from host_lib import params as _params, step_cfg as _cfg  # noqa: E402

T = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["cf2x", "cf2p"])
@pytest.mark.parametrize("act", ["pid", "vel", "one_d_pid"])
@pytest.mark.parametrize("S", [5, 8])
def test_restatement_forward_is_the_batched_oracle(model, act, S):
    """obs12, reward, the state and the nine members of 4 steps of 5 drones equal oracle.batched_oracle's to 1e-12; for pid the
    waypoints sit on both sides of the 1 m approach limit"""
    from oracle import bullet_math as bm
    from oracle.batched_oracle import BatchedAviary
    n, K = 5, 4
    cfg = ref.config(model, act, S, False, "hover")
    orc = BatchedAviary(urdf(model), model, n, 1, physics_flags=0, pyb_freq=240, ctrl_freq=240 // S, act=act, task="hover")
    inp = pref.make_inputs(orc.C, cfg, n, K, seed=3)
    orc.pos[:, 0], orc.quat[:, 0], orc.vel[:, 0], orc.rpy_rates[:, 0] = inp.pos, inp.quat, inp.vel, inp.rates
    orc.rpy[:, 0] = bm.euler_from_quaternion_b(inp.quat)
    orc.pid.integral_pos_e[:, 0], orc.pid.last_rpy[:, 0], orc.pid.integral_rpy_e[:, 0] = inp.int_pos, inp.last_rpy, inp.int_rpy
    c = ref.consts(orc.C, n)
    pc = pref.pid_consts(orc.pid.GRAVITY, orc.pid.KF, orc.C.SPEED_LIMIT)
    stats = {}
    obs, rew, kin, mem = pref.rollout(c, pc, cfg, tuple(T(v) for v in (inp.pos, inp.quat, inp.vel, inp.rates)),
                                      tuple(T(v) for v in (inp.int_pos, inp.last_rpy, inp.int_rpy)), T(inp.actions), T(inp.target), stats)
    for t in range(K):
        o64, r64, _, _, _ = orc.step(inp.actions[t].reshape(n, 1, -1))
        assert np.abs(obs[t].numpy() - o64[:, 0]).max() < 1e-12, t
        assert np.abs(rew[t].numpy() - r64).max() < 1e-12, t
    for got, want in zip(kin + mem, (orc.pos, orc.quat, orc.vel, orc.rpy_rates, orc.pid.integral_pos_e, orc.pid.last_rpy, orc.pid.integral_rpy_e)):
        assert np.abs(got.numpy() - want[:, 0]).max() < 1e-12
    if act == "pid":
        assert stats["beyond_1m"] > 0 and stats["within_1m"] > 0


GRADCHECK_SEED = {"pid": 5, "vel": 5, "one_d_pid": 5}          # (chosen for the distance the test asserts)


@pytest.mark.parametrize("act,S", [("pid", 2), ("vel", 2), ("one_d_pid", 1)])
def test_restatement_gradients_pass_gradcheck(act, S):
    """float64 autograd of the restatement against finite differences: 2 drones, K = 3, with respect to the actions, the state, the
    members and the gains (in units of their own size).  No drone-step within 2 % of a select threshold (asserted: a finite difference
    across a kink says nothing); a clamp that is engaged, as the torque clamps often are, contributes its zero."""
    C = _params("cf2x")
    cfg = ref.config("cf2x", act, S, False, "hover")
    inp = pref.make_inputs(C, cfg, 2, 3, seed=GRADCHECK_SEED[act])
    if act == "pid":
        inp.actions[:, 0] = inp.pos[0] + np.array([0.1, 0.05, -0.08])         # (one drone within the 1 m limit, one beyond)
        inp.actions[:, 1] = inp.pos[1] + np.array([0.9, 0.7, 0.5])
    c = ref.consts(C, 2)
    unit = T(pref.DEFAULT_GAINS).clamp(min=1.0)                               # (i_tor x, y are zero: their unit is 1)
    stats = {}

    def f(pos, quat, vel, rates, ip, lrpy, ir, a, g, st=None):
        pc = pref.pid_consts_of(C, g * unit)
        obs, rew, kin, mem = pref.rollout(c, pc, cfg, (pos, quat, vel, rates), (ip, lrpy, ir), a, T(inp.target), st)
        return torch.cat([obs.reshape(-1), rew.reshape(-1)] + [k.reshape(-1) for k in kin + mem])

    args = [T(v).clone().requires_grad_(True) for v in (inp.pos, inp.quat, inp.vel, inp.rates, inp.int_pos, inp.last_rpy, inp.int_rpy, inp.actions,
                                                        pref.DEFAULT_GAINS / unit.numpy())]
    f(*args, st=stats)
    assert min(stats["near"].values()) > 0.02, stats["near"]
    if act == "pid":
        assert stats["beyond_1m"] == 3 and stats["within_1m"] == 3
    assert torch.autograd.gradcheck(f, args, eps=1e-7, atol=1e-5, rtol=1e-4)


@pytest.fixture(scope="module")
def case_runs():
    """every GPU case once: the float64 gradients with the forward's statistics, and the float32 run of the same restatement"""
    out = {}
    for name in pref.GPU_CASES:
        cfg, K, kind, seed = pref.case(name)
        C = _params(cfg.model)
        inp = pref.make_inputs(C, cfg, 70, K, seed=seed, kind=kind)
        stats = {}
        g64 = pref.reference_grads(C, cfg, inp, torch.float64, stats=stats)
        g32 = pref.reference_grads(C, cfg, inp, torch.float32)
        out[name] = (cfg, inp, g64, g32, stats)
    return out


@pytest.mark.parametrize("name", list(pref.GPU_CASES))
def test_float32_restatement_follows_the_float64_one_on_the_gpu_inputs(case_runs, name):
    """the rule of tests/test_host_diff.py: max |g32 - g64| / max |g64| per group stays below 1e-5 on the restatement itself, so that a
    device gradient within 1e-4 of the float64 one is a statement about the kernel, not about the inputs' conditioning"""
    cfg, _, g64, g32, _ = case_runs[name]
    err = pref.group_errors(g32, g64)
    print(name, {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) < 1e-5, err
    assert all(np.isfinite(g64[k]).all() for k in pref.GROUPS)
    # every group has a gradient -- but p_for under VEL: the position error of that mapping is identically zero
    dead = {"p_for"} if cfg.act == "vel" else set()
    assert {k for k in pref.GROUPS if not np.abs(g64[k]).max() > 0} == dead


@pytest.mark.parametrize("name", list(pref.GPU_CASES))
def test_gpu_inputs_keep_their_distance_from_every_select_threshold(case_runs, name):
    """no drone-step of any case within 1e-3 (relative) of the integrator clamps +-2, +-0.15, +-1 and +-1500, the +-3200 torque
    clamps, the PWM limits, along = 0, the 1 m approach limit or the gimbal test (nor of the reward clamp and the no-turn test the
    physics has): a float32 run then takes the branches of the float64 one.  The saturated cases hold drone-steps on both sides of
    the clamp they are about, the pid case waypoints on both sides of the limit."""
    cfg, _, _, _, stats = case_runs[name]
    near = dict(stats["near"], gimbal=(ref.GIMBAL - stats["sarg_max"]) / ref.GIMBAL)
    print(name, {k: f"{v:.1e}" for k, v in near.items()})
    want = {"int_pos_2", "int_pos_z_0.15", "int_rpy_1500", "int_rpy_xy_1", "torque_3200", "pwm_limits", "along_0", "gimbal"} | ({"approach_1m"} if cfg.act == "pid" else set())
    assert set(near) == want
    assert min(near.values()) >= 1e-3, near
    assert stats["n2_min"] > 100 * ref.TURN_N2
    lo, hi = stats["lanes"]["reward_arg"]
    if name == "far_vel_k4_s5":
        # every other drone beyond the reward clamp at ALL steps (2 - d^4 below -1e-3 throughout), the others inside it throughout
        far = hi < -1e-3
        assert np.array_equal(far, np.arange(70) % 2 == 0) and (lo[~far] > 1e-3).all() and far.sum() == 35
    else:
        assert stats["reward_arg_min"] > 1e-3
    if name == "sat_int_k10_s5":
        assert stats["int_z_saturated"] >= 70 and stats["int_z_free"] >= 70, stats
    if name == "sat_pwm_k4_s5":
        assert stats["pwm_saturated"] >= 100 and stats["pwm_free"] >= 100, stats
    if name == "pid_k8_s5":
        assert stats["beyond_1m"] >= 70 and stats["within_1m"] >= 70, stats


def test_shared_action_inputs_meet_the_same_two_rules():
    """the GPU suite's shared-action test (one VEL block at every step of 8): its float32 restatement within 1e-5 of the float64 one,
    every drone-step 1e-3 from every threshold"""
    cfg, K, kind, _ = pref.case("vel_k8_s5")
    C = _params(cfg.model)
    inp = pref.make_inputs(C, cfg, 70, K, seed=pref.SHARED_SEED, kind=kind)
    stats = {}
    g64 = pref.reference_grads(C, cfg, inp, torch.float64, shared_action=True, stats=stats)
    err = pref.group_errors(pref.reference_grads(C, cfg, inp, torch.float32, shared_action=True), g64)
    assert g64["actions"].shape == (1, 70, 4) and max(err.values()) < 1e-5, err
    assert min(stats["near"].values()) >= 1e-3 and (ref.GIMBAL - stats["sarg_max"]) / ref.GIMBAL >= 1e-3, stats["near"]


@pytest.mark.parametrize("n", sorted(pref.SIZE_SEEDS))
def test_size_sweep_inputs_meet_the_same_two_rules(n):
    """the GPU suite's size sweep ("vel_k8_s5" at N = 1, 64 and 65 with the seeds of pref.SIZE_SEEDS): float32 restatement within 1e-5
    of the float64 one, every drone-step 1e-3 from every threshold"""
    cfg, K, kind, _ = pref.case("vel_k8_s5")
    C = _params(cfg.model)
    inp = pref.make_inputs(C, cfg, n, K, seed=pref.SIZE_SEEDS[n], kind=kind)
    stats = {}
    g64 = pref.reference_grads(C, cfg, inp, torch.float64, stats=stats)
    err = pref.group_errors(pref.reference_grads(C, cfg, inp, torch.float32), g64)
    assert max(err.values()) < 1e-5, err
    assert min(stats["near"].values()) >= 1e-3 and (ref.GIMBAL - stats["sarg_max"]) / ref.GIMBAL >= 1e-3, stats["near"]
    assert stats["reward_arg_min"] > 1e-3 and stats["n2_min"] > 100 * ref.TURN_N2


def test_pack_and_unpack_pid_are_inverse_and_differentiable():
    from gym_pybullet_drones_amd.diff import pack_pid, unpack_pid
    g = torch.Generator().manual_seed(0)
    parts = [torch.randn((70, 3), generator=g, dtype=torch.float64, requires_grad=True) for _ in range(3)]
    pid = pack_pid(*parts)
    assert pid.shape == (9, 128) and not pid[:, 70:].any()
    assert torch.equal(pid[:, :70], torch.cat(parts, dim=1).detach().t())          # rows: integral pos e | last rpy | integral rpy e
    assert all(torch.equal(a, b) for a, b in zip(unpack_pid(pid, 70), parts))
    w = torch.randn(pid.shape, generator=g, dtype=torch.float64)
    grads = torch.autograd.grad((pid * w).sum(), parts)
    assert all(torch.equal(a, b) for a, b in zip(grads, unpack_pid(w, 70)))


# ---- csrc/dslpid_vjp.inc and the entries' host side: one run of tests/c/diff_pid_host.c -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_run():
    from gym_pybullet_drones_amd import _native
    exe = host_lib.program("diff_pid_host", include=(_native.CSRC,))
    values = os.path.join(os.path.dirname(exe), "dslpid_formulas.txt")
    return host_lib.run(exe, values), values


#: the slices of a line of the formulas file: the inputs X (34), the outputs' cotangents (13), the inputs' cotangents (34), the gains' (18)
_X = dict(pos=(0, 3), vel=(3, 6), R=(6, 15), rpy=(15, 18), tpos=(18, 21), tyaw=(21, 22), tvel=(22, 25), ip=(25, 28), lrpy=(28, 31), ir=(31, 34))


def test_controller_adjoint_compiled_for_the_host_matches_float64_autograd():
    """csrc/dslpid_vjp.inc -- the text the device sweep compiles -- evaluated in a plain C program on 400 controller calls (under the
    sanitizers), against float64 autograd of the restatement's controller alone at the same float32 inputs: max |a32 - a64| / max |a64|
    per output group over the calls.  First-run bound 1e-4 (the project's fp32 tolerance).  MEASURED on the host build (libm's square
    roots, not the device's): 1.5e-05 at most (the d_tor group; 3.3e-07 at most outside the two torque-gain groups), DESIGN.md section 3.16."""
    run, path = _host_run()
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    lines = open(path).read().splitlines()
    dt, gravity, kf = [float(v) for v in lines[0].split()][:3]
    rows = np.array([[float(v) for v in l.split()] for l in lines[1:]])
    assert rows.shape == (400, 34 + 13 + 34 + 18)
    X, o, a, G = rows[:, :34], rows[:, 34:47], rows[:, 47:81], rows[:, 81:]
    leaf = lambda v: T(v).clone().requires_grad_(True)     # noqa: E731
    e_p = leaf(X[:, 18:21] - X[:, 0:3])
    vel, Rm, rpy, tyaw, tvel = (leaf(X[:, slice(*_X[k])]) for k in ("vel", "R", "rpy", "tyaw", "tvel"))
    mem = tuple(leaf(X[:, slice(*_X[k])]) for k in ("ip", "lrpy", "ir"))
    gains = leaf(np.asarray(pref.DEFAULT_GAINS, dtype=np.float32).astype(np.float64))
    pc = pref.pid_consts(np.float32(gravity), np.float32(kf), 0.25, gains)
    stats = {}
    R = [[Rm[:, 3 * i + j] for j in range(3)] for i in range(3)]
    rpm, mem_k = pref.controller(pc, dt, e_p, vel, R, rpy, tyaw[:, 0], tvel, mem, stats)
    # per-call gradients: the calls are independent, so the gradient of the sum is the stack of the calls' own
    loss = (T(o[:, 0:4]) * rpm).sum() + sum((T(o[:, 4 + 3 * i:7 + 3 * i]) * m).sum() for i, m in enumerate(mem_k))
    g = torch.autograd.grad(loss, (e_p, vel, Rm, rpy, tyaw, tvel) + mem)
    want = dict(tpos=g[0], pos=-g[0], vel=g[1], R=g[2], rpy=g[3], tyaw=g[4], tvel=g[5], ip=g[6], lrpy=g[7], ir=g[8])
    err = {k: float(np.abs(a[:, slice(*_X[k])] - want[k].numpy()).max() / np.abs(want[k].numpy()).max()) for k in _X}
    # the gains' cotangents are per call in the file, autograd's a sum over calls: compare float64 sums of the C values over blocks of calls
    per_call = []
    for i in range(0, 400, 100):          # the gains group by group on four blocks of calls (a sum over few calls hides less)
        sl = slice(i, i + 100)
        rpm_b, mem_b = pref.controller(pc, dt, e_p[sl], vel[sl], [[c[sl] for c in r] for r in R], rpy[sl], tyaw[sl, 0], tvel[sl], tuple(m[sl] for m in mem))
        lb = (T(o[sl, 0:4]) * rpm_b).sum() + sum((T(o[sl, 4 + 3 * j:7 + 3 * j]) * m).sum() for j, m in enumerate(mem_b))
        per_call.append((torch.autograd.grad(lb, gains)[0].numpy(), G[sl].sum(0).reshape(6, 3)))
    for j, name in enumerate(pref.GAINS):
        err[name] = max(float(np.abs(got[j] - ref_[j]).max() / np.abs(ref_[j]).max()) for ref_, got in per_call)
    print("MEASURED dslpid_vjp_host", " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    # the draws meet every clamp on both sides (so the adjoint's selects are all exercised) ...
    assert stats["int_z_saturated"] > 20 and stats["int_z_free"] > 20 and stats["pwm_saturated"] > 50 and stats["pwm_free"] > 50
    # ... and none of them sits where float32 and float64 could disagree about a branch
    assert min(stats["near"].values()) > 1e-5, stats["near"]
    assert max(err.values()) < 1e-4, err


def test_host_side_of_the_pid_entries_under_asan_and_ubsan():
    """tests/c/diff_pid_host.c linked to the host-only build of the five units and the launch stub under -fsanitize=address,undefined:
    the tape's size, one launch per accepted call with its geometry and the instantiation (three widths, with and without g_gains),
    every refusal with its code and message, nothing launched by a refusal"""
    run, _ = _host_run()
    print(run.stdout[-6000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") >= 100
    for kernel in ("gpd_rollout_tape_pid_kernel<AW 3>", "gpd_rollout_tape_pid_kernel<AW 4>", "gpd_rollout_tape_pid_kernel<AW 1>", "<AW 3, GG 1>",
                   "<AW 3, GG 0>", "<AW 4, GG 1>", "<AW 4, GG 0>", "<AW 1, GG 1>", "<AW 1, GG 0>"):
        assert kernel in run.stdout, kernel


# ---- the entries through ctypes ------------------------------------------------------------------------------------------------------
def _calls(L, P, cfg, st, p, out):
    return {
        "gpd_rollout_tape_pid_floats": lambda: L.gpd_rollout_tape_pid_floats(ctypes.byref(cfg), 4, 128, ctypes.byref(out)),
        "gpd_rollout_tape_pid": lambda: L.gpd_rollout_tape_pid(ctypes.byref(P), ctypes.byref(st), ctypes.byref(cfg), 4, p, 280, p, p, 840, p, p, p, 70, p, None),
        "gpd_rollout_vjp_pid": lambda: L.gpd_rollout_vjp_pid(ctypes.byref(P), ctypes.byref(cfg), 128, 4, p, 280, p, p, p, 840, p, 70, p, p, p, p, None),
    }


@pytest.mark.parametrize("change,code,reason", [
    (dict(act_type=0), "ENOTSUP", "gpd_rollout_tape / gpd_rollout_vjp"), (dict(act_type=3), "ENOTSUP", "gpd_rollout_tape / gpd_rollout_vjp"),
    (dict(act_type=5), "ENOTSUP", "gpd_rollout_tape / gpd_rollout_vjp"), (dict(act_type=6), "ENOTSUP", "gpd_rollout_tape / gpd_rollout_vjp"),
    (dict(physics_flags=2), "ENOTSUP", "physics_flags"), (dict(physics_flags=1), "ENOTSUP", "physics_flags"),
    (dict(physics_flags=4), "ENOTSUP", "physics_flags"), (dict(physics_flags=8), "ENOTSUP", "physics_flags"),
    (dict(physics_flags=16), "ENOTSUP", "physics_flags"), (dict(drones_per_env=2, num_envs=35), "ENOTSUP", "drones_per_env"),
    (dict(task=2), "ENOTSUP", "task"), (dict(auto_reset=1), "ENOTSUP", "auto_reset"), (dict(act_type=9), "EINVAL", "act_type"),
    (dict(substeps=0), "EINVAL", "positive"), (dict(num_envs=2 ** 26 + 1), "EINVAL", "ld")])
def test_unsupported_configurations_are_refused_with_entry_and_reason(change, code, reason):
    """every entry, every rejected configuration: the code and a message that starts with the entry's name and gives the reason.  The
    pointers are fake: a call that got as far as a launch would not return a negative code on a machine without a device."""
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    L = _native.lib()
    P = _params("cf2x").to_struct(pid_model=DroneModel.CF2X)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cfg = _cfg(**dict(dict(act_type=2, substeps=5), **change))
    st = _native.GpdState(kin=p.value, last_rpm=p.value, pid=p.value, step_counter=p.value, ld=128)
    for name, f in _calls(L, P, cfg, st, p, ctypes.c_int64(0)).items():
        assert f() == getattr(_native, "GPD_" + code), name
        msg = L.gpd_last_error().decode()
        assert msg.startswith(name + ":") and reason in msg, msg


def test_racer_dw_force_missing_members_and_bad_arguments_are_refused():
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    L = _native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    cfg = _cfg(act_type=1, substeps=5)
    ok = dict(kin=p.value, last_rpm=p.value, pid=p.value, step_counter=p.value, ld=128)
    racer = _params("racer").to_struct(pid_model=DroneModel.RACE)          # (no DSLPID for this airframe: pid_kf stays 0)
    for name, f in list(_calls(L, racer, cfg, _native.GpdState(**ok), p, ctypes.c_int64(0)).items())[1:]:
        assert f() == _native.GPD_ENOTSUP and L.gpd_last_error().decode().startswith(name + ": no DSLPID controller"), name
    P = _params("cf2x").to_struct(pid_model=DroneModel.CF2X)

    def tape(st, K=4, tape_=p, target=p, a_stride=210):
        return L.gpd_rollout_tape_pid(ctypes.byref(P), ctypes.byref(st), ctypes.byref(cfg), K, p, a_stride, target, p, 840, p, p, p, 70, tape_, None)

    def vjp(K=4, ld=128, g_kin=p, g_pid=p, g_act=p, g_gains=None, tape_=p):
        return L.gpd_rollout_vjp_pid(ctypes.byref(P), ctypes.byref(cfg), ld, K, p, 210, p, tape_, None, 840, None, 70, g_kin, g_pid, g_act, g_gains, None)

    assert tape(_native.GpdState(**dict(ok, dw_force=p.value))) == _native.GPD_ENOTSUP and b"gpd_rollout_tape_pid: state.dw_force" in L.gpd_last_error()
    assert tape(_native.GpdState(**dict(ok, pid=None))) == _native.GPD_EINVAL and b"gpd_rollout_tape_pid: PID action type needs state.pid" in L.gpd_last_error()
    for rc in (tape(_native.GpdState(**ok), K=0), tape(_native.GpdState(**ok), tape_=None), tape(_native.GpdState(**ok), tape_=odd),
               tape(_native.GpdState(**ok), target=None), tape(_native.GpdState(**ok), a_stride=-1), tape(_native.GpdState(**dict(ok, ld=64))),
               tape(_native.GpdState(**dict(ok, kin=odd.value)))):
        assert rc == _native.GPD_EINVAL and L.gpd_last_error().decode().startswith("gpd_rollout_tape_pid:")
    for rc in (vjp(K=0), vjp(ld=64), vjp(g_kin=None), vjp(g_kin=odd), vjp(g_pid=None), vjp(g_pid=odd), vjp(g_act=None),
               vjp(g_gains=odd), vjp(tape_=None), vjp(tape_=odd)):
        assert rc == _native.GPD_EINVAL and L.gpd_last_error().decode().startswith("gpd_rollout_vjp_pid:")
    # g_actions has to be 16-byte aligned where its rows are stored as float4: under VEL (tests/c/diff_pid_host.c: PID accepts the offset)
    vel = _cfg(act_type=2, substeps=5)
    rc = L.gpd_rollout_vjp_pid(ctypes.byref(P), ctypes.byref(vel), 128, 4, p, 280, p, p, None, 840, None, 70, p, p, odd, None, None)
    assert rc == _native.GPD_EINVAL and b"gpd_rollout_vjp_pid: g_actions must be 16-byte aligned" in L.gpd_last_error()


def test_size_query_gives_twenty_two_rows_per_step():
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    out = ctypes.c_int64(-1)
    for K, ld in ((1, 128), (20, 128), (20, 65536), (64, 1 << 26)):
        cfg = _cfg(num_envs=min(ld, 70), act_type=2, substeps=5)
        assert L.gpd_rollout_tape_pid_floats(ctypes.byref(cfg), K, ld, ctypes.byref(out)) == 0
        assert out.value == 22 * K * ld
    assert L.gpd_rollout_tape_pid_floats(ctypes.byref(_cfg(act_type=2)), 2 ** 31 - 1, 2 ** 32 - 1, ctypes.byref(out)) == _native.GPD_ERANGE


def test_new_entries_are_bound_and_the_abi_version_stays():
    from gym_pybullet_drones_amd import _native, diff, engine
    from gym_pybullet_drones_amd.envs.VectorAviary import VectorAviary
    assert _native.ABI_VERSION == 9 and _native.lib().gpd_abi_version() == 9
    assert {"gpd_rollout_tape_pid_floats", "gpd_rollout_tape_pid", "gpd_rollout_vjp_pid"} <= set(_native.exported_symbols())
    assert len(_native.UNITS) == 5 and {"dslpid_vjp.inc", "diff_pid_kernels.inc"} <= set(_native.HEADERS)
    assert all(os.path.exists(os.path.join(_native.CSRC, h)) for h in _native.HEADERS)
    assert callable(engine.SimCore.rollout_diff_pid) and callable(VectorAviary.rollout_diff_pid)
    assert all(callable(getattr(diff, f)) for f in ("tape_floats_pid", "tape_forward_pid", "sweep_pid", "pack_pid", "unpack_pid"))


def test_params_with_gains_replaces_the_eighteen_gains_of_a_copy():
    from gym_pybullet_drones_amd import diff
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    P = _params("cf2x").to_struct(pid_model=DroneModel.CF2X)
    own = diff.gains_of(P)
    assert own.shape == (6, 3) and np.allclose(own.numpy(), pref.DEFAULT_GAINS)
    Q = diff.params_with_gains(P, own * 2)
    assert torch.equal(diff.gains_of(Q), own * 2) and torch.equal(diff.gains_of(P), own)          # (the core's block is untouched)
    Q2 = diff.params_with_gains(P, own)
    assert bytes(Q2) == bytes(P)                                                                  # (own gains: the same bytes)

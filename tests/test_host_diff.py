"""The differentiable rollout without a GPU: the float64 yardstick (tests/helpers/diff_f64.py) held against the batched oracle and
against finite differences, its float32 run against its float64 run on the GPU tests' inputs, the safety caps of those inputs, and the
host side of the three new entries (include/gpd.h `gpd_rollout_tape_floats` / `gpd_rollout_tape` / `gpd_rollout_vjp`): the size query,
every rejected configuration with its code and message, and tests/c/diff_host.c under AddressSanitizer + UBSan against the launch stub."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, urdf

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import diff_f64 as ref  # noqa: E402
import host_lib  # noqa: E402
from host_lib import REJECTED, params as _params, step_cfg as _cfg  # noqa: E402


@pytest.mark.parametrize("model", ["cf2x", "cf2p", "racer"])
@pytest.mark.parametrize("drag", [False, True])
@pytest.mark.parametrize("S", [1, 8])
def test_restatement_forward_is_the_batched_oracle(model, drag, S):
    """obs12, reward and the state of 3 steps equal oracle.batched_oracle's to 1e-12 (RPM actions; cf2x also the clipped raw RPMs and
    the one-value action)"""
    from oracle.batched_oracle import BatchedAviary
    n, K = 5, 3
    for act in (("rpm", "raw_rpm", "one_d_rpm") if model == "cf2x" else ("rpm",)):
        cfg = ref.config(model, act, S, drag, "hover")
        orc = BatchedAviary(urdf(model), model, n, 1, physics_flags=2 if drag else 0, pyb_freq=240, ctrl_freq=240 // S, act=act, task="hover")
        inp = ref.make_inputs(orc.C, cfg, n, K, seed=3)
        orc.pos[:, 0], orc.quat[:, 0], orc.vel[:, 0], orc.rpy_rates[:, 0], orc.last_rpm[:, 0] = inp.pos, inp.quat, inp.vel, inp.rates, inp.last_rpm
        c = ref.consts(orc.C, n)
        T = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731
        obs, rew, kin = ref.rollout(c, cfg, tuple(T(v) for v in (inp.pos, inp.quat, inp.vel, inp.rates)), T(inp.actions),
                                    T(inp.last_rpm).sum(-1), T(inp.target))
        for t in range(K):
            o64, r64, _, _, _ = orc.step(inp.actions[t].reshape(n, 1, -1))
            assert np.abs(obs[t].numpy() - o64[:, 0]).max() < 1e-12, (act, t)
            assert np.abs(rew[t].numpy() - r64).max() < 1e-12, (act, t)
        for got, want in zip(kin, (orc.pos, orc.quat, orc.vel, orc.rpy_rates)):
            assert np.abs(got.numpy() - want[:, 0]).max() < 1e-12


@pytest.mark.parametrize("act,drag,S", [("rpm", True, 2), ("one_d_rpm", False, 1), ("raw_rpm", False, 1)])
def test_restatement_gradients_pass_gradcheck(act, drag, S):
    """float64 autograd of the restatement against finite differences: 2 drones, K = 3"""
    C = _params("cf2x")
    cfg = ref.config("cf2x", act, S, drag, "hover")
    inp = ref.make_inputs(C, cfg, 2, 3, seed=5, outside_clip=False)
    c = ref.consts(C, 2)
    T = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731
    scale = 1.0 if act == "rpm" or act == "one_d_rpm" else 1e-3      # (raw RPMs are ~1e4: differentiate in units of 1000 rpm)

    def f(pos, quat, vel, rates, a):
        obs, rew, kin = ref.rollout(c, cfg, (pos, quat, vel, rates), a / scale, T(inp.first_sum), T(inp.target))
        return torch.cat([obs.reshape(-1), rew.reshape(-1)] + [k.reshape(-1) for k in kin])

    args = [T(v).clone().requires_grad_(True) for v in (inp.pos, inp.quat, inp.vel, inp.rates, inp.actions * scale)]
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.fixture(scope="module")
def case_runs():
    """every GPU case once: the float64 gradients with the forward's safety statistics, and the float32 run of the same restatement"""
    out = {}
    for name in ref.GPU_CASES:
        cfg, K, scales = ref.case(name)
        C = _params(cfg.model)
        inp = ref.make_inputs(C, cfg, 70, K, seed=1)
        stats = {}
        g64 = ref.reference_grads(C, cfg, inp, torch.float64, scales, stats=stats)
        g32 = ref.reference_grads(C, cfg, inp, torch.float32, scales)
        out[name] = (C, cfg, inp, g64, g32, stats)
    return out


@pytest.mark.parametrize("name", list(ref.GPU_CASES))
def test_float32_restatement_follows_the_float64_one_on_the_gpu_inputs(case_runs, name):
    """what float32 costs on these inputs, measured on the restatement itself: max |g32 - g64| / max |g64| per group stays below 1e-5
    (so that a device gradient within 1e-4 of the float64 one is a statement about the kernel, not about the inputs' conditioning)"""
    _, _, _, g64, g32, _ = case_runs[name]
    err = ref.group_errors(g32, g64)
    print(name, {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) < 1e-5, err
    assert all(np.isfinite(g64[k]).all() and np.abs(g64[k]).max() > 0 for k in ref.GROUPS)


@pytest.mark.parametrize("name", list(ref.GPU_CASES))
def test_gpu_inputs_stay_inside_the_references_safety_caps(case_runs, name):
    """no drone comes within 1e-3 of the gimbal threshold, the reward clamp or a RAW_RPM bound, and no |w|^2 within a factor 100 of
    the 1e-16 of the no-turn test: on either side of such a threshold float32 and float64 may take different branches"""
    C, cfg, inp, _, _, stats = case_runs[name]
    assert stats["sarg_max"] < ref.GIMBAL - 1e-3
    assert stats["reward_arg_min"] > 1e-3
    assert stats["n2_min"] > 100 * ref.TURN_N2
    if cfg.act == "raw_rpm":
        a = inp.actions
        assert np.minimum(np.abs(a), np.abs(a - C.MAX_RPM)).min() > 1e-3
        outside = ((a < 0) | (a > C.MAX_RPM)).mean()
        assert 0.25 < outside < 0.42, outside          # "a third of the actions outside the clip"


def test_at_rest_inputs_take_the_no_turn_branch_with_finite_gradients():
    """ONE_D_RPM from body rates exactly zero: equal thrusts, no torque, |w| stays 0 -- the `turn` select keeps q, and the restatement's
    gradients are finite there (a plain sin(t) / |w| is NaN)"""
    C = _params("cf2x")
    cfg = ref.config("cf2x", "one_d_rpm", 2, False, "hover")
    inp = ref.make_inputs(C, cfg, 70, 4, seed=2, at_rest=True)
    stats = {}
    g = ref.reference_grads(C, cfg, inp, torch.float64, stats=stats)
    assert stats["n2_min"] == 0.0
    assert all(np.isfinite(g[k]).all() for k in ref.GROUPS) and np.abs(g["actions"]).max() > 0


def test_pack_and_unpack_kin_are_inverse_and_differentiable():
    from gym_pybullet_drones_amd.diff import pack_kin, unpack_kin
    from gym_pybullet_drones_amd.engine import kin_rows_from_planes
    g = torch.Generator().manual_seed(0)
    parts = [torch.randn((70, k), generator=g, dtype=torch.float64, requires_grad=True) for k in (3, 4, 3, 3)]
    kin = pack_kin(*parts)
    assert kin.shape == (13 * 128,)
    rows = kin_rows_from_planes(kin.detach(), 128)                 # the engine's own reading of the plane layout
    assert torch.equal(rows[:, :70], torch.cat(parts, dim=1).detach().t()) and not rows[:, 70:].any()
    back = unpack_kin(kin, 70)
    assert all(torch.equal(a, b) for a, b in zip(back, parts))
    w = torch.randn(kin.shape, generator=g, dtype=torch.float64)
    grads = torch.autograd.grad((kin * w).sum(), parts)
    ws = unpack_kin(w, 70)
    assert all(torch.equal(a, b) for a, b in zip(grads, ws))


# ---- the host side of the entries -------------------------------------------------------------------------------------------------
def test_size_query_gives_thirteen_rows_per_step_and_one():
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    out = ctypes.c_int64(-1)
    for K, ld in ((1, 128), (20, 128), (20, 65536), (64, 1 << 26)):
        cfg = _cfg(num_envs=min(ld, 70))
        assert L.gpd_rollout_tape_floats(ctypes.byref(cfg), K, ld, ctypes.byref(out)) == 0
        assert out.value == (13 * K + 1) * ld
    assert L.gpd_rollout_tape_floats(ctypes.byref(_cfg()), 1, 64, ctypes.byref(out)) == _native.GPD_EINVAL        # ld < 70 drones
    assert L.gpd_rollout_tape_floats(ctypes.byref(_cfg()), 2 ** 31 - 1, 2 ** 32 - 1, ctypes.byref(out)) == _native.GPD_ERANGE


@pytest.mark.parametrize("change,reason", REJECTED)
def test_unsupported_configurations_return_enotsup_with_entry_and_reason(change, reason):
    """every entry, every rejected configuration: GPD_ENOTSUP and a message that starts with the entry's name and gives the reason.
    The pointers are fake addresses: a call that got as far as a launch would not return a negative code on a machine without a
    device (tests/c/diff_host.c counts the launches against the stub: none)."""
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    L = _native.lib()
    P = _params("cf2x").to_struct(pid_model=DroneModel.CF2X)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cfg = _cfg(**change)
    st = _native.GpdState(kin=p.value, last_rpm=p.value, step_counter=p.value, ld=128)
    out = ctypes.c_int64(0)
    calls = {
        "gpd_rollout_tape_floats": lambda: L.gpd_rollout_tape_floats(ctypes.byref(cfg), 4, 128, ctypes.byref(out)),
        "gpd_rollout_tape": lambda: L.gpd_rollout_tape(ctypes.byref(P), ctypes.byref(st), ctypes.byref(cfg), 4, p, 280, p, p, 840, p, p, p, 70, None, p, None),
        "gpd_rollout_vjp": lambda: L.gpd_rollout_vjp(ctypes.byref(P), ctypes.byref(cfg), 128, 4, p, 280, p, None, p, p, 840, p, 70, p, p, None),
    }
    for name, f in calls.items():
        assert f() == _native.GPD_ENOTSUP, name
        msg = L.gpd_last_error().decode()
        assert msg.startswith(name + ":") and reason in msg, msg


def test_dw_force_and_bad_arguments_are_refused_before_any_device_work():
    from gym_pybullet_drones_amd import _native
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    L = _native.lib()
    P = _params("cf2x").to_struct(pid_model=DroneModel.CF2X)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    cfg = _cfg()

    def tape(st, K=4, tape_=p, target=p, plant=None, a_stride=280, cfg_=cfg):
        return L.gpd_rollout_tape(ctypes.byref(P), ctypes.byref(st), ctypes.byref(cfg_), K, p, a_stride, target, p, 840, p, p, p, 70, plant, tape_, None)

    def vjp(K=4, ld=128, g_kin=p, g_act=p, tape_=p):
        return L.gpd_rollout_vjp(ctypes.byref(P), ctypes.byref(cfg), ld, K, p, 280, p, None, tape_, None, 840, None, 70, g_kin, g_act, None)

    ok = dict(kin=p.value, last_rpm=p.value, step_counter=p.value, ld=128)
    assert tape(_native.GpdState(**dict(ok, dw_force=p.value))) == _native.GPD_ENOTSUP and b"gpd_rollout_tape: state.dw_force" in L.gpd_last_error()
    for rc in (tape(_native.GpdState(**ok), K=0), tape(_native.GpdState(**ok), tape_=None), tape(_native.GpdState(**ok), tape_=odd),
               tape(_native.GpdState(**ok), target=None), tape(_native.GpdState(**ok), plant=odd), tape(_native.GpdState(**ok), a_stride=-1),
               tape(_native.GpdState(**dict(ok, ld=64))), tape(_native.GpdState(**dict(ok, last_rpm=None)), cfg_=_cfg(physics_flags=2)),
               tape(_native.GpdState(**dict(ok, kin=odd.value)))):
        assert rc == _native.GPD_EINVAL and L.gpd_last_error().decode().startswith("gpd_rollout_tape:")
    for rc in (vjp(K=0), vjp(ld=64), vjp(g_kin=None), vjp(g_kin=odd), vjp(g_act=None), vjp(g_act=odd), vjp(tape_=None), vjp(tape_=odd)):
        assert rc == _native.GPD_EINVAL and L.gpd_last_error().decode().startswith("gpd_rollout_vjp:")


def test_new_entries_are_bound_and_the_abi_version_stays():
    from gym_pybullet_drones_amd import _native
    assert _native.ABI_VERSION == 9 and _native.lib().gpd_abi_version() == 9
    assert {"gpd_rollout_tape_floats", "gpd_rollout_tape", "gpd_rollout_vjp"} <= set(_native.exported_symbols())
    assert len(_native.UNITS) == 5 and "diff_kernels.inc" in _native.HEADERS


def test_host_side_of_the_diff_entries_under_asan_and_ubsan():
    """tests/c/diff_host.c linked to the host-only build of the five units and the launch stub under -fsanitize=address,undefined
    (tests/helpers/host_lib.py; one run, shared with tests/test_host_sysid.py): accepted and rejected arguments, and the kernel each
    accepted call launches"""
    run, _ = host_lib.diff_host()
    print(run.stdout[-4000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") + run.stdout.startswith("ok ") >= 60 + 50          # (this module's entries + the plant-gradient ones)
    assert "gpd_rollout_tape_kernel" in run.stdout and "gpd_rollout_vjp_kernel" in run.stdout          # (the kernels are named)

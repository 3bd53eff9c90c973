"""The differentiable rollout without a GPU: the float64 yardstick (tests/helpers/diff_f64.py) held against the batched oracle and
against finite differences (on the far side of the tumbling and gimbal selects too), its float32 run against its float64 run on the GPU
tests' inputs, the safety caps of those inputs, the conditions of the edge cases (which lanes sit on which side of every select, with
what margin), and the
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


# ---- the far side of the selects: the conditions of the edge cases (conditions, not measurements) -------------------------------------
@pytest.fixture(scope="module")
def edge_runs():
    """every edge case once, as `case_runs`: the statistics now per lane"""
    out = {}
    for kind in ref.EDGE_CASES:
        cfg, K = ref.edge_case(kind)
        C = _params(cfg.model)
        inp = ref.make_edge_inputs(C, cfg, ref.EDGE_N, K, kind)
        stats = {}
        g64 = ref.reference_grads(C, cfg, inp, torch.float64, stats=stats)
        g32 = ref.reference_grads(C, cfg, inp, torch.float32)
        out[kind] = (C, cfg, inp, g64, g32, stats)
    return out


def _sides(stats):
    """per lane, over every step and sub-step of a run: which side of each select it sat on, or neither (inside the margin).  The
    margins: 1e-3 below and 5e-6 above the gimbal test, 1e-3 on either side of the reward clamp, a factor 100 above the no-turn test
    or exactly at rest, 1e-2 on either side of the tumbling test u = 1."""
    L = stats["lanes"]
    return dict(gimbal=L["sarg_abs"][0] >= ref.GIMBAL + 5e-6, regular=L["sarg_abs"][1] < ref.GIMBAL - 1e-3,
                far=L["reward_arg"][1] < -1e-3, near=L["reward_arg"][0] > 1e-3,
                turning=L["n2"][0] > 100 * ref.TURN_N2, at_rest=L["n2"][1] == 0.0,
                tumbling=L["u"][0] - 1.0 > 1e-2, slow=L["u"][1] < 1.0 - 1e-2)


#: the side the rare lanes of each kind sit on at every step and sub-step (every other select: the ordinary side)
RARE_SIDE = {"tumble": {"tumbling"}, "gimbal": {"gimbal", "at_rest"}, "near_gimbal": {"at_rest"}, "reward_far": {"far"}, "wide_attitude": set()}


def test_edge_cases_cover_the_three_airframes_on_four_waves():
    assert {d["model"] for d in ref.EDGE_CASES.values()} == {"cf2x", "cf2p", "racer"}
    assert ref.EDGE_N == 200 and (ref.EDGE_N + 63) // 64 == 4
    rare = ref.rare_lanes()
    assert rare[:128:3].all() and rare.sum() == 43 and not rare[128:].any()          # waves 0 and 1 diverge, waves 2 and 3 do not
    assert ref.EDGE_CASES["tumble"]["K"] * ref.EDGE_CASES["tumble"]["S"] <= 8


@pytest.mark.parametrize("kind", list(ref.EDGE_CASES))
def test_edge_inputs_sit_on_the_intended_side_of_every_select_with_margin(edge_runs, kind):
    """the rare lanes on the far side at EVERY step and sub-step with the margins of `_sides`, every other lane -- and the rare lanes at
    every other select -- on the ordinary side with the margins of the GPU cases: float32 and float64 take the same branches.  Both
    sides are populated: at least 40 rare lanes and 100 ordinary ones."""
    _, cfg, inp, _, _, stats = edge_runs[kind]
    side, rare = _sides(stats), inp.rare
    assert rare.sum() >= 40 and (~rare).sum() >= 100
    for far, ordinary in (("gimbal", "regular"), ("far", "near"), ("at_rest", "turning"), ("tumbling", "slow")):
        assert (side[far] | side[ordinary]).all(), (far, ordinary)                  # (no lane inside a margin, or on both sides in turn)
        want = rare if far in RARE_SIDE[kind] else np.zeros_like(rare)
        assert np.array_equal(side[far], want), far
    L = stats["lanes"]
    if kind == "tumble":
        assert stats["u_max"] > 1.0 + 1e-2 and L["u"][0][rare].min() - 1.0 > 1e-2 and L["u"][1][~rare].max() < 1e-3
        assert np.count_nonzero(inp.rates[rare, :2].any(axis=1)) >= 20 and np.count_nonzero(~inp.rates[rare, :2].any(axis=1)) >= 20     # off z, about z
    if kind == "gimbal":
        assert L["sarg_abs"][0][rare].min() >= ref.GIMBAL + 5e-6 and L["sarg_abs"][1][rare].max() > 1.0      # (some above 1: rsq of a negative)
    if kind == "near_gimbal":
        assert L["sarg_abs"][0][rare].min() > 0.99 and L["sarg_abs"][1][rare].max() < ref.GIMBAL - 1e-3
    if kind == "reward_far":
        assert L["reward_arg"][1][rare].max() < -1e-3 and L["reward_arg"][0][~rare].min() > 1e-3
    if kind == "wide_attitude":
        q = inp.quat[rare]
        length = np.linalg.norm(q, axis=1)
        assert (q[:, 3] < 0).sum() >= 10 and (q[:, 3] > 0).sum() >= 10
        assert (length < 0.99).sum() >= 10 and (length > 1.01).sum() >= 5 and L["sarg_abs"][1][rare].max() > 0.9


@pytest.mark.parametrize("kind", list(ref.EDGE_CASES))
def test_float32_restatement_follows_the_float64_one_on_the_edge_inputs(edge_runs, kind):
    """the rule of the GPU cases, unchanged: max |g32 - g64| / max |g64| per group below 1e-5 on the restatement itself, finite
    gradients, and a forward whose float32 run stays within 1e-5 of each observation column's scale"""
    _, _, _, g64, g32, _ = edge_runs[kind]
    err = ref.group_errors(g32, g64)
    print(kind, {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) < 1e-5, err
    assert all(np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0 for k in ref.GROUPS for g in (g64, g32))
    assert ref.forward_error(g32["forward"][0].numpy(), g64["forward"][0].numpy()) < 1e-5
    # the GPU test also holds the rare lanes on their own (a larger gradient elsewhere must not hide them): the same rule there
    rare = edge_runs[kind][2].rare
    lanes = lambda g: {k: (g[k][:, rare] if k == "actions" else g[k][rare]) for k in ref.GROUPS}     # noqa: E731
    err = ref.group_errors(lanes(g32), lanes(g64))
    print(kind, "rare lanes", {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) < 1e-5, err


def test_tumbling_with_plant_scales_meets_the_same_conditions():
    """`tumble` with per-drone scales within +-20 % and the scales as leaves (the GPU suite's run through gpd_rollout_vjp_plant, the first
    step of the case): the rare lanes tumble at every sub-step, nobody else does, every other select keeps its margin, and the float32 restatement stays
    within 1e-5 of the float64 one -- the five groups and every scale the configuration reads"""
    import sysid_f64 as sid
    cfg, K = ref.edge_case("tumble")
    C = _params(cfg.model)
    inp, scales = ref.first_steps(ref.make_edge_inputs(C, cfg, ref.EDGE_N, K, "tumble"), ref.TUMBLE_PLANT_K), ref.edge_scales()
    stats = {}
    g64 = ref.reference_grads(C, cfg, inp, torch.float64, scales, stats=stats, wrt_scales=True)
    g32 = ref.reference_grads(C, cfg, inp, torch.float32, scales, wrt_scales=True)
    side = _sides(stats)
    assert np.array_equal(side["tumbling"], inp.rare) and np.array_equal(side["slow"], ~inp.rare)
    assert side["regular"].all() and side["near"].all() and side["turning"].all()
    err = dict(ref.group_errors(g32, g64), **sid.scale_errors(g32["scales"], g64["scales"]))
    print({k: f"{v:.1e}" for k, v in err.items()})
    assert set(err) == set(ref.GROUPS) | {"mass", "ixx", "iyy", "izz", "kf", "km"}
    assert max(err.values()) < 1e-5, err


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_size_sweep_inputs_meet_the_rules_of_the_gpu_cases(n):
    """the GPU suite's size sweep (RPM, S = 2, K = 4, drag, `make_inputs` at N drones): the 1e-5 rule and the safety caps at every N"""
    cfg = ref.config("cf2x", "rpm", 2, True, "hover")
    C = _params("cf2x")
    inp = ref.make_inputs(C, cfg, n, 4, seed=1)
    stats = {}
    g64 = ref.reference_grads(C, cfg, inp, torch.float64, stats=stats)
    err = ref.group_errors(ref.reference_grads(C, cfg, inp, torch.float32), g64)
    assert max(err.values()) < 1e-5, err
    assert stats["sarg_max"] < ref.GIMBAL - 1e-3 and stats["reward_arg_min"] > 1e-3 and stats["n2_min"] > 100 * ref.TURN_N2 and stats["u_max"] < 1e-3


@pytest.mark.parametrize("kind", ["tumble", "gimbal", "wide_attitude"])
def test_restatement_gradients_pass_gradcheck_on_the_far_side(kind):
    """the yardstick itself on the far side of the tumbling and gimbal selects and at wide attitudes: float64 autograd against finite
    differences on 3 rare lanes (drones 0, 3 and 6 of a draw of 7), the eps and tolerances of the gradcheck above"""
    cfg, K = ref.edge_case(kind)
    C = _params(cfg.model)
    inp = ref.lanes_of(ref.make_edge_inputs(C, cfg, 7, K, kind, seed=5), [0, 3, 6])
    if kind == "gimbal":
        # The gimbal lanes are at rest, and the no-turn select is a kink of its own: the function as executed keeps q there, a finite
        # difference in the rates leaves it.  Here they roll instead: at pitch +-pi/2 the body's x axis is the vertical, a roll rate
        # turns the yaw alone, J w is parallel to w and nothing makes a torque -- the lane turns and stays in the gimbal branch.
        inp.rates[:, 0] = np.array([0.75, -0.5, 0.25])
    c = ref.consts(C, 3)
    T = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731
    stats = {}

    def f(pos, quat, vel, rates, a, st=None):
        obs, rew, kin = ref.rollout(c, cfg, (pos, quat, vel, rates), a, T(inp.first_sum), T(inp.target), st)
        return torch.cat([obs.reshape(-1), rew.reshape(-1)] + [k.reshape(-1) for k in kin])

    args = [T(v).clone().requires_grad_(True) for v in (inp.pos, inp.quat, inp.vel, inp.rates, inp.actions)]
    f(*args, st=stats)
    side = _sides(stats)
    assert inp.rare.all() and all(side[k].all() for k in RARE_SIDE[kind] - ({"at_rest"} if kind == "gimbal" else set()))
    assert all((side[a] | side[b]).all() for a, b in (("gimbal", "regular"), ("far", "near"), ("at_rest", "turning"), ("tumbling", "slow")))
    assert torch.autograd.gradcheck(f, args, eps=1e-6, atol=1e-6, rtol=1e-5)


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

"""The differentiable rollout on the device (include/gpd.h `gpd_rollout_tape` / `gpd_rollout_vjp`, gym_pybullet_drones_amd/diff.py):
the taped forward against `gpd_rollout` / `gpd_rollout_plant` bit for bit, the reverse sweep against float64 autograd over the torch
restatement of tests/helpers/diff_f64.py (whose forward tests/test_host_diff.py holds against the batched oracle and whose gradients it
holds against finite differences), chaining, shared action blocks, the at-rest branch, NULL cotangents, determinism, an optimiser
through torch, and the example.  N = 70 drones (ld = 128: two waves, one ragged) unless stated otherwise.  Section 10 flies the far side
of the selects (ref.EDGE_CASES: tumbling, gimbal lock, the clamped reward, wide attitudes; 200 drones, four waves, two of them
divergent) and section 11 the sizes around a wave and a block."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import diff_f64 as ref  # noqa: E402
from diff_gpu import N, core as _core, cotangent_block, loss as _loss, padding_is_poison, set_state as _set, swept, taped  # noqa: E402
from host_lib import params as _params  # noqa: E402

pytestmark = pytest.mark.gpu


def _leaves(inp, dev):
    f = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev).requires_grad_(True)     # noqa: E731
    return [f(inp.pos), f(inp.quat), f(inp.vel), f(inp.rates)]


def device_grads(core, inp, dev, shared_action=False, with_obs=True):
    """gradients of sum(cotangent * output) through `SimCore.rollout_diff`: dict of numpy arrays by group (ref.GROUPS)"""
    from gym_pybullet_drones_amd.diff import pack_kin
    _set(core, inp)
    leaves = _leaves(inp, dev)
    a = torch.as_tensor(inp.actions[0:1] if shared_action else inp.actions, dtype=torch.float32, device=dev).requires_grad_(True)
    obs, rew, kin_k, term, trunc = core.rollout_diff(a, pack_kin(*leaves), num_steps=inp.K)
    assert not term.requires_grad and not trunc.requires_grad and obs.shape == (inp.K, inp.n, 12) and rew.shape == (inp.K, inp.n)
    grads = torch.autograd.grad(_loss(inp, dev, obs, rew, kin_k, inp.n, with_obs), [a] + leaves)
    out = {k: g.detach().cpu().numpy().astype(np.float64) for k, g in zip(ref.GROUPS, grads)}
    out["obs"] = obs.detach().cpu().numpy()
    return out


# ---- 1. the taped forward is the rollout, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["rpm", "one_d_rpm", "raw_rpm", "direct_rpm"])
@pytest.mark.parametrize("drag", [False, True])
def test_taped_forward_is_bitwise_the_rollout(gpu_device, act, drag):
    """every output and everything left behind (state, last_rpm, step_counter, bad), K in {1, 3, 20}, S in {1, 8}, task hover"""
    for S in (1, 8):
        cfg = ref.config("cf2x", act, S, drag, "hover")
        a_core, b_core = _core(cfg, gpu_device, nan_guard=True), _core(cfg, gpu_device, nan_guard=True)
        for K in (1, 3, 20):
            inp = ref.make_inputs(a_core.P, cfg, N, K, seed=K)
            acts = torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device)
            _set(a_core, inp)
            _set(b_core, inp)
            want = [t.clone() for t in a_core.rollout(acts)]
            got = b_core.rollout_diff(acts)
            for name, w, g in zip(("obs12", "reward", "terminated", "truncated"), want, (got[0], got[1], got[3], got[4])):
                assert torch.equal(w.view(g.shape), g), (name, S, K)
            assert torch.equal(got[2], b_core.kin_store)
            for name in ("kin_store", "last_rpm", "step_counter", "bad", "obs12", "reward"):
                assert torch.equal(getattr(a_core, name), getattr(b_core, name)), (name, S, K)
            assert not bool(b_core.bad.any()) and int(b_core.step_counter[0]) == K * S


def test_taped_forward_with_plant_rows_is_bitwise_the_plant_rollout(gpu_device):
    cfg, K, scales = ref.case("plant_drag_k8_s2")
    a_core, b_core = _core(cfg, gpu_device, nan_guard=True), _core(cfg, gpu_device, nan_guard=True)
    inp = ref.make_inputs(a_core.P, cfg, N, K, seed=4)
    acts = torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device)
    for core in (a_core, b_core):
        core.set_plant(torch.as_tensor(scales, dtype=torch.float32, device=gpu_device).view(9, N, 1))
        _set(core, inp)
    want = [t.clone() for t in a_core.rollout(acts)]
    got = b_core.rollout_diff(acts)
    for w, g in zip(want, (got[0], got[1], got[3], got[4])):
        assert torch.equal(w.view(g.shape), g)
    for name in ("kin_store", "last_rpm", "step_counter", "bad"):
        assert torch.equal(getattr(a_core, name), getattr(b_core, name)), name
    nominal = _core(cfg, gpu_device)
    _set(nominal, inp)
    assert not torch.equal(nominal.rollout(acts)[0], got[0])          # (the plant does something)


# ---- 2. gradients against the float64 reference -----------------------------------------------------------------------------------
#: bound per case.  The rule: 3x the largest figure the MI355X measured over the five groups, never above the project's
#: fp32 tolerance of 1e-4; the 3x covers run-to-run differences of compiler and clock.  Every case prints its figures
#: as `MEASURED <case> ...`; the largest of each is recorded here and all of them in profiles/diff_mi355x.json.
#: MEASURED on the MI355X (the group in brackets):
#:   rpm_k32_s1 5.62e-07 (quat)   rpm_k8_s8 8.54e-07 (vel)   drag_k16_s8 2.27e-05 (quat)   one_d_k5_s2 4.04e-06 (actions)
#:   raw_k3_clipped 2.00e-07 (quat)   cf2p_drag_k8_s2 3.37e-07 (actions)   racer_k8_s1 2.51e-07 (actions)   plant_drag_k8_s2 2.78e-07 (actions)
#:   shared 2.72e-07 (quat)   at_rest 5.72e-06 (actions)
FIGURES = {"rpm_k32_s1": 5.62e-07, "rpm_k8_s8": 8.54e-07, "drag_k16_s8": 2.27e-05, "one_d_k5_s2": 4.04e-06, "raw_k3_clipped": 2.00e-07, "cf2p_drag_k8_s2": 3.37e-07,
           "racer_k8_s1": 2.51e-07, "plant_drag_k8_s2": 2.78e-07,
           # sections 4 and 5
           "shared": 2.72e-07, "at_rest": 5.72e-06}
BOUND = {k: min(1e-4, 3 * v) for k, v in FIGURES.items()}


@pytest.mark.parametrize("name", list(ref.GPU_CASES))
def test_gradients_match_float64_autograd(gpu_device, name):
    """max |g32 - g64| / max |g64| for g_actions and the pos / quat / vel / rates groups of g_kin, per case of ref.GPU_CASES."""
    cfg, K, scales = ref.case(name)
    core = _core(cfg, gpu_device)
    if scales is not None:
        core.set_plant(torch.as_tensor(scales, dtype=torch.float32, device=gpu_device).view(9, N, 1))
    inp = ref.make_inputs(core.P, cfg, N, K, seed=1)
    g64 = ref.reference_grads(core.P, cfg, inp, torch.float64, scales)
    got = device_grads(core, inp, gpu_device)
    err = ref.group_errors(got, g64)
    print("MEASURED", name, " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    # the forward agrees too (what the gradients are gradients of)
    obs64 = g64["forward"][0].numpy()
    _set(core, inp)
    obs32 = core.rollout_diff(torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device))[0].cpu().numpy()
    assert np.abs(obs32 - obs64).max() < 1e-4
    assert all(np.isfinite(got[k]).all() for k in ref.GROUPS)
    assert max(err.values()) < BOUND[name], err
    if cfg.act == "raw_rpm":          # zero gradient outside the clip, exactly
        outside = (inp.actions < 0) | (inp.actions > core.P.MAX_RPM)
        assert outside.any() and not got["actions"][outside].any() and got["actions"][~outside].all()


# ---- 3. chaining -------------------------------------------------------------------------------------------------------------------
def test_three_chained_calls_give_the_bits_of_one(gpu_device):
    """K = 12 in one call and three chained calls of 4 (kin_K of one as kin0 of the next): bit-equal gradients (flags 0)"""
    from gym_pybullet_drones_amd.diff import pack_kin
    cfg = ref.config("cf2x", "rpm", 2, False, "hover")
    core = _core(cfg, gpu_device)
    inp = ref.make_inputs(core.P, cfg, N, 12, seed=6)
    one = device_grads(core, inp, gpu_device)
    _set(core, inp)
    leaves = _leaves(inp, gpu_device)
    a = torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device).requires_grad_(True)
    kin, obs, rew = pack_kin(*leaves), [], []
    for i in range(3):
        o, r, kin, _, _ = core.rollout_diff(a[4 * i:4 * i + 4], kin)
        obs.append(o)
        rew.append(r)
    grads = torch.autograd.grad(_loss(inp, gpu_device, torch.cat(obs), torch.cat(rew), kin, N), [a] + leaves)
    for k, g in zip(ref.GROUPS, grads):
        assert np.array_equal(g.cpu().numpy().astype(np.float64), one[k]), k


# ---- 4. a shared action block ------------------------------------------------------------------------------------------------------
def test_shared_action_block_gradient_is_the_sum_over_the_steps(gpu_device):
    """action_step_stride == 0, the per-step blocks summed in Python: against the reference with the same block at every step"""
    cfg = ref.config("cf2x", "rpm", 2, True, "hover")
    core = _core(cfg, gpu_device)
    inp = ref.make_inputs(core.P, cfg, N, 6, seed=7)
    g64 = ref.reference_grads(core.P, cfg, inp, torch.float64, shared_action=True)
    got = device_grads(core, inp, gpu_device, shared_action=True)
    assert got["actions"].shape == (1, N, 4)
    err = ref.group_errors(got, g64)
    print("MEASURED shared", " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    assert max(err.values()) < BOUND["shared"], err


# ---- 5. at rest --------------------------------------------------------------------------------------------------------------------
def test_at_rest_gradients_are_finite_and_match(gpu_device):
    """ONE_D_RPM from body rates exactly zero: the no-turn branch of the quaternion update"""
    cfg = ref.config("cf2x", "one_d_rpm", 2, False, "hover")
    core = _core(cfg, gpu_device)
    inp = ref.make_inputs(core.P, cfg, N, 4, seed=2, at_rest=True)
    g64 = ref.reference_grads(core.P, cfg, inp, torch.float64)
    got = device_grads(core, inp, gpu_device)
    assert float(core.body_rates().abs().max()) == 0.0               # (still exactly at rest: the branch was the no-turn one)
    assert all(np.isfinite(got[k]).all() for k in ref.GROUPS)
    err = ref.group_errors(got, g64)
    print("MEASURED at_rest", " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    assert max(err.values()) < BOUND["at_rest"], err


# ---- 6. / 7. NULL cotangents, determinism ------------------------------------------------------------------------------------------
def test_null_obs_cotangent_is_a_zero_tensor_and_two_sweeps_give_the_same_bits(gpu_device):
    cfg = ref.config("cf2x", "rpm", 8, True, "hover")
    core = _core(cfg, gpu_device)
    K = 5
    inp = ref.make_inputs(core.P, cfg, N, K, seed=8)
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=gpu_device).contiguous()     # noqa: E731
    acts, tape = taped(core, inp, K)
    g_kin0 = torch.randn(13 * core.ld, device=gpu_device)
    sweep = lambda g_obs, g_rew: swept(core, K, acts, tape, g_obs, g_rew, g_kin0)[:2]     # noqa: E731

    g_rew = T(inp.g_rew)
    null, zero = sweep(None, g_rew), sweep(torch.zeros((K, N, 12), device=gpu_device), g_rew)
    assert torch.equal(null[0], zero[0]) and torch.equal(null[1], zero[1]) and bool(torch.isfinite(null[1]).all())
    null_r, zero_r = sweep(T(inp.g_obs), None), sweep(T(inp.g_obs), torch.zeros((K, N), device=gpu_device))
    assert torch.equal(null_r[0], zero_r[0]) and torch.equal(null_r[1], zero_r[1])
    first, second = sweep(T(inp.g_obs), g_rew), sweep(T(inp.g_obs), g_rew)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert not torch.equal(first[1], null[1])                        # (the observation cotangent does something)
    assert torch.equal(first[0][4 * core.ld + 4 * N:8 * core.ld], g_kin0[4 * core.ld + 4 * N:8 * core.ld])     # rows past N untouched


# ---- 8. through torch ---------------------------------------------------------------------------------------------------------------
def test_adam_on_an_action_sequence_follows_the_float64_run(gpu_device):
    """10 Adam iterations (lr 0.1) on a K = 15, S = 8 action sequence of 64 drones from offsets of +-0.3 m and body rates +-0.1 rad/s;
    loss = mean |p - target|^2 + 0.01 mean |v|^2 over steps and drones.  The same run in the float64 restatement; at every iteration
    the loss differs from the reference's by less than a tenth of the reference's own total decrease."""
    from gym_pybullet_drones_amd.diff import pack_kin
    n, K = 64, 15
    cfg = ref.config("cf2x", "rpm", 8, False, "hover")
    core = _core(cfg, gpu_device, n=n)
    rng = np.random.default_rng(11)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)     # noqa: E731
    pos = f32(np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.3, 0.3, (n, 3)))
    quat = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))
    vel, rates = np.zeros((n, 3)), f32(rng.uniform(-0.1, 0.1, (n, 3)))
    target = np.array([0.0, 0.0, 1.0])

    def run(dtype, dev, forward):
        a = torch.zeros((K, n, 4), dtype=dtype, device=dev, requires_grad=True)
        opt = torch.optim.Adam([a], lr=0.1)
        tgt = torch.as_tensor(target, dtype=dtype, device=dev)
        losses = []
        for _ in range(10):
            opt.zero_grad()
            obs = forward(a)
            loss = ((obs[..., 0:3] - tgt) ** 2).sum(-1).mean() + 0.01 * (obs[..., 6:9] ** 2).sum(-1).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return np.array(losses)

    c = ref.consts(core.P, n)
    T64 = lambda v: torch.as_tensor(v, dtype=torch.float64)     # noqa: E731
    zero = torch.zeros(n, dtype=torch.float64)
    want = run(torch.float64, "cpu", lambda a: ref.rollout(c, cfg, (T64(pos), T64(quat), T64(vel), T64(rates)), a, zero, T64(target).expand(n, 3))[0])
    T32 = lambda v: torch.as_tensor(v, dtype=torch.float32, device=gpu_device)     # noqa: E731
    kin0 = pack_kin(T32(pos), T32(quat), T32(vel), T32(rates))
    got = run(torch.float32, gpu_device, lambda a: core.rollout_diff(a, kin0)[0])
    decrease = want[0] - want[-1]
    print("MEASURED adam f64", want[0], "->", want[-1], " max |loss32 - loss64| =", np.abs(got - want).max())
    assert decrease > 0.01
    assert np.abs(got - want).max() < 0.1 * decrease, (got, want)


def test_unsupported_configuration_raises_gpderror_with_the_librarys_message(gpu_device):
    from gym_pybullet_drones_amd import _native, engine
    core = engine.SimCore(num_envs=8, drones_per_env=1, act_code=1, task=engine.TASK_HOVER, target_pos=[[0.0, 0.0, 1.0]], device=gpu_device)
    before = core.kin_store.clone()
    with pytest.raises(_native.GpdError, match="gpd_rollout_tape_floats: the DSLPID action types are not differentiable"):
        core.rollout_diff(torch.zeros((2, 8, 3), device=gpu_device))
    assert torch.equal(before, core.kin_store)
    two = engine.SimCore(num_envs=4, drones_per_env=2, device=gpu_device)
    with pytest.raises(_native.GpdError, match="drones_per_env"):
        two.rollout_diff(torch.zeros((2, 8, 4), device=gpu_device))


def test_vector_aviary_rollout_diff_backpropagates(gpu_device):
    from gym_pybullet_drones_amd.envs import VectorHoverAviary
    from gym_pybullet_drones_amd.utils.enums import ActionType
    env = VectorHoverAviary(N, act=ActionType.RPM, ctrl_freq=30, auto_reset=False, device=gpu_device)
    env.reset()
    a = torch.zeros((4, N, 1, 4), device=gpu_device, requires_grad=True)
    obs, rew, kin_k, term, trunc = env.rollout_diff(a)
    assert obs.shape == (4, N, 1, 12) and rew.shape == (4, N) and kin_k.shape == (13 * env.core.ld,) and term.dtype == torch.bool
    rew.sum().backward()
    # the drones start below the target: more thrust on every rotor raises the reward
    assert a.grad.shape == a.shape and bool((a.grad > 0).all())


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------
def test_example_apg_losses_fall(gpu_device):
    spec = importlib.util.spec_from_file_location("example_apg", os.path.join(REPO, "examples", "apg.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    traj, policy = m.run(num_envs=64, traj_iters=15, policy_iters=15, horizon=15, device=gpu_device, verbose=False)
    # (half a second at +-5 % rpm moves a drone a few centimetres: the float32 restatement on the CPU gives 0.0985 -> 0.0849 for the
    # sequences and 0.1010 -> 0.0887 for the policy at this size; both must have fallen by at least 5 %)
    assert traj[-1] < 0.95 * traj[0] and policy[-1] < 0.95 * policy[0], (traj, policy)
    assert all(b < a for a, b in zip(traj, traj[1:]))


# ---- 10. the far side of the selects -------------------------------------------------------------------------------------------------
# tests/test_host_diff.py establishes the conditions of every kind on the CPU: which lanes sit on the far side at every step and
# sub-step and with what margin, that every other lane keeps the margins of the cases above, and that the float32 restatement stays
# within 1e-5 of the float64 one -- so that a device gradient within the bound is a statement about the kernel.
#: MEASURED on the MI355X, the largest of the five groups of each kind (the group in brackets; beside it the forward obs12 against the
#: float64 run relative to each column's scale, `ref.forward_error`), the bound the rule of section 2:
#:   tumble 1.58e-06 (actions; forward 2.58e-06)   gimbal 1.64e-06 (actions; forward 1.97e-07)   near_gimbal 2.46e-06 (quat; forward 3.94e-07)
#:   reward_far 2.51e-07 (actions; forward 2.09e-07)   wide_attitude 2.01e-06 (quat; forward 8.11e-07)   gimbal_yaw_only 1.56e-07 (rates)
#:   tumble_plant 2.86e-06 (mass; forward 7.94e-07)
EDGE_FIGURES = {"tumble": 1.58e-06, "gimbal": 1.64e-06, "near_gimbal": 2.46e-06, "reward_far": 2.51e-07, "wide_attitude": 2.01e-06,
                # the yaw cotangent alone on the gimbal inputs; `tumble` with the plant scales as leaves (the scales' own groups included)
                "gimbal_yaw_only": 1.56e-07, "tumble_plant": 2.86e-06}
EDGE_BOUND = {k: min(1e-4, 3 * v) for k, v in EDGE_FIGURES.items()}
EDGE_N = ref.EDGE_N


@functools.lru_cache(maxsize=None)
def _edge(kind):
    """an edge case's (cfg, K, inputs, float64 gradients): computed once, shared by the tests of this section, never written to"""
    cfg, K = ref.edge_case(kind)
    C = _params(cfg.model)
    inp = ref.make_edge_inputs(C, cfg, EDGE_N, K, kind)
    return cfg, K, inp, ref.reference_grads(C, cfg, inp, torch.float64)


def _measured(name, err, forward=None):
    print("MEASURED", name, " ".join(f"{k}={v:.2e}" for k, v in err.items()) + ("" if forward is None else f" forward_obs12_rel={forward:.2e}"))


@pytest.mark.parametrize("kind", list(ref.EDGE_CASES))
def test_edge_gradients_match_float64_autograd(gpu_device, kind):
    """the metric of section 2 with the rare lanes (every third drone of waves 0 and 1) on the far side of the kind's select; the
    forward obs12 against the float64 run relative to each column's scale (a tumbling drone's angular velocity reaches 1700 rad/s)"""
    cfg, K, inp, g64 = _edge(kind)
    core = _core(cfg, gpu_device, n=EDGE_N)
    assert core.ld == 256
    got = device_grads(core, inp, gpu_device)
    err = ref.group_errors(got, g64)
    forward = ref.forward_error(got["obs"], g64["forward"][0].numpy())
    _measured(kind, err, forward)
    assert forward < 1e-4
    assert all(np.isfinite(got[k]).all() for k in ref.GROUPS)
    assert max(err.values()) < EDGE_BOUND[kind], err
    # ... and on the rare lanes alone, which a larger gradient elsewhere must not hide: the same metric over those lanes
    rare = {k: (v[:, inp.rare] if k == "actions" else v[inp.rare]) for k, v in got.items() if k in ref.GROUPS}
    rare64 = {k: (g64[k][:, inp.rare] if k == "actions" else g64[k][inp.rare]) for k in ref.GROUPS}
    err_rare = ref.group_errors(rare, rare64)
    _measured(kind + "_rare_lanes", err_rare)
    assert max(err_rare.values()) < EDGE_BOUND[kind], err_rare


@pytest.mark.parametrize("kind", list(ref.EDGE_CASES))
def test_edge_taped_forward_is_bitwise_the_rollout(gpu_device, kind):
    """as section 1, on the inputs of every edge kind at its own K: every output and everything left behind"""
    cfg, K, inp, _ = _edge(kind)
    a_core, b_core = _core(cfg, gpu_device, n=EDGE_N, nan_guard=True), _core(cfg, gpu_device, n=EDGE_N, nan_guard=True)
    acts = torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device)
    _set(a_core, inp)
    _set(b_core, inp)
    want = [t.clone() for t in a_core.rollout(acts)]
    got = b_core.rollout_diff(acts)
    for name, w, g in zip(("obs12", "reward", "terminated", "truncated"), want, (got[0], got[1], got[3], got[4])):
        assert torch.equal(w.view(g.shape), g), name
    assert torch.equal(got[2], b_core.kin_store)
    for name in ("kin_store", "last_rpm", "step_counter", "bad", "obs12", "reward"):
        assert torch.equal(getattr(a_core, name), getattr(b_core, name)), name
    assert not bool(b_core.bad.any()) and int(b_core.step_counter[0]) == K * cfg.S
    rare = torch.as_tensor(inp.rare, device=gpu_device)
    if kind == "gimbal":          # (the device took the branch too: roll exactly 0 and pitch exactly +-pi/2 on the rare lanes, nowhere else)
        on = (got[0][..., 3] == 0.0) & (got[0][..., 4].abs() == float(np.float32(0.5 * np.pi)))
        assert bool((on == rare).all())
    if kind == "reward_far":
        assert bool(((got[1] == 0.0) == rare).all())


def _unpacked(core, g_kin, g_act):
    from gym_pybullet_drones_amd.diff import unpack_kin
    out = {k: v.cpu().numpy().astype(np.float64) for k, v in zip(ref.GROUPS[1:], unpack_kin(g_kin, core.N))}
    out["actions"] = g_act.cpu().numpy().astype(np.float64)
    return out


def test_far_lanes_get_exact_zeros_from_the_reward_cotangent(gpu_device):
    """`reward_far`, the raw entries: g_reward alone (g_obs NULL, g_kin0 zero).  A lane beyond the clamp at all K steps has every
    gradient exactly 0.0; every near lane has a gradient; the rows past N of g_kin keep their poison."""
    cfg, K, inp, _ = _edge("reward_far")
    core = _core(cfg, gpu_device, n=EDGE_N)
    acts, tape, _, rew = taped(core, inp, K, with_outputs=True)
    far = inp.rare
    assert bool(((rew == 0.0).cpu().numpy() == far).all())
    g_kin, g_act, _ = swept(core, K, acts, tape, None, torch.as_tensor(inp.g_rew, dtype=torch.float32, device=gpu_device).contiguous(),
                            cotangent_block(core))
    assert padding_is_poison(core, g_kin)
    got = _unpacked(core, g_kin, g_act)
    assert all(np.isfinite(v).all() for v in got.values())
    for k, v in got.items():
        v = v[:, far] if k == "actions" else v[far]
        assert not v.any(), k                                         # (exactly zero: no NaN either, NaN != 0)
    assert got["pos"][~far].any(axis=1).all() and got["actions"][:, ~far].any(axis=(0, 2)).all() and got["quat"][~far].any(axis=1).all()


def _sparse_errors(got, want, full):
    """`ref.group_errors` for a run whose cotangents are a subset of the case's: a group whose float64 gradient is zero under them
    (nothing, or the rounding of terms that cancel: below 1e-9 of the group's scale `full` under the case's full cotangents) is held
    absolutely, against that scale"""
    err = {}
    for k in ref.GROUPS:
        scale, top = float(np.abs(full[k]).max()), float(np.abs(want[k]).max())
        err[k] = float(np.abs(got[k] - want[k]).max() / (top if top > 1e-9 * scale else scale))
    return err


def test_gimbal_lanes_discard_the_regular_branch(gpu_device):
    """`gimbal`, the raw entries, g_kin0 zero and g_reward NULL.  On a gimbal lane roll and pitch are constants and the regular branch
    of rpy_vjp is rsq of (1 - s)(1 + s) at s = 1 to rounding -- inf, or NaN where s > 1 -- times the pitch cotangent.
    (a) cotangents on the roll and pitch columns alone: the gimbal lanes get exactly 0.0 everywhere, no NaN (the select discards
        0 * inf); the ordinary lanes a finite gradient.
    (b) the yaw cotangent alone: the gimbal lanes' g_quat has z and w exactly 0 (yaw = 2 atan2(+-x, -+y) there, and a lane at rest
        passes the quaternion's cotangent through every sub-step), x and y not; the whole gradient against float64."""
    cfg, K, inp, g64_full = _edge("gimbal")
    core = _core(cfg, gpu_device, n=EDGE_N)
    C = _params(cfg.model)
    acts, tape, obs, _ = taped(core, inp, K, with_outputs=True)
    gim = inp.rare
    on = ((obs[..., 3] == 0.0) & (obs[..., 4].abs() == float(np.float32(0.5 * np.pi)))).cpu().numpy()
    assert (on == gim).all()
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=gpu_device).contiguous()     # noqa: E731
    # (a)
    g_obs = np.zeros_like(inp.g_obs)
    g_obs[..., 3:5] = inp.g_obs[..., 3:5]
    g_kin, g_act, _ = swept(core, K, acts, tape, T(g_obs), None, cotangent_block(core))
    assert padding_is_poison(core, g_kin)
    got = _unpacked(core, g_kin, g_act)
    assert all(np.isfinite(v).all() for v in got.values())
    for k, v in got.items():
        assert not (v[:, gim] if k == "actions" else v[gim]).any(), k
    assert got["quat"][~gim].any(axis=1).all() and got["rates"][~gim].any(axis=1).all()
    # (b)
    g_obs = np.zeros_like(inp.g_obs)
    g_obs[..., 5] = inp.g_obs[..., 5]
    g_kin, g_act, _ = swept(core, K, acts, tape, T(g_obs), None, cotangent_block(core))
    assert padding_is_poison(core, g_kin)
    got = _unpacked(core, g_kin, g_act)
    assert all(np.isfinite(v).all() for v in got.values())
    assert not got["quat"][gim, 2:4].any() and got["quat"][gim, 0:2].all()
    g64 = ref.reference_grads(C, cfg, ref.with_cotangents(inp, g_obs=g_obs), torch.float64)
    err = _sparse_errors(got, g64, g64_full)
    _measured("gimbal_yaw_only", err)
    assert max(err.values()) < EDGE_BOUND["gimbal_yaw_only"], err


def test_tumbling_through_the_plant_sweep_matches_float64_autograd(gpu_device):
    """`tumble` through gpd_rollout_vjp_plant (another instantiation of the sweep: it also sums the cotangents of J and J_INV from the
    same torques and rate cotangents) with the scales as leaves, the first step of the case (ref.TUMBLE_PLANT_K): the five groups
    and every scale the configuration reads"""
    import sysid_f64 as sid
    cfg, _, inp, _ = _edge("tumble")
    inp = ref.first_steps(inp, ref.TUMBLE_PLANT_K)
    core = _core(cfg, gpu_device, n=EDGE_N)
    scales = ref.edge_scales(EDGE_N)
    g64 = ref.reference_grads(core.P, cfg, inp, torch.float64, scales, wrt_scales=True)
    from gym_pybullet_drones_amd.diff import pack_kin
    _set(core, inp)
    leaves = _leaves(inp, gpu_device)
    a = torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device).requires_grad_(True)
    s = torch.as_tensor(scales, dtype=torch.float32, device=gpu_device).requires_grad_(True)
    obs, rew, kin_k, _, _ = core.rollout_diff(a, pack_kin(*leaves), plant_scales=s)
    grads = torch.autograd.grad(_loss(inp, gpu_device, obs, rew, kin_k, inp.n), [a] + leaves + [s])
    got = {k: g.detach().cpu().numpy().astype(np.float64) for k, g in zip(ref.GROUPS + ("scales",), grads)}
    err = dict(ref.group_errors(got, g64), **sid.scale_errors(got["scales"], g64["scales"]))
    _measured("tumble_plant", err, ref.forward_error(obs.detach().cpu().numpy(), g64["forward"][0].numpy()))
    assert all(np.isfinite(v).all() for v in got.values())
    assert set(err) == set(ref.GROUPS) | {"mass", "ixx", "iyy", "izz", "kf", "km"}
    assert max(err.values()) < EDGE_BOUND["tumble_plant"], err


# ---- 11. sizes ------------------------------------------------------------------------------------------------------------------------
def _block_size():
    """the kernels' block size (csrc/gpd_common.inc GPD_BLOCK)"""
    import re
    from gym_pybullet_drones_amd import _native
    return int(re.search(r"^#define GPD_BLOCK (\d+)$", open(os.path.join(_native.CSRC, "gpd_common.inc")).read(), flags=re.M).group(1))


#: MEASURED on the MI355X, the largest of the five groups at each N (the bound: the rule of section 2):
#:   N = 1: 6.59e-07 (vel)   N = 64: 2.27e-07 (actions)   N = 65: 1.93e-07 (actions)   N = 257: 2.95e-07 (quat)
SIZE_FIGURES = {1: 6.59e-07, 64: 2.27e-07, 65: 1.93e-07, 257: 2.95e-07}


@pytest.mark.parametrize("n", ["1", "64", "65", "block+1"])
def test_sizes_around_a_wave_and_a_block(gpu_device, n):
    """one ordinary case (RPM, S = 2, K = 4, drag) at N = 1, a full wave, a wave and a lane, a block and a lane -- the raw entries into
    poisoned outputs: the gradients against float64, the rows N .. ld-1 of g_kin untouched, g_act written in full"""
    n = _block_size() + 1 if n == "block+1" else int(n)
    assert n in SIZE_FIGURES
    cfg, K = ref.config("cf2x", "rpm", 2, True, "hover"), 4
    core = _core(cfg, gpu_device, n=n)
    assert core.ld == (n + 63) // 64 * 64
    inp = ref.make_inputs(core.P, cfg, n, K, seed=1)
    g64 = ref.reference_grads(core.P, cfg, inp, torch.float64)
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=gpu_device).contiguous()     # noqa: E731
    acts, tape, obs, _ = taped(core, inp, K, with_outputs=True)
    g_kin, g_act, _ = swept(core, K, acts, tape, T(inp.g_obs), T(inp.g_rew), cotangent_block(core, (inp.g_pos, inp.g_quat, inp.g_vel, inp.g_rates)))
    assert padding_is_poison(core, g_kin)
    assert g_act.shape == (K, n, 4) and bool(torch.isfinite(g_act).all()) and bool(g_act.any(dim=2).all())
    got = _unpacked(core, g_kin, g_act)
    err = ref.group_errors(got, g64)
    _measured(f"size_{n}", err, ref.forward_error(obs.cpu().numpy(), g64["forward"][0].numpy()))
    assert np.abs(obs.cpu().numpy() - g64["forward"][0].numpy()).max() < 1e-4
    assert max(err.values()) < min(1e-4, 3 * SIZE_FIGURES[n]), err

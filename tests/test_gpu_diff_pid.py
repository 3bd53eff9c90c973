"""The differentiable rollout through the DSLPID loop on the device (include/gpd.h `gpd_rollout_tape_pid` / `gpd_rollout_vjp_pid`,
gym_pybullet_drones_amd/diff.py): the taped forward against `gpd_rollout` bit for bit, the reverse sweep against float64 autograd over the
torch restatement of tests/helpers/diff_pid_f64.py (whose forward tests/test_host_diff_pid.py holds against the batched oracle, whose
gradients it holds against finite differences, and whose float32 run it holds against its float64 run on these inputs), the exact zeros
of saturated rotors, of a zero direction and of drones beyond the reward clamp, the sizes around a wave, chaining through `kin_K` / `pid_K`, shared action blocks, the gains flag, the surface, and
examples/tune_pid.py.  N = 70 drones (ld = 128: two waves, one ragged) unless stated otherwise."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import diff_f64 as ref  # noqa: E402
import diff_pid_f64 as pref  # noqa: E402

pytestmark = pytest.mark.gpu
N = 70


def _core(cfg, dev, n=N, nan_guard=False, physics=0, act_code=None):
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    pyb_freq = round(1.0 / cfg.h)
    return engine.SimCore(drone_model=getattr(DroneModel, ref.MODELS[cfg.model]), num_envs=n, drones_per_env=1, physics=physics, pyb_freq=pyb_freq,
                          ctrl_freq=pyb_freq // cfg.S, act_code=pref.ACT_CODE[cfg.act] if act_code is None else act_code, task=engine.TASK_HOVER,
                          target_pos=[[0.0, 0.0, 1.0]], auto_reset=False, track_rpm=True, nan_guard=nan_guard, device=dev)


def _set(core, inp):
    """the inputs' state into the core: the logical [13, n] rows, the nine members, no RPMs carried in"""
    kin = np.concatenate([inp.pos, inp.quat, inp.vel, inp.rates], axis=1).T
    state = dict(kin=torch.as_tensor(kin, dtype=torch.float32), last_rpm=torch.zeros((4, inp.n)), step_counter=torch.zeros(core.E, dtype=torch.int32))
    if core.pid is not None:
        state["pid"] = torch.as_tensor(np.concatenate([inp.int_pos, inp.last_rpy, inp.int_rpy], axis=1).T, dtype=torch.float32)
    core.set_state(**state)


def _leaves(inp, dev):
    f = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev).requires_grad_(True)     # noqa: E731
    return [f(v) for v in (inp.pos, inp.quat, inp.vel, inp.rates, inp.int_pos, inp.last_rpy, inp.int_rpy)]


def _loss(inp, dev, obs, rew, kin_k, pid_k, with_members=True):
    from gym_pybullet_drones_amd.diff import unpack_kin, unpack_pid
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev)     # noqa: E731
    if with_members:
        return pref.loss_of(inp, T, obs, rew, unpack_kin(kin_k, inp.n), unpack_pid(pid_k, inp.n))
    return (T(inp.g_rew) * rew).sum() + (T(inp.g_obs) * obs).sum() + sum(
        (T(g) * k).sum() for g, k in zip((inp.g_pos, inp.g_quat, inp.g_vel, inp.g_rates), unpack_kin(kin_k, inp.n)))


def _own_gains(core):
    from gym_pybullet_drones_amd import diff
    return diff.gains_of(core._params)


def device_grads(core, inp, dev, shared_action=False, gains="own", chunks=1):
    """gradients of `pref.loss_of` through `SimCore.rollout_diff_pid` (in `chunks` chained calls): dict of numpy arrays by group"""
    from gym_pybullet_drones_amd.diff import pack_kin, pack_pid
    _set(core, inp)
    leaves = _leaves(inp, dev)
    a = torch.as_tensor(inp.actions[0:1] if shared_action else inp.actions, dtype=torch.float32, device=dev).requires_grad_(True)
    g = None if gains is None else _own_gains(core).requires_grad_(True)
    kin, pid, obs, rew, per = pack_kin(*leaves[:4]), pack_pid(*leaves[4:]), [], [], inp.K // chunks
    for i in range(chunks):
        block = a if shared_action else a[per * i:per * (i + 1)]
        o, r, kin, pid, term, trunc = core.rollout_diff_pid(block, kin, pid, num_steps=per, pid_gains=g)
        assert not term.requires_grad and not trunc.requires_grad and o.shape == (per, inp.n, 12) and r.shape == (per, inp.n)
        obs.append(o)
        rew.append(r)
    obs, rew = torch.cat(obs), torch.cat(rew)
    grads = torch.autograd.grad(_loss(inp, dev, obs, rew, kin, pid), [a] + leaves + ([] if g is None else [g]))
    out = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in zip(pref.GROUPS[:8], grads)}
    if g is not None:
        out.update({name: grads[8][i].detach().cpu().numpy().astype(np.float64) for i, name in enumerate(pref.GAINS)})
    out["forward"] = (obs.detach(), rew.detach(), kin.detach(), pid.detach())
    return out


# ---- 1. the taped forward is the rollout, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["pid", "vel", "one_d_pid"])
def test_taped_forward_is_bitwise_the_rollout(gpu_device, act):
    """every output and everything left behind (state, members, last_rpm, step_counter, bad), S in {5, 8}, K in {1, 3, 12}"""
    for S in (5, 8):
        cfg = ref.config("cf2x", act, S, False, "hover")
        a_core, b_core = _core(cfg, gpu_device, nan_guard=True), _core(cfg, gpu_device, nan_guard=True)
        for K in (1, 3, 12):
            inp = pref.make_inputs(a_core.P, cfg, N, K, seed=K)
            acts = torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device)
            _set(a_core, inp)
            _set(b_core, inp)
            want = [t.clone() for t in a_core.rollout(acts)]
            got = b_core.rollout_diff_pid(acts)
            for name, w, g in zip(("obs12", "reward", "terminated", "truncated"), want, (got[0], got[1], got[4], got[5])):
                assert torch.equal(w.view(g.shape), g), (name, S, K)
            assert torch.equal(got[2], b_core.kin_store) and torch.equal(got[3], b_core.pid)
            for name in ("kin_store", "pid", "last_rpm", "step_counter", "bad", "obs12", "reward"):
                assert torch.equal(getattr(a_core, name), getattr(b_core, name)), (name, S, K)
            assert not bool(b_core.bad.any()) and int(b_core.step_counter[0]) == K * S
            assert bool(b_core.pid[:, :N].abs().sum(dim=1).min() > 0) and bool(b_core.last_rpm[:, :N].min() > 0)


# ---- 2. gradients against the float64 reference -----------------------------------------------------------------------------------
#: bound per case.  The rule written at the top of section 2 of tests/test_gpu_diff.py: 3x the largest figure the MI355X measured over
#: the groups, never above the project's fp32 tolerance of 1e-4.  1e-4 is ten times the conditioning rule the inputs meet on the CPU
#: (tests/test_host_diff_pid.py): the room the polynomial atan2 / asin and the 1-ulp reciprocal square roots need over a plain float32 run.
#: MEASURED on the MI355X, the largest of the 14 groups of each case (the group in brackets; the forward obs12 against the float64 run, absolute,
#: beside it -- the observed angular velocity, which carries the rounding of the Euler-angle difference times d_tor x the control rate):
#:   vel_k8_s5 1.53e-06 (d_tor; forward 2.97e-05)      pid_k8_s5 3.23e-05 (d_tor; 2.61e-05)         one_d_k6_s8 8.52e-06 (d_tor; 6.83e-05)
#:   cf2p_vel_k6_s5 3.41e-06 (d_tor; 9.11e-06)         sat_int_k10_s5 9.51e-06 (int_rpy; 9.29e-05)  sat_pwm_k4_s5 1.14e-06 (int_pos; 1.06e-05)
#: the shared action block (section 5): 2.54e-06 (d_tor).  3x each figure, never above 1e-4:
#: far_vel_k4_s5 (every other drone beyond the reward clamp): 2.37e-06 (d_tor; forward 5.51e-06)
FIGURES = {"vel_k8_s5": 1.53e-06, "pid_k8_s5": 3.23e-05, "one_d_k6_s8": 8.52e-06, "cf2p_vel_k6_s5": 3.41e-06, "sat_int_k10_s5": 9.51e-06,
           "sat_pwm_k4_s5": 1.14e-06, "far_vel_k4_s5": 2.37e-06, "shared_vel_k8_s5": 2.54e-06}
BOUND = {k: min(1e-4, 3 * v) for k, v in FIGURES.items()}


@pytest.mark.parametrize("name", list(pref.GPU_CASES))
def test_gradients_match_float64_autograd(gpu_device, name):
    """max |g32 - g64| / max |g64| for g_actions, the pos / quat / vel / rates groups of g_kin, the three groups of g_pid and the six
    gain vectors, per case of pref.GPU_CASES; the forward obs12 within 1e-4 of the float64 run."""
    cfg, K, kind, seed = pref.case(name)
    core = _core(cfg, gpu_device)
    inp = pref.make_inputs(core.P, cfg, N, K, seed=seed, kind=kind)
    g64 = pref.reference_grads(core.P, cfg, inp, torch.float64, gains=_own_gains(core).double().numpy())
    got = device_grads(core, inp, gpu_device)
    err = pref.group_errors(got, g64)
    print("MEASURED", name, " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    obs32 = got["forward"][0].cpu().numpy()
    print("MEASURED", name, f"forward_obs12={np.abs(obs32 - g64['forward'][0].numpy()).max():.2e}")
    assert np.abs(obs32 - g64["forward"][0].numpy()).max() < 1e-4
    assert all(np.isfinite(got[k]).all() for k in pref.GROUPS)
    assert max(err.values()) < BOUND[name], err


# ---- 3. exact zeros ---------------------------------------------------------------------------------------------------------------
def test_saturated_rotors_and_a_zero_direction_give_exact_zeros(gpu_device):
    """K = 1, VEL.  Every other drone falls at 3 m/s and is told to climb: the thrust the velocity error asks for puts all four PWMs at
    MAX_PWM whatever the torques add, so nothing reaches the rotors from the controller -- g_actions is exactly zero and g_kin is what
    the physics alone gives, bit for bit the sweep of a DIRECT_RPM core flown with those RPMs.  A row whose direction a_xyz is zero
    has an exactly zero gradient towards it."""
    from gym_pybullet_drones_amd.diff import pack_kin, pack_pid
    cfg = ref.config("cf2x", "vel", 5, False, "hover")
    core = _core(cfg, gpu_device)
    inp = pref.make_inputs(core.P, cfg, N, 1, seed=11)
    falling = np.arange(N) % 2 == 0
    inp.vel[falling, 2] = -3.0
    inp.actions[0, falling] = np.array([0.0, 0.0, 1.0, 1.0])
    still = np.arange(N) % 7 == 3                                   # (odd and even drones among them)
    inp.actions[0, still, 0:3] = 0.0
    _set(core, inp)
    leaves = _leaves(inp, gpu_device)
    a = torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device).requires_grad_(True)
    kin0 = pack_kin(*leaves[:4]).detach().requires_grad_(True)
    obs, rew, kin_k, pid_k, _, _ = core.rollout_diff_pid(a, kin0, pack_pid(*leaves[4:]))
    g_a, g_kin = torch.autograd.grad(_loss(inp, gpu_device, obs, rew, kin_k, pid_k, with_members=False), [a, kin0])
    # (rpm = fmaf(scale, pwm, const) at pwm = MAX_PWM: the product exactly, one rounding)
    max_rpm = np.float32(float(core._params.pwm2rpm_scale) * float(core._params.max_pwm) + float(core._params.pwm2rpm_const))
    rpm = core.last_rpm[:, :N].t().contiguous()
    clipped = (rpm == float(max_rpm)).all(dim=1).cpu().numpy()
    assert clipped[falling].all() and not clipped[~falling].any()
    g_a = g_a.cpu().numpy()
    assert not g_a[0, clipped].any() and np.isfinite(g_a).all()
    assert not g_a[0, still, 0:3].any() and g_a[0, ~still & ~clipped, 0:3].any(axis=1).all()
    # the physics alone: the same state and cotangents through the RPM entries, flown with the RPMs the controller commanded
    rpm_cfg = ref.config("cf2x", "direct_rpm", 5, False, "hover")
    rpm_core = _core(rpm_cfg, gpu_device, act_code=ref.ACT_CODE["direct_rpm"])
    _set(rpm_core, inp)
    kin0_b = kin0.detach().clone().requires_grad_(True)
    obs_b, rew_b, kin_b, _, _ = rpm_core.rollout_diff(rpm.view(1, N, 4), kin0_b)
    assert torch.equal(obs_b, obs) and torch.equal(kin_b, kin_k)
    g_kin_b, = torch.autograd.grad(_loss(inp, gpu_device, obs_b, rew_b, kin_b, None, with_members=False), [kin0_b])
    from gym_pybullet_drones_amd.diff import unpack_kin
    for name, got, want in zip(pref.KIN_GROUPS, unpack_kin(g_kin, N), unpack_kin(g_kin_b, N)):
        got, want = got.cpu().numpy(), want.cpu().numpy()
        assert np.array_equal(got[clipped], want[clipped]), name
        # elsewhere the controller does contribute -- through the attitude and the velocity it reads (under VEL the target position is
        # the position, so the position error does not depend on it, and the controller never reads the body rates)
        assert np.array_equal(got[~clipped], want[~clipped]) == (name in ("pos", "rates")), name


def _raw_sweep(core, inp, K, g_obs, g_rew, cot=None):
    """the raw entries outside autograd: the inputs' state, one taped forward, one sweep into poisoned outputs -- g_kin0 / g_pid0 the
    cotangents `cot` = (pos, quat, vel, rates, int_pos, last_rpy, int_rpy) or zeros for drones 0 .. N-1 and 7.0 past them, NaN for
    g_act, 7.0 for g_gains: (reward, g_kin, g_pid, g_act, g_gains)"""
    from gym_pybullet_drones_amd import diff
    from diff_gpu import cotangent_block
    dev, n, ld = core.device, core.N, core.ld
    _set(core, inp)
    acts = torch.as_tensor(inp.actions, dtype=torch.float32, device=dev).contiguous()
    tape = torch.empty(diff.tape_floats_pid(core, K), dtype=torch.float32, device=dev)
    obs, rew = torch.empty((K, n, 12), device=dev), torch.empty((K, n), device=dev)
    flags = torch.empty((2, K, n), dtype=torch.bool, device=dev)
    diff.tape_forward_pid(core, core._params, K, acts, n * inp.A, obs, rew, flags[0], flags[1], tape)
    T = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.float32, device=dev).contiguous()     # noqa: E731
    g_kin = cotangent_block(core, None if cot is None else cot[:4])
    g_pid = torch.full((9, ld), 7.0, device=dev)
    g_pid[:, :n] = 0.0 if cot is None else torch.as_tensor(np.concatenate(cot[4:], axis=1).T, dtype=torch.float32, device=dev)
    g_act, g_gains = torch.full((K, n, inp.A), float("nan"), device=dev), torch.full((18, ld), 7.0, device=dev)
    diff.sweep_pid(core, core._params, K, acts, n * inp.A, tape, T(g_obs), T(g_rew), g_kin, g_pid, g_act, g_gains)
    return rew, g_kin, g_pid, g_act, g_gains


def test_drones_beyond_the_reward_clamp_get_exact_zeros_from_the_reward_cotangent(gpu_device):
    """far_vel_k4_s5, g_reward alone (g_obs NULL, g_kin0 and g_pid0 zero): a drone beyond the clamp at all K steps -- every other one,
    tests/test_host_diff_pid.py -- has exactly 0.0 in g_actions, g_kin, g_pid and its column of g_gains; every other drone has a
    gradient; nothing past drone N - 1 is written"""
    from gym_pybullet_drones_amd.diff import unpack_kin
    from diff_gpu import padding_is_poison
    cfg, K, kind, seed = pref.case("far_vel_k4_s5")
    core = _core(cfg, gpu_device)
    inp = pref.make_inputs(core.P, cfg, N, K, seed=seed, kind=kind)
    rew, g_kin, g_pid, g_act, g_gains = _raw_sweep(core, inp, K, None, inp.g_rew)
    far = np.arange(N) % 2 == 0
    assert ((rew == 0.0).cpu().numpy() == far).all()
    assert padding_is_poison(core, g_kin) and bool((g_pid[:, N:] == 7.0).all()) and bool((g_gains[:, N:] == 7.0).all())
    parts = [p.cpu().numpy() for p in unpack_kin(g_kin, N)] + [g_pid[:, :N].t().cpu().numpy(), g_gains[:, :N].t().cpu().numpy(),
                                                               g_act.cpu().numpy().transpose(1, 0, 2).reshape(N, -1)]
    assert all(np.isfinite(p).all() for p in parts)
    for p in parts:
        assert not p[far].any()                                       # (exactly zero; a NaN is not)
    for p in (parts[0], parts[2], parts[4], parts[6]):                # pos, vel, the members, the actions
        assert p[~far].any(axis=1).all()


# ---- 3b. sizes ------------------------------------------------------------------------------------------------------------------------
#: MEASURED on the MI355X, the largest of the 14 groups of "vel_k8_s5" at each N (the bound: the rule of section 2):
#:   N = 1: 4.27e-06 (last_rpy)   N = 64: 1.90e-06 (i_tor)   N = 65: 1.73e-06 (d_tor)
SIZE_FIGURES = {1: 4.27e-06, 64: 1.90e-06, 65: 1.73e-06}


@pytest.mark.parametrize("n", sorted(pref.SIZE_SEEDS))
def test_sizes_around_a_wave(gpu_device, n):
    """"vel_k8_s5" at N = 1, a full wave, a wave and a lane (the seeds of pref.SIZE_SEEDS, which tests/test_host_diff_pid.py holds to
    the two rules) through the raw entries into poisoned outputs: every group against float64 -- the gains' gradient as the float64
    sum of the lanes' columns --, nothing past drone N - 1 written, g_act written in full"""
    from gym_pybullet_drones_amd.diff import unpack_kin
    from diff_gpu import padding_is_poison
    cfg, K, kind, _ = pref.case("vel_k8_s5")
    core = _core(cfg, gpu_device, n=n)
    assert core.ld == (n + 63) // 64 * 64
    inp = pref.make_inputs(core.P, cfg, n, K, seed=pref.SIZE_SEEDS[n], kind=kind)
    g64 = pref.reference_grads(core.P, cfg, inp, torch.float64, gains=_own_gains(core).double().numpy())
    cot = (inp.g_pos, inp.g_quat, inp.g_vel, inp.g_rates, inp.g_int_pos, inp.g_last_rpy, inp.g_int_rpy)
    _, g_kin, g_pid, g_act, g_gains = _raw_sweep(core, inp, K, inp.g_obs, inp.g_rew, cot)
    assert padding_is_poison(core, g_kin) and bool((g_pid[:, n:] == 7.0).all()) and bool((g_gains[:, n:] == 7.0).all())
    assert bool(torch.isfinite(g_act).all()) and bool(g_act.any(dim=2).all())
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in zip(pref.KIN_GROUPS, unpack_kin(g_kin, n))}
    got.update({k: g_pid[3 * i:3 * i + 3, :n].t().cpu().numpy().astype(np.float64) for i, k in enumerate(pref.PID_GROUPS)})
    got["actions"] = g_act.cpu().numpy().astype(np.float64)
    got.update({k: g_gains[3 * i:3 * i + 3, :n].double().sum(dim=1).cpu().numpy() for i, k in enumerate(pref.GAINS)})
    err = pref.group_errors(got, g64)
    print("MEASURED", f"size_{n}", " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    assert max(err.values()) < min(1e-4, 3 * SIZE_FIGURES[n]), err


# ---- 4. chaining -------------------------------------------------------------------------------------------------------------------
CHAINED_GAINS_FIGURE = 1.07e-07          # the largest of the six measured figures below


def test_three_chained_calls_give_the_bits_of_one(gpu_device):
    """K = 12 in one call and three chained calls of 4 (kin_K / pid_K of one as kin0 / pid0 of the next): bit-equal gradients for the
    actions and every group of the initial state and members -- each of their words has one writer and the cotangents cross the call
    boundary as the float32 values the registers held.  The gains' gradient cannot be the same bits: it is a SUM over steps and drones
    that the lane takes in registers over the whole sweep (include/gpd.h), and three chained calls return three float32 sums of four
    steps each, which autograd adds -- the same terms in another order.  It is held to 3x what the MI355X measured, relative to the
    vector's largest entry (the rule of section 2).  MEASURED: p_for 3.20e-08, i_for 1.07e-07, d_for 6.73e-08, p_tor 6.66e-09,
    i_tor 8.11e-08, d_tor 7.48e-08 -- one or two units in the last place of a float32."""
    cfg = ref.config("cf2x", "pid", 5, False, "hover")
    core = _core(cfg, gpu_device)
    inp = pref.make_inputs(core.P, cfg, N, 12, seed=6)
    one = device_grads(core, inp, gpu_device)
    three = device_grads(core, inp, gpu_device, chunks=3)
    for k in pref.GROUPS[:8]:
        assert np.array_equal(three[k], one[k]) and np.abs(one[k]).max() > 0, k
    for a, b in zip(one["forward"], three["forward"]):
        assert torch.equal(a, b)
    print("MEASURED chained_gains", " ".join(f"{k}={np.abs(three[k] - one[k]).max() / np.abs(one[k]).max():.2e}" for k in pref.GAINS))
    for k in pref.GAINS:
        assert np.abs(three[k] - one[k]).max() <= 3 * CHAINED_GAINS_FIGURE * np.abs(one[k]).max(), k


# ---- 5. a shared action block ------------------------------------------------------------------------------------------------------
def test_shared_action_block_gradient_is_the_sum_over_the_steps(gpu_device):
    """action_step_stride == 0, the per-step blocks summed in Python: against the reference with the same block at every step"""
    cfg, K, kind, seed = pref.case("vel_k8_s5")
    core = _core(cfg, gpu_device)
    inp = pref.make_inputs(core.P, cfg, N, K, seed=pref.SHARED_SEED, kind=kind)
    g64 = pref.reference_grads(core.P, cfg, inp, torch.float64, shared_action=True, gains=_own_gains(core).double().numpy())
    got = device_grads(core, inp, gpu_device, shared_action=True)
    err = pref.group_errors(got, g64)
    print("MEASURED shared_vel_k8_s5", " ".join(f"{k}={v:.2e}" for k, v in err.items()))
    assert got["actions"].shape == (1, N, 4) and max(err.values()) < BOUND["shared_vel_k8_s5"], err


# ---- 6. the gains flag, determinism --------------------------------------------------------------------------------------------------
def test_sweep_without_gains_gives_the_same_bits_and_two_calls_agree(gpu_device):
    """the raw entries outside autograd: one taped forward, then sweeps into poisoned buffers with and without g_gains"""
    from gym_pybullet_drones_amd import diff
    cfg, K, kind, seed = pref.case("pid_k8_s5")
    core = _core(cfg, gpu_device)
    inp = pref.make_inputs(core.P, cfg, N, K, seed=seed, kind=kind)
    dev = gpu_device
    _set(core, inp)
    acts = torch.as_tensor(inp.actions, dtype=torch.float32, device=dev).contiguous()
    tape = torch.empty(diff.tape_floats_pid(core, K), dtype=torch.float32, device=dev)
    assert tape.numel() == 22 * K * core.ld
    obs, rew = torch.empty((K, N, 12), device=dev), torch.empty((K, N), device=dev)
    flags = torch.empty((2, K, N), dtype=torch.bool, device=dev)
    diff.tape_forward_pid(core, core._params, K, acts, N * 3, obs, rew, flags[0], flags[1], tape)
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev)     # noqa: E731
    g_kin0 = diff.pack_kin(T(inp.g_pos), T(inp.g_quat), T(inp.g_vel), T(inp.g_rates))
    g_pid0 = diff.pack_pid(T(inp.g_int_pos), T(inp.g_last_rpy), T(inp.g_int_rpy))

    def swept(with_gains):
        g_kin, g_pid = g_kin0.clone(), g_pid0.clone()
        g_act, g_gains = torch.full((K, N, 3), float("nan"), device=dev), torch.full((18, core.ld), 7.0, device=dev)
        diff.sweep_pid(core, core._params, K, acts, N * 3, tape, T(inp.g_obs), T(inp.g_rew), g_kin, g_pid, g_act, g_gains if with_gains else None)
        return g_kin, g_pid, g_act, g_gains

    a, b, c = swept(True), swept(True), swept(False)
    assert bool((c[3] == 7.0).all())                                   # nobody wrote the gains' buffer ...
    assert bool((a[3][:, :N] != 7.0).all()) and bool((a[3][:, N:] == 7.0).all())          # ... drones 0 .. N-1 of every row otherwise
    for x, y, z in zip(a[:3], b[:3], c[:3]):
        assert torch.equal(x, y) and torch.equal(x, z) and bool(torch.isfinite(x).all())
    assert torch.equal(a[3], b[3])
    assert bool(a[0][:4 * core.ld].view(core.ld, 4)[N:].eq(g_kin0[:4 * core.ld].view(core.ld, 4)[N:]).all())      # (the padding is left alone)


# ---- 7. the surface ----------------------------------------------------------------------------------------------------------------
def test_surface_refusals_and_own_gains(gpu_device):
    from gym_pybullet_drones_amd import _native, engine
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    cfg = ref.config("cf2x", "vel", 5, False, "hover")
    core = _core(cfg, gpu_device)
    inp = pref.make_inputs(core.P, cfg, N, 4, seed=2)
    acts = torch.as_tensor(inp.actions, dtype=torch.float32, device=gpu_device)
    with pytest.raises(_native.GpdError, match="the DSLPID action types are not differentiable"):
        core.rollout_diff(acts)
    rpm_core = _core(ref.config("cf2x", "rpm", 5, False, "hover"), gpu_device, act_code=0)
    with pytest.raises(_native.GpdError, match="gpd_rollout_tape_pid_floats: the RPM action types go through gpd_rollout_tape / gpd_rollout_vjp"):
        rpm_core.rollout_diff_pid(torch.zeros((4, N, 4), device=gpu_device))
    with pytest.raises(_native.GpdError, match="physics_flags are not differentiable together with DSLPID"):
        _core(cfg, gpu_device, physics=2).rollout_diff_pid(acts)
    # (an airframe without DSLPID -- pid_kf <= 0 -- cannot be reached from here: `SimCore` refuses the DSLPID action types for the racer
    # and packs the CF2X controller for every airframe; tests/c/diff_pid_host.c and tests/test_host_diff_pid.py hold that refusal)
    with pytest.raises(ValueError, match="pid_gains"):
        core.rollout_diff_pid(acts, pid_gains=torch.ones(5))
    with pytest.raises(ValueError, match="pid0"):
        core.rollout_diff_pid(acts, pid0=torch.zeros(9))
    # pid_gains equal to the core's own gains: the bits of pid_gains=None on every shared output
    with_own, without = device_grads(core, inp, gpu_device, gains="own"), device_grads(core, inp, gpu_device, gains=None)
    for k in pref.GROUPS[:8]:
        assert np.array_equal(with_own[k], without[k]), k
    for x, y in zip(with_own["forward"], without["forward"]):
        assert torch.equal(x, y)
    assert all(np.abs(with_own[k]).max() > 0 for k in pref.GAINS if k != "p_for")
    # ... and other gains fly another flight, without touching the core's own
    before = bytes(core._params)
    _set(core, inp)
    other = core.rollout_diff_pid(acts, pid_gains=_own_gains(core) * 0.5)[0]
    assert bytes(core._params) == before and not torch.equal(other, with_own["forward"][0])


# ---- 8. the example ----------------------------------------------------------------------------------------------------------------
class _RestatementBackend:
    """examples/tune_pid.py's backend interface over the float64 restatement on the CPU: the same start, the same waypoints"""
    dtype = torch.float64

    def __init__(self, tp, wp):
        from host_lib import params
        self.C, self.n = params("cf2x"), wp.shape[0]
        self.cfg = ref.config("cf2x", "pid", 240 // tp.CTRL_FREQ, False, "none")
        self.c = ref.consts(self.C, self.n)
        self.wp = torch.as_tensor(wp, dtype=torch.float64)

    def waypoint(self):
        return self.wp

    def start(self):
        z = torch.zeros((self.n, 3), dtype=torch.float64)
        pos = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(self.n, 3)
        return (pos, torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(self.n, 4), z, z), (z, z, z)

    def chunk(self, gains, state, horizon):
        obs, _, kin, mem = pref.rollout(self.c, pref.pid_consts_of(self.C, gains), self.cfg, state[0], state[1], self.wp.expand(horizon, -1, -1))
        return obs[..., 0:3], (kin, mem)


def test_tune_pid_example_descends_like_the_float64_restatement(gpu_device):
    """`python examples/tune_pid.py --num-envs 128 --iters 8`, the script itself in a process of its own: the loss it prints is finite
    throughout, the gains it prints stay positive, the final loss is below the starting loss and below TWICE the final loss of the same
    optimisation -- same start, same iterations, the example's own `tune()` -- flown through the float64 restatement on the CPU (an Adam
    path is not reproducible across precisions; the threshold is the CPU's figure, not the device's).  Beyond what the threshold
    asks: the device's descent is at least half the restatement's.
    MEASURED on the MI355X: 0.090534 -> 0.079372; the float64 restatement on the CPU: 0.090534 -> 0.079364."""
    import ast
    import re
    import subprocess
    script = os.path.join(REPO, "examples", "tune_pid.py")
    run = subprocess.run([sys.executable, script, "--num-envs", "128", "--iters", "8", "--device", str(gpu_device)], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    rows = re.findall(r"^iter +(\d+) +loss (\S+) +p_for (\[.*?\]) +i_for (\[.*?\]) +d_for (\[.*?\])$", run.stdout, flags=re.M)
    assert [int(r[0]) for r in rows] == list(range(9)), run.stdout[-2000:]
    dev = [float(r[1]) for r in rows]
    gains = np.array([[ast.literal_eval(v) for v in r[2:5]] for r in rows])          # [9 iterations, 3 rows, 3]
    last = re.search(r"^loss (\S+) -> (\S+) over 8 iterations on 128 step responses$", run.stdout, flags=re.M)
    assert last and [float(last.group(1)), float(last.group(2))] == [dev[0], dev[-1]] and "tuned position loop:" in run.stdout
    spec = importlib.util.spec_from_file_location("example_tune_pid", script)
    tp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tp)
    cpu, _ = tp.tune(_RestatementBackend(tp, tp.waypoints(128, 0)), iters=8, verbose=False)
    print(f"MEASURED tune_pid cpu_f64 {cpu[0]:.6f} -> {cpu[-1]:.6f}   device {dev[0]:.6f} -> {dev[-1]:.6f}")
    assert np.isfinite(dev).all() and np.isfinite(gains).all() and (gains > 0).all()
    assert np.allclose(gains[0], np.array(tp.REFERENCE_GAINS[0:3]) * np.array(tp.DETUNE)[:, None], rtol=1e-6) and not np.allclose(gains[-1], gains[0], rtol=0.05)
    assert cpu[-1] < cpu[0]
    assert dev[-1] < dev[0]
    assert dev[-1] < 2.0 * cpu[-1]
    assert dev[0] - dev[-1] > 0.5 * (cpu[0] - cpu[-1])

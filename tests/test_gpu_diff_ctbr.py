"""The differentiable rollout on thrust and body-rate commands on the device (`gpd_rollout_tape_ctbr` / `gpd_rollout_vjp_ctbr`,
DESIGN.md section 3.18): the taped forward against `gpd_rollout_ctbr` bit for bit, the sweep's gradients against float64 autograd of
tests/helpers/diff_ctbr_f64.py per group (rows; pos / quat / vel / rates of kin_0; the four gain triples), the sizes, the padding, chained
calls, K = 1 in "pos" mode against the composition of `gpd_ctbr` with "cmd" mode, the clips' exact zeros, and the example.

Metric: max |g32 - g64| / max |g64| per group.  BOUND is min(1e-4, 3 x the largest figure the case measured on an MI355X) -- 1e-4 is the
project's limit, the 3 x leaves room for box-to-box rounding of the 1-ulp hardware sqrt / rsq.  Every case prints a
MEASURED line before it asserts.  Shapes: 70 drones (a full wave and a ragged one), 200 for the edge kinds (the rare lanes diverge inside
waves 0 and 1), K <= 8."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import ctbr_f64 as H  # noqa: E402
import diff_ctbr_f64 as D  # noqa: E402

pytestmark = pytest.mark.gpu
LIMIT = 1e-4
#: the largest figure over the groups each case measured (profiles/diff_ctbr_mi355x.json "parity")
MEASURED = {"cmd_k8_s5": 5.339e-07, "cmd_k3_s8_cf2p": 5.261e-07, "cmd_k8_s1_racer": 2.224e-07, "pos_k8_s5": 7.843e-07, "pos_k3_s8_plant":
            4.635e-07, "held_rows": 3.906e-07, "thrust_low": 4.099e-07, "thrust_high": 3.725e-07, "rate_beyond": 3.725e-07, "rotor_zero":
            3.725e-07, "rotor_max": 3.973e-07, "shepperd_c2": 1.034e-06, "qe_neg": 3.521e-07}
EDGE_KINDS = D.CMD_KINDS + D.POS_KINDS
POISON = 7.0


def bound(name):
    return min(LIMIT, 3.0 * MEASURED[name]) if name in MEASURED else LIMIT


def _core(dev, model, S, n):
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    return engine.SimCore(drone_model=getattr(DroneModel, D.ref.MODELS[model]), num_envs=n, drones_per_env=1, physics=0, pyb_freq=240,
                          ctrl_freq=240 // S, act_code=D.ref.ACT_CODE["raw_rpm"], task=engine.TASK_NONE, auto_reset=False, track_rpm=True, device=dev)


def _ctrl(dev, model, n):
    from gym_pybullet_drones_amd.control import VectorCTBR
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    return VectorCTBR(n, drone_model=getattr(DroneModel, D.ref.MODELS[model]), device=dev)


def _load(core, inp):
    kin = np.concatenate([inp.pos, inp.quat, inp.vel, inp.rates], axis=1).T
    core.set_state(kin=torch.as_tensor(kin, dtype=torch.float32), last_rpm=torch.zeros((4, core.N)), step_counter=torch.zeros(core.E, dtype=torch.int32))


def _setup(dev, name):
    C, cfg, inp, scales = D.case(name)
    core, ctrl = _core(dev, cfg.model, cfg.S, inp.n), _ctrl(dev, cfg.model, inp.n)
    if scales is not None:
        core.set_plant(torch.as_tensor(scales, dtype=torch.float32, device=dev))
    return C, cfg, inp, scales, core, ctrl


def _device_grads(core, ctrl, inp, with_gains=True):
    """rollout_diff_ctbr from the inputs' state and the tests' loss (a random-weight linear functional of obs12 and kin_K), backwards:
    the gradients by group (numpy float64), obs12 and kin_K"""
    from gym_pybullet_drones_amd.diff import pack_kin, unpack_kin
    dev, n = core.device, core.N
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev)     # noqa: E731
    leaves = [T(v).requires_grad_(True) for v in (inp.pos, inp.quat, inp.vel, inp.rates)]
    rows = T(inp.rows[0] if inp.held else inp.rows).requires_grad_(True)
    gains = T(D.GAINS).requires_grad_(True) if with_gains else None
    obs, kin_k = core.rollout_diff_ctbr(ctrl, rows, pack_kin(*leaves, ld=core.ld), num_steps=inp.K, mode=inp.mode, gains=gains)
    loss = (T(inp.g_obs) * obs).sum() + sum((T(g) * k).sum() for g, k in zip((inp.g_pos, inp.g_quat, inp.g_vel, inp.g_rates), unpack_kin(kin_k, n)))
    loss.backward()
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)     # noqa: E731
    got = {"rows": f64(rows.grad).reshape(inp.rows.shape), **{k: f64(v.grad) for k, v in zip(D.GROUPS[1:5], leaves)}}
    if with_gains:
        got.update({name: f64(gains.grad)[i] for i, name in enumerate(D.GAIN_FIELDS)})
    return got, obs.detach(), kin_k.detach()


def _report(name, err):
    print(f"MEASURED {name} " + " ".join(f"{k}={v:.3e}" for k, v in err.items()) + f" max={max(err.values()):.3e} bound={bound(name):.3e}")


# ---- 1. the taped forward is gpd_rollout_ctbr, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("plant", [False, True])
@pytest.mark.parametrize("model", ["cf2x", "cf2p"])
@pytest.mark.parametrize("mode", ["cmd", "pos"])
def test_taped_forward_is_rollout_ctbr_bit_for_bit(gpu_device, mode, model, plant):
    from gym_pybullet_drones_amd import diff
    n = 70
    C = H.UrdfConstants(H.URDF[model], model)
    ctrl = _ctrl(gpu_device, model, n)
    for S in (1, 5, 8):
        core = _core(gpu_device, model, S, n)
        if plant:
            core.set_plant(torch.as_tensor(D.plant_scales(n), dtype=torch.float32, device=gpu_device))
        for K in (1, 3, 8):
            inp = D.make_inputs(C, n, K, mode, seed=3)
            rows = torch.as_tensor(inp.rows, dtype=torch.float32, device=gpu_device).contiguous()
            _load(core, inp)
            obs, cmd = core.rollout_ctbr(ctrl, rows, K, mode=mode, want_cmd=True)
            want = [t.clone() for t in (obs, cmd, core.kin_store, core.last_rpm, core.step_counter)]
            _load(core, inp)
            obs2, cmd2 = torch.full((K, n, 12), float("nan"), device=gpu_device), torch.full((K, n, 4), float("nan"), device=gpu_device)
            tape = torch.empty(diff.tape_floats_ctbr(core, K), device=gpu_device)
            diff.tape_forward_ctbr(core, ctrl.struct(), mode, K, rows, rows.numel() // K, obs2, tape, cmd2)
            got = (obs2, cmd2, core.kin_store, core.last_rpm, core.step_counter)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (mode, model, plant, S, K)
            assert tape.numel() == 13 * K * core.ld and int(core.step_counter[0]) == K * S
            # the tape's first block is the state the call started from, in the plane layout
            _load(core, inp)
            assert torch.equal(tape[:13 * core.ld].view(-1)[:4 * n], core.kin_store.view(-1)[:4 * n])


# ---- 2. gradients against the float64 restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.CASES) + list(EDGE_KINDS))
def test_gradients_against_float64_autograd(gpu_device, name):
    C, cfg, inp, scales, core, ctrl = _setup(gpu_device, name)
    want = D.reference_grads(C, cfg, inp, scales=scales)
    got, obs, _ = _device_grads(core, ctrl, inp)
    assert all(np.isfinite(v).all() for v in got.values()), name
    fwd = D.ref.forward_error(obs.cpu().numpy(), want["forward"][0].numpy())
    err = D.group_errors(got, want)
    _report(name, err)
    print(f"MEASURED {name} forward={fwd:.3e}")
    assert fwd < LIMIT and max(err.values()) <= bound(name), (name, err)
    if inp.mode == "pos":        # the slots of a target row the forward ignores: exact zeros
        assert (got["rows"][..., 3:6] == 0).all() and (got["rows"][..., 9:12] == 0).all()
    else:                        # no outer loop: its gains have exactly no gradient
        assert all((got[k] == 0).all() for k in ("k_p", "k_d", "k_rates"))
    # beyond a clip the clipped component's gradient is exactly 0.0
    r, g = inp.rows, got["rows"]
    if name == "thrust_low":
        assert (r[:, inp.rare, 0] < 0).all() and (g[:, inp.rare, 0] == 0).all() and (g[:, ~inp.rare, 0] != 0).any()
    if name == "thrust_high":
        assert (r[:, inp.rare, 0] > H.THRUST_MAX).all() and (g[:, inp.rare, 0] == 0).all()
    if name == "rate_beyond":
        out = np.abs(r[..., 1:]) > H.RATE_MAX
        assert out.sum() >= 8 and (g[..., 1:][out] == 0).all()


def test_gains_none_gives_no_gain_gradient_and_the_same_bits(gpu_device):
    C, cfg, inp, scales, core, ctrl = _setup(gpu_device, "pos_k8_s5")
    with_g, obs_a, kin_a = _device_grads(core, ctrl, inp, with_gains=True)
    without, obs_b, kin_b = _device_grads(core, ctrl, inp, with_gains=False)
    assert "k_p" not in without and torch.equal(obs_a, obs_b) and torch.equal(kin_a, kin_b)
    assert all(np.array_equal(with_g[k], without[k]) for k in D.GROUPS[:5])
    # a gains tensor that does not require grad: used, no gradient
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=gpu_device)     # noqa: E731
    gains, rows = T(D.GAINS), T(inp.rows).requires_grad_(True)
    _load(core, inp)
    obs, _ = core.rollout_diff_ctbr(ctrl, rows, mode="pos", gains=gains)
    obs.sum().backward()
    assert gains.grad is None and rows.grad is not None and torch.equal(obs, obs_a)
    # other gains fly another flight
    _load(core, inp)
    obs2, _ = core.rollout_diff_ctbr(ctrl, rows.detach(), mode="pos", gains=gains * 1.5)
    assert not torch.equal(obs2, obs_a)


# ---- 3. sizes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_sizes(gpu_device, n):
    C = H.UrdfConstants(H.URDF["cf2x"], "cf2x")
    cfg = D.config("cf2x", 5)
    for mode in ("cmd", "pos"):
        inp = D.make_inputs(C, n, 3, mode, seed=4)
        core, ctrl = _core(gpu_device, "cf2x", 5, n), _ctrl(gpu_device, "cf2x", n)
        _load(core, inp)
        want = D.reference_grads(C, cfg, inp)
        got, _, _ = _device_grads(core, ctrl, inp)
        err = D.group_errors(got, want)
        _report(f"size_{n}_{mode}", err)
        assert max(err.values()) <= LIMIT, (n, mode, err)


# ---- 4. the padding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cmd", "pos"])
def test_padding_lanes_stay_untouched(gpu_device, mode):
    """the words of g_kin and g_gains past drone N - 1 are the sweep's to leave alone (diff_gpu.padding_is_poison's idea)"""
    from gym_pybullet_drones_amd import diff
    n, K = 70, 3
    C = H.UrdfConstants(H.URDF["cf2x"], "cf2x")
    inp = D.make_inputs(C, n, K, mode, seed=6)
    core, ctrl = _core(gpu_device, "cf2x", 5, n), _ctrl(gpu_device, "cf2x", n)
    ld = core.ld
    assert ld > n
    _load(core, inp)
    rows = torch.as_tensor(inp.rows, dtype=torch.float32, device=gpu_device).contiguous()
    obs, tape = torch.empty((K, n, 12), device=gpu_device), torch.empty(diff.tape_floats_ctbr(core, K), device=gpu_device)
    diff.tape_forward_ctbr(core, ctrl.struct(), mode, K, rows, rows.numel() // K, obs, tape)
    parts = [torch.as_tensor(g, dtype=torch.float32, device=gpu_device) for g in (inp.g_pos, inp.g_quat, inp.g_vel, inp.g_rates)]
    g_kin = diff.pack_kin(*parts, ld=ld)
    for plane in range(3):
        g_kin[4 * ld * plane:4 * ld * (plane + 1)].view(ld, 4)[n:] = POISON
    g_kin[12 * ld + n:] = POISON
    g_rows = torch.full((K, n, rows.shape[-1]), float("nan"), device=gpu_device)
    g_gains = torch.full((12, ld), POISON, device=gpu_device)
    g_obs = torch.as_tensor(inp.g_obs, dtype=torch.float32, device=gpu_device).contiguous()
    diff.sweep_ctbr(core, ctrl.struct(), mode, K, rows, rows.numel() // K, tape, g_obs, g_kin, g_rows, g_gains)
    assert all(bool((g_kin[4 * ld * p:4 * ld * (p + 1)].view(ld, 4)[n:] == POISON).all()) for p in range(3))
    assert bool((g_kin[12 * ld + n:] == POISON).all()) and bool((g_gains[:, n:] == POISON).all())
    assert bool(torch.isfinite(g_rows).all()) and bool(torch.isfinite(g_gains[:, :n]).all()) and bool((g_gains[:, :n] != POISON).all())
    # two sweeps give the same bits (no atomics), with and without the gains' output
    g_kin2 = diff.pack_kin(*parts, ld=ld)
    g_rows2 = torch.empty_like(g_rows)
    diff.sweep_ctbr(core, ctrl.struct(), mode, K, rows, rows.numel() // K, tape, g_obs, g_kin2, g_rows2, None)
    assert torch.equal(g_rows2, g_rows) and torch.equal(diff.unpack_kin(g_kin2, n)[1], diff.unpack_kin(g_kin, n)[1])


# ---- 5. chained calls --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["cmd", "pos"])
def test_three_chained_calls_are_one_call(gpu_device, mode):
    from gym_pybullet_drones_amd.diff import pack_kin
    n, K = 70, 12
    C = H.UrdfConstants(H.URDF["cf2x"], "cf2x")
    inp = D.make_inputs(C, n, K, mode, seed=8)
    core, ctrl = _core(gpu_device, "cf2x", 5, n), _ctrl(gpu_device, "cf2x", n)
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=gpu_device)     # noqa: E731
    w_obs, w_kin = T(inp.g_obs), torch.randn(13 * core.ld, device=gpu_device, generator=torch.Generator(gpu_device).manual_seed(1))

    def run(chunks):
        leaves = [T(v).requires_grad_(True) for v in (inp.pos, inp.quat, inp.vel, inp.rates)]
        rows, gains = T(inp.rows).requires_grad_(True), T(D.GAINS).requires_grad_(True)
        kin, obs = pack_kin(*leaves, ld=core.ld), []
        for a in range(0, K, K // chunks):
            o, kin = core.rollout_diff_ctbr(ctrl, rows[a:a + K // chunks], kin, mode=mode, gains=gains)
            obs.append(o)
        obs = torch.cat(obs)
        ((w_obs * obs).sum() + (w_kin * kin).sum()).backward()
        return [obs.detach(), kin.detach(), rows.grad] + [v.grad for v in leaves], gains.grad
    one, g_one = run(1)
    three, g_three = run(3)
    assert all(torch.equal(a, b) for a, b in zip(one, three))
    # the gains' gradient is summed over drones per call and over the calls by autograd: the same terms in another order
    assert torch.allclose(g_one, g_three, rtol=1e-5, atol=1e-6 * float(g_one.abs().max()))


# ---- 6. K = 1 in "pos" mode is gpd_ctbr composed with K = 1 in "cmd" mode ---------------------------------------------------------------
def test_pos_mode_of_one_step_is_the_composition(gpu_device):
    """the gradients of one "pos" step equal those of (gpd_ctbr, one "cmd" step) with the command's cotangent taken through the outer
    loop's adjoint on the host restatement (float64 autograd of diff_ctbr_f64.outer), to the bound of the gradient tests"""
    n = 70
    C = H.UrdfConstants(H.URDF["cf2x"], "cf2x")
    inp = D.make_inputs(C, n, 1, "pos", seed=9)
    core, ctrl = _core(gpu_device, "cf2x", 5, n), _ctrl(gpu_device, "cf2x", n)
    _load(core, inp)
    pos_g, obs_pos, _ = _device_grads(core, ctrl, inp, with_gains=False)
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=gpu_device)     # noqa: E731
    cmd = ctrl.compute(T(inp.pos), T(inp.quat), T(inp.vel), T(inp.rows[0, :, 0:3]), T(inp.rows[0, :, 6:9]))
    from types import SimpleNamespace
    as_cmd = SimpleNamespace(**{**vars(inp), "mode": "cmd", "rows": cmd.cpu().numpy().astype(np.float64)[None]})
    cmd_g, obs_cmd, _ = _device_grads(core, ctrl, as_cmd, with_gains=False)
    assert torch.equal(obs_pos, obs_cmd)
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)     # noqa: E731
    xs = [leaf(v) for v in (inp.pos, inp.quat, inp.vel, inp.rows[0, :, 0:3], inp.rows[0, :, 6:9])]
    out = D.outer(D.controller(C), torch.as_tensor(D.GAINS), *xs)
    through = [g.numpy() for g in torch.autograd.grad((torch.as_tensor(cmd_g["rows"][0]) * out).sum(), xs)]
    want = {"pos": cmd_g["pos"] + through[0], "quat": cmd_g["quat"] + through[1], "vel": cmd_g["vel"] + through[2], "rates": cmd_g["rates"],
            "rows": np.concatenate([through[3], np.zeros((n, 3)), through[4], np.zeros((n, 3))], axis=1)[None]}
    err = D.group_errors(pos_g, want, D.GROUPS[:5])
    _report("pos_k1_composition", err)
    assert max(err.values()) <= LIMIT, err


# ---- 7. the aviary's method and the example ----------------------------------------------------------------------------------------------
def test_vector_aviary_rollout_diff_ctbr(gpu_device):
    from gym_pybullet_drones_amd.control import VectorCTBR
    from gym_pybullet_drones_amd.envs import VectorCtrlAviary
    n = 70
    env = VectorCtrlAviary(n, pyb_freq=240, ctrl_freq=48, device=gpu_device)
    env.reset()
    ctrl = VectorCTBR(n, device=gpu_device)
    cmd = torch.tensor([10.5, 0.0, 0.0, 0.0], device=gpu_device).repeat(n, 1).requires_grad_(True)
    obs, kin_k = env.rollout_diff_ctbr(ctrl, cmd, num_steps=4)
    assert obs.shape == (4, n, 1, 12) and kin_k.shape == (13 * env.core.ld,)
    obs[-1, :, 0, 2].sum().backward()
    # more thrust raises every drone; a held block's gradient is the sum over the steps, in the block's shape
    assert cmd.grad.shape == cmd.shape and bool((cmd.grad[:, 0] > 0).all())


def test_example_apg_ctbr_losses_fall(gpu_device):
    spec = importlib.util.spec_from_file_location("example_apg_ctbr", os.path.join(REPO, "examples", "apg_ctbr.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    traj, policy = m.run(num_envs=128, traj_iters=12, policy_iters=12, horizon=12, device=gpu_device, verbose=False)
    print(f"MEASURED example trajectory {traj[0]:.5f} -> {traj[-1]:.5f}; policy {policy[0]:.5f} -> {policy[-1]:.5f}")
    assert traj[-1] < traj[0] and policy[-1] < policy[0], (traj, policy)

"""The device harness of tests/test_gpu_diff.py and tests/test_gpu_sysid.py: a core for a configuration of tests/helpers/diff_f64.py,
the inputs' state into it, the loss whose gradients the tests compare, and the raw entries outside autograd -- one taped forward, and
reverse sweeps over it into poisoned outputs (`diff.tape_forward` / `diff.sweep`).  Test infrastructure."""
import numpy as np
import torch

import diff_f64 as ref

N = 70          # ld = 128: two waves, one ragged
MODELS = ref.MODELS


def core(cfg, dev, n=N, task="hover", nan_guard=False):
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    pyb_freq = round(1.0 / cfg.h)
    return engine.SimCore(drone_model=getattr(DroneModel, MODELS[cfg.model]), num_envs=n, drones_per_env=1, physics=2 if cfg.drag else 0,
                          pyb_freq=pyb_freq, ctrl_freq=pyb_freq // cfg.S, act_code=ref.ACT_CODE[cfg.act],
                          task=engine.TASK_HOVER if task == "hover" else engine.TASK_NONE, target_pos=[[0.0, 0.0, 1.0]], auto_reset=False,
                          track_rpm=True, nan_guard=nan_guard, device=dev)


def set_state(core, inp):
    """the inputs' state into the core (the logical [13, n] rows; the RPMs the first drag term sees)"""
    kin = np.concatenate([inp.pos, inp.quat, inp.vel, inp.rates], axis=1).T
    core.set_state(kin=torch.as_tensor(kin, dtype=torch.float32), last_rpm=torch.as_tensor(inp.last_rpm.T, dtype=torch.float32),
                   step_counter=torch.zeros(core.E, dtype=torch.int32))


def loss(inp, dev, obs, rew, kin_k, n, with_obs=True):
    """sum(cotangent * output) over reward, the final state (`kin_k` None: left out) and -- `with_obs` -- the observations"""
    from gym_pybullet_drones_amd.diff import unpack_kin
    T = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev)     # noqa: E731
    total = (T(inp.g_rew) * rew).sum()
    if kin_k is not None:
        total = total + sum((T(g) * k).sum() for g, k in zip((inp.g_pos, inp.g_quat, inp.g_vel, inp.g_rates), unpack_kin(kin_k, n)))
    return total + (T(inp.g_obs) * obs).sum() if with_obs else total


def taped(core, inp, K, with_outputs=False):
    """the inputs' state and `gpd_rollout_tape` over their K action blocks, outside autograd: (actions, tape), and -- `with_outputs` --
    the obs12 [K, n, 12] and reward [K, n] it wrote"""
    from gym_pybullet_drones_amd import diff
    dev, n = core.device, core.N
    set_state(core, inp)
    acts = torch.as_tensor(inp.actions, dtype=torch.float32, device=dev).contiguous()
    tape = torch.empty(diff.tape_floats(core, K), dtype=torch.float32, device=dev)
    obs, rew = torch.empty((K, n, 12), device=dev), torch.empty((K, n), device=dev)
    flags = torch.empty((2, K, n), dtype=torch.bool, device=dev)
    diff.tape_forward(core, K, acts, n * inp.A, obs, rew, flags[0], flags[1], tape)
    return (acts, tape, obs, rew) if with_outputs else (acts, tape)


POISON = 7.0


def cotangent_block(core, parts=None):
    """a `g_kin` block [13 * ld] for `swept`: the cotangents `parts` = (pos, quat, vel, rates) of drones 0 .. N-1 (None: zeros) and
    POISON in every word past them -- the rows N .. ld-1 a sweep must leave alone"""
    from gym_pybullet_drones_amd.diff import pack_kin
    n, ld, dev = core.N, core.ld, core.device
    if parts is None:
        parts = [torch.zeros((n, k), device=dev) for k in (3, 4, 3, 3)]
    block = pack_kin(*[torch.as_tensor(p, dtype=torch.float32, device=dev) for p in parts], ld=ld)
    for plane in range(3):
        block[4 * ld * plane:4 * ld * (plane + 1)].view(ld, 4)[n:] = POISON
    block[12 * ld + n:] = POISON
    return block


def padding_is_poison(core, g_kin):
    """every word of a swept `g_kin` past drone N - 1 is still POISON"""
    n, ld = core.N, core.ld
    planes = all(bool((g_kin[4 * ld * p:4 * ld * (p + 1)].view(ld, 4)[n:] == POISON).all()) for p in range(3))
    return planes and bool((g_kin[12 * ld + n:] == POISON).all())


def swept(core, K, acts, tape, g_obs, g_rew, g_kin0, with_rows=False):
    """one reverse sweep over `tape` into poisoned outputs -- a clone of `g_kin0`, NaN for g_act, 7.0 for the plant rows' cotangents
    (`with_rows`: `gpd_rollout_vjp_plant`, else `gpd_rollout_vjp` leaves them alone): (g_kin, g_act, g_rows)"""
    from gym_pybullet_drones_amd import _native, diff
    dev, n = core.device, core.N
    g_kin, g_act = g_kin0.clone(), torch.full((K, n, core.A), float("nan"), device=dev)
    g_rows = torch.full((_native.PLANT_ROWS, core.ld), 7.0, device=dev)
    diff.sweep(core, K, acts, acts.numel() // K, tape, g_obs, g_rew, g_kin, g_act, g_rows=g_rows if with_rows else None)
    return g_kin, g_act, g_rows

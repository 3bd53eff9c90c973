"""Inputs of the CTBR-task tests (tests/test_gpu_ctbr_task.py, tests/test_host_ctbr_task.py): start states, counters and commands placed
so that every cause of an episode end occurs a few steps into a launch, and a float64 prediction of which drone ends when and why
(tests/helpers/ctbr_f64.py: the rate loop over the oracle's integrator, then the task of envs/HoverAviary.py restated in float64).
numpy only: the host test checks the prediction, the device test asserts the same condition on the composition's own flags.

A drone's group is n % 6:
  0  box     flies out of xy_bound along +-x            3  near    climbs into term_dist of the target (terminated)
  1  clock   its counter passes trunc_counter           4  none    hovers half a metre from the target
  2  tilt    rolls (odd rounds: pitches) past tilt_bound 5  ceiling climbs past z_bound
Each event is placed 2.5 control steps after the start: step 2 of a launch, half a step of margin either way."""
import numpy as np

import ctbr_f64 as H

GROUPS = ("box", "clock", "tilt", "near", "none", "ceiling")
XY_BOUND, Z_BOUND, TILT_BOUND, TERM_DIST, TRUNC_COUNTER = 1.5, 2.0, 0.4, 0.05, 1000
EVERY = 1 | 2 | 8 | 16          # GPD_PHYS_GND | DRAG | GROUND | DAMP
LEAD = 2.5                      # control steps between the start and the event
SPEED, RATE, CLIMB = 2.0, 5.0, 0.6


def quat_of_rpy(rpy):
    """x, y, z, w of roll, pitch, yaw [n, 3] (the ZYX convention of the simulator)"""
    r, p, y = (np.asarray(rpy, dtype=np.float64)[:, i] / 2 for i in range(3))
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


class Scene:
    pass


def scene(N, K, S, seed=3, target_per_env=0, init_per_env=0):
    """start state, counters, targets, reset poses and K blocks of physical commands (thrust m/s^2 | rates rad/s) for N drones at S
    sub-steps per control step"""
    rng = np.random.default_rng(seed)
    dt = S / 240.0
    g = np.arange(N) % 6
    sign = np.where((np.arange(N) // 6) % 2 == 0, 1.0, -1.0)
    s = Scene()
    s.N, s.K, s.S, s.group = N, K, S, g
    target = np.tile(np.array([0.0, 0.0, 1.0]), (N, 1))
    if target_per_env:
        target += rng.uniform(-0.1, 0.1, (N, 3))
    pos = target + np.stack([0.5 * sign, rng.uniform(-0.2, 0.2, N), rng.uniform(-0.2, 0.2, N)], axis=-1)       # (none, clock: half a metre off)
    rpy, vel, w = np.zeros((N, 3)), rng.normal(0.0, 0.05, (N, 3)), rng.normal(0.0, 0.1, (N, 3))
    cmd = np.concatenate([rng.uniform(9.0, 10.6, (K, N, 1)), rng.normal(0.0, 0.3, (K, N, 3))], axis=-1)
    hover = np.array([9.8, 0.0, 0.0, 0.0])
    box, tilt, near, ceil = g == 0, g == 2, g == 3, g == 5
    pos[box] = np.stack([sign[box] * (XY_BOUND - LEAD * SPEED * dt), 0.2 * sign[box], np.full(box.sum(), 1.0)], axis=-1)
    vel[box] = np.stack([sign[box] * SPEED, np.zeros(box.sum()), np.zeros(box.sum())], axis=-1)
    axis = np.where((np.arange(N) // 6) % 2 == 0, 0, 1)         # roll in even rounds, pitch in odd ones
    for n in np.flatnonzero(tilt):
        rpy[n, axis[n]] = sign[n] * (TILT_BOUND - LEAD * RATE * dt) if LEAD * RATE * dt < TILT_BOUND else 0.0
        w[n] = 0.0
        w[n, axis[n]] = sign[n] * RATE
    pos[near] = target[near] - np.array([0.0, 0.0, 1.0]) * (TERM_DIST + LEAD * CLIMB * dt)
    vel[near] = np.array([0.0, 0.0, CLIMB])
    pos[ceil] = np.stack([0.3 * sign[ceil], np.full(ceil.sum(), -0.3), np.full(ceil.sum(), Z_BOUND - LEAD * SPEED * dt)], axis=-1)
    vel[ceil] = np.array([0.0, 0.0, SPEED])
    w[box | near | ceil] = 0.0
    cmd[:, box | near | ceil] = hover
    for n in np.flatnonzero(tilt):
        cmd[:, n] = hover
        cmd[:, n, 1 + axis[n]] = sign[n] * RATE
    # aggressive commands for the drones that restart from the reset pose: from step 3 on, beyond both clips in places
    late = np.arange(K) >= 3
    cmd[np.ix_(late, box)] = np.array([60.0, 9.0, -9.0, 3.0])
    cmd[np.ix_(late, ceil)] = np.array([-5.0, -2.0, 2.0, -9.0])
    s.counter = np.where(g == 1, TRUNC_COUNTER - S, rng.integers(0, 40, N) * S).astype(np.int32)
    s.pos, s.rpy, s.vel, s.w = pos, rpy, vel, w
    s.quat = quat_of_rpy(rpy)
    s.kin = np.concatenate([pos, s.quat, vel, w], axis=-1).T.astype(np.float32)        # the logical [13, N] rows
    s.last_rpm = rng.uniform(12000.0, 16000.0, (4, N)).astype(np.float32)
    s.cmd = cmd.astype(np.float32)
    s.target = (target if target_per_env else target[0:1]).astype(np.float32)
    init_xyz = np.stack([rng.uniform(-0.5, 0.5, N), rng.uniform(-0.5, 0.5, N), rng.uniform(0.4, 0.8, N)], axis=-1)
    init_rpy = np.stack([rng.uniform(-0.1, 0.1, N), rng.uniform(-0.1, 0.1, N), rng.uniform(-3.0, 3.0, N)], axis=-1)
    if not init_per_env:
        init_xyz, init_rpy = np.tile(init_xyz[0:1], (N, 1)), np.tile(init_rpy[0:1], (N, 1))
    s.init_xyz, s.init_rpy, s.target_per_env, s.init_per_env = init_xyz, init_rpy, target_per_env, init_per_env
    return s


def causes(obs12, counter, target):
    """the task of envs/HoverAviary.py on rows: (terminated, clock, box, tilt), each [n] bool -- any dtype, evaluated as given"""
    p, roll, pitch = obs12[:, 0:3], obs12[:, 3], obs12[:, 4]
    dist = np.sqrt(((target - p) ** 2).sum(axis=-1))
    box = (np.abs(p[:, 0]) > XY_BOUND) | (np.abs(p[:, 1]) > XY_BOUND) | (p[:, 2] > Z_BOUND)
    tilt = (np.abs(roll) > TILT_BOUND) | (np.abs(pitch) > TILT_BOUND)
    return dist < TERM_DIST, counter > TRUNC_COUNTER, box, tilt


def predict(s, flags=0, mass_scale=None, auto_reset=True):
    """float64: for every drone the first step it ends at (K: never) and the causes at that step [4, N]; `predict.ends` keeps the
    [K, N] flags of the latest call"""
    sim = H.CtbrF64("cf2x", s.N, pos=s.pos, quat=s.quat, vel=s.vel, w=s.w, last_rpm=s.last_rpm.T.astype(np.float64), physics_flags=flags,
                    ctrl_freq=240 // s.S, mass_scale=mass_scale)
    av = sim.av
    counter = s.counter.astype(np.int64).copy()
    first, why = np.full(s.N, s.K), np.zeros((4, s.N), dtype=bool)
    init_q = quat_of_rpy(s.init_rpy)
    predict.ends = np.zeros((s.K, s.N), dtype=bool)
    for t in range(s.K):
        obs, _ = sim.step(s.cmd[t].astype(np.float64))
        c = causes(obs, counter, s.target.astype(np.float64))
        done = c[0] | c[1] | c[2] | c[3]
        predict.ends[t] = done
        new = done & (first == s.K)
        first[new] = t
        why[:, new] = np.stack(c)[:, new]
        counter = counter + s.S
        if auto_reset and done.any():
            av.pos[done, 0], av.quat[done, 0], av.vel[done, 0], av.rpy_rates[done, 0] = s.init_xyz[done], init_q[done], 0.0, 0.0
            av.last_rpm[done] = 0.0
            counter[done] = 0
    return first, why


def condition(first, why, K):
    """what the K = 6 cases need of their inputs: (share that ends before the last step, distinct causes among clock / box / tilt,
    drones that terminate)"""
    early = first < K - 1
    return float(early.mean()), int(sum(bool(why[i, early].any()) for i in (1, 2, 3))), int(why[0, early].sum())

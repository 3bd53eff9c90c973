#!/usr/bin/env python3
"""Tuning the cascaded PID by back-propagation through the flight (`rollout_diff_pid(..., pid_gains=)`, gym_pybullet_drones_amd/diff.py).

N Crazyflies (CF2X) hover at rest and are each given a waypoint a few decimetres away (`ActionType.PID`): N step responses of the
closed loop, flown for `chunks` x `horizon` control steps at 48 Hz (by default 2 x 8: a third of a second, the start of the response).
The position loop starts deliberately detuned -- a third of the proportional gains, 2.5 times the derivative gains: a sluggish,
over-damped response -- and Adam runs on the LOGARITHMS of its nine gains (p_for, i_for, d_for; the attitude loop keeps the reference's),
the loss being the mean squared distance to the waypoint over the flight.  The gradient comes out of the reverse sweep through physics
and controller (`gpd_rollout_vjp_pid`); the flight is cut into chunks chained through `kin_K` / `pid_K`, so that a chunk's tape is all a
launch ever holds.  Prints the loss and the gains per iteration.

Keep the differentiated flight SHORT.  The attitude loop is stiff (p_tor 70 000, and d_tor 20 000 on a finite difference of Euler angles
at 48 Hz) and its +-3200 torque clamps engage and release all the time; the sensitivity of the trajectory to the gains grows with every
control step, and beyond some 20 of them the exact gradient at a point -- which is what the sweep returns, and what a finite difference
confirms -- no longer describes the landscape around it: at 48 steps it is a thousand times the slope of the loss over a 1 % change of a
gain, with either sign.  Up to 16 steps gradient and landscape agree and Adam descends.

`tune()` is the optimisation and knows nothing of the device: it flies through a backend with `start()` and `chunk()`.  `DeviceBackend`
is the simulator; a test flies the same optimisation through a float64 restatement.

Usage:  python examples/tune_pid.py [--num-envs 4096] [--iters 40] [--horizon 8] [--chunks 2]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

#: the reference's gains, rows p_for, i_for, d_for, p_tor, i_tor, d_tor (control/DSLPIDControl.py:37-46)
REFERENCE_GAINS = ((.4, .4, 1.25), (.05, .05, .05), (.2, .2, .5), (70000., 70000., 60000.), (.0, .0, 500.), (20000., 20000., 12000.))
#: where the tuning starts: the position loop's rows scaled by these
DETUNE = (1.0 / 3.0, 1.0, 2.5)
CTRL_FREQ = 48


def waypoints(num_envs, seed=0):
    """[N, 3] float32-representable waypoints 0.2 .. 0.4 m from the start pose (0, 0, 1), in random directions"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((num_envs, 3))
    d *= (rng.uniform(0.2, 0.4, (num_envs, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    return (np.array([0.0, 0.0, 1.0]) + d).astype(np.float32)


class DeviceBackend:
    """the simulator: one `SimCore` of N single-drone aviaries flying `ActionType.PID`"""
    dtype = torch.float32

    def __init__(self, wp, device="cuda:0"):
        from gym_pybullet_drones_amd import engine
        self.dev = torch.device(device)
        self.n = wp.shape[0]
        self.core = engine.SimCore(num_envs=self.n, drones_per_env=1, pyb_freq=240, ctrl_freq=CTRL_FREQ, act_code=1, task=engine.TASK_NONE,
                                   initial_xyzs=[[0.0, 0.0, 1.0]], auto_reset=False, device=self.dev)
        self.wp = torch.as_tensor(wp, device=self.dev)
        self.kin0, self.pid0 = self.core.kin_store.clone(), self.core.pid.clone()

    def start(self):
        """the state a flight starts from: at rest at (0, 0, 1), the controller's members zero"""
        return self.kin0, self.pid0

    def chunk(self, gains, state, horizon):
        """`horizon` control steps towards the waypoints with `gains` [6, 3] -> (positions [horizon, N, 3], the state after them)"""
        obs, _, kin, pid, _, _ = self.core.rollout_diff_pid(self.wp, state[0], state[1], num_steps=horizon, pid_gains=gains)
        return obs[..., 0:3], (kin, pid)

    def waypoint(self):
        return self.wp


def tune(backend, iters=40, horizon=8, chunks=2, lr=0.1, verbose=True):
    """Adam on the logarithms of the position loop's nine gains -> (the loss per iteration, the gains [6, 3] per iteration; the last
    entry of either belongs to the tuned gains' own flight)"""
    ref = torch.tensor(REFERENCE_GAINS, dtype=backend.dtype)
    log_g = torch.log(ref[0:3] * torch.tensor(DETUNE, dtype=backend.dtype)[:, None]).requires_grad_(True)
    opt = torch.optim.Adam([log_g], lr=lr)
    wp = backend.waypoint()
    losses, history = [], []
    for it in range(iters + 1):
        opt.zero_grad()
        gains = torch.cat([torch.exp(log_g), ref[3:6]])
        state, total = backend.start(), 0.0
        for _ in range(chunks):
            pos, state = backend.chunk(gains, state, horizon)
            total = total + ((pos - wp) ** 2).sum()
        loss = total / (chunks * horizon * pos.shape[1])
        losses.append(float(loss.detach()))
        history.append(gains.detach().clone())
        if verbose:
            g = gains.detach()[0:3]
            print(f"iter {it:3d}  loss {losses[-1]:.6f}  p_for {g[0].tolist()}  i_for {g[1].tolist()}  d_for {g[2].tolist()}")
        if it == iters:
            break
        loss.backward()
        opt.step()
    return losses, history


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--horizon", type=int, default=8, help="control steps per chunk (one taped launch)")
    ap.add_argument("--chunks", type=int, default=2)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    losses, history = tune(DeviceBackend(waypoints(a.num_envs, a.seed), a.device), a.iters, a.horizon, a.chunks, a.lr)
    print(f"loss {losses[0]:.6f} -> {losses[-1]:.6f} over {a.iters} iterations on {a.num_envs} step responses")
    print("tuned position loop:", [[round(v, 4) for v in row] for row in history[-1][0:3].tolist()])


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Sampling-based MPC over thrust and body-rate commands: the course of `examples/avoid.py` and `examples/mppi.py` -- N drones, each in
an aviary of its own with the same random cylinders from the same seed and the same starts -- flown on CTBR commands
(`VectorCtrlAviary.rollout_ctbr(mode="cmd")`: the body-rate loop inside every physics sub-step).  Every control step each drone rolls
256 perturbed command sequences half a second ahead through the physics AND the rate loop, scores them against a goal a little ahead
of it and the clearance to its cylinders, and flies the first command of the weighted average (`VectorAviary.mppi_ctbr`, one launch
per plan).  Printed beside a blind flight towards the same goal: `rollout_ctbr(mode="pos")`, the reference's CTBRControl outer loop,
which knows nothing of the cylinders.

Usage:  python examples/mppi_ctbr.py [--drones 4096]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd.control import VectorCTBR  # noqa: E402
from gym_pybullet_drones_amd.envs import VectorCtrlAviary  # noqa: E402
from gym_pybullet_drones_amd.mppi import MPPICost  # noqa: E402
from gym_pybullet_drones_amd.obstacles import ObstacleField  # noqa: E402

PASSED_X = 2.0      # m: beyond the last cylinder
GOAL_X = 3.5        # m: where both flights are headed
AHEAD = 1.5         # m: the goal of a step is at most this far ahead in x (it sets the speed: both flights chase the same point)


def fly(field, start, planned, duration_sec, device, horizon=24, samples=256, sigma=(2.0, 3.0, 3.0, 0.5), lam=0.05, seed=0, cost=None):
    """(share that touched a cylinder, share that passed x >= PASSED_X); `planned`: CTBRMPPI's commands, else the outer loop's"""
    n = len(start)
    env = VectorCtrlAviary(n, 1, initial_xyzs=start[:, None, :], pyb_freq=240, ctrl_freq=48, device=device)
    env.reset()
    env.set_obstacles(field)
    ctrl = VectorCTBR(n, device=env.device)
    if planned:
        cost = MPPICost(w_pos=1.0, w_vel=0.05, w_tilt=0.5, w_rate=0.002, w_term=4.0, w_obs=300.0, obst_margin=0.35) if cost is None else cost
        planner = env.mppi_ctbr(ctrl, horizon, samples, sigma=sigma, lam=lam, cost=cost, seed=seed)
    goal = torch.as_tensor(np.stack([np.full(n, GOAL_X), start[:, 1], start[:, 2]], axis=1), dtype=torch.float32, device=env.device)
    collided = torch.zeros(n, dtype=torch.bool, device=env.device)
    for _ in range(int(duration_sec * env.CTRL_FREQ)):
        g = goal.clone()
        g[:, 0] = torch.minimum(goal[:, 0], env.core.positions()[:, 0] + AHEAD)
        if planned:
            env.rollout_ctbr(ctrl, planner.plan(g), 1, mode="cmd", last_only=True)
            planner.advance()
        else:
            env.rollout_ctbr(ctrl, g, 1, mode="pos", last_only=True)
        collided |= env.obstacle_hits()[:, 0]
    passed = env.core.positions()[:, 0] >= PASSED_X
    out = float(collided.float().mean()), float(passed.float().mean())
    env.close()
    return out


def run(drones=4096, cylinders=6, duration_sec=8, device="cuda:0", **planner):
    """avoid.py's course and seed.  Returns (blind collided share, MPPI collided share, MPPI share that passed x >= +2 m)."""
    rng = np.random.default_rng(0)
    field = ObstacleField.random_cylinders(drones, cylinders, (-1.5, -1.5, 1.5, 1.5), (0.15, 0.3), (1.5, 2.5), rng)
    start = np.stack([np.full(drones, -2.5), rng.uniform(-1.0, 1.0, drones), np.full(drones, 1.0)], axis=1)
    blind, blind_passed = fly(field, start, False, duration_sec, device)
    hit, passed = fly(field, start, True, duration_sec, device, **planner)
    print(f"[mppi_ctbr.py] {drones} drones through {cylinders} cylinders each: the outer loop alone {100.0 * blind:.1f} % collided "
          f"({100.0 * blind_passed:.1f} % passed x >= {PASSED_X:+.0f} m); MPPI over CTBR commands {100.0 * hit:.1f} % collided, "
          f"{100.0 * passed:.1f} % passed")
    return blind, hit, passed


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=4096)
    ap.add_argument("--cylinders", type=int, default=6)
    ap.add_argument("--duration_sec", type=float, default=8)
    a = ap.parse_args()
    run(drones=a.drones, cylinders=a.cylinders, duration_sec=a.duration_sec)

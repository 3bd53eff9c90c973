#!/usr/bin/env python3
"""Sampling-based MPC demo: the course of `examples/avoid.py` -- N drones (`VectorVelocityAviary`, 48 Hz velocity commands tracked by
the embedded DSLPID controllers), each in an aviary of its own with the same random cylinders from the same seed and the same starts --
flown by MPPI over the velocity commands: every control step each drone rolls 256 perturbed command sequences half a second ahead
through the physics AND its controller, scores them against a goal beyond the course and the clearance to its cylinders, and flies the
first command of the weighted average (`VectorAviary.mppi`, one launch per plan).  Printed beside the blind flight of avoid.py.

Usage:  python examples/mppi.py [--drones 4096]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import avoid  # noqa: E402
from gym_pybullet_drones_amd.envs import VectorVelocityAviary  # noqa: E402
from gym_pybullet_drones_amd.mppi import MPPICost  # noqa: E402
from gym_pybullet_drones_amd.obstacles import ObstacleField  # noqa: E402

PASSED_X = 2.0      # m: beyond the last cylinder


def fly_mppi(field, start, duration_sec, speed, device, horizon=24, samples=256, seed=0):
    """(share that touched a cylinder, share that passed x >= PASSED_X)"""
    n = len(start)
    env = VectorVelocityAviary(n, 1, initial_xyzs=start[:, None, :], pyb_freq=240, ctrl_freq=48, device=device)
    env.reset()
    env.set_obstacles(field)
    cost = MPPICost(w_pos=0.3, w_vel=0.0, w_tilt=0.5, w_rate=0.002, w_term=4.0, w_obs=300.0, obst_margin=0.35)
    planner = env.mppi(horizon, samples, sigma=(0.4, 0.4, 0.15, 0.5), lam=0.05, cost=cost, seed=seed,
                       act_lo=(-1.0, -1.0, -1.0, 0.0), act_hi=(1.0, 1.0, 1.0, speed))
    planner.reset(value=(1.0, 0.0, 0.0, speed))                                     # the blind flight's command as the first nominal
    goal = torch.as_tensor(np.stack([np.full(n, 3.5), start[:, 1], start[:, 2]], axis=1), dtype=torch.float32, device=env.device)
    collided = torch.zeros(n, dtype=torch.bool, device=env.device)
    for _ in range(int(duration_sec * env.CTRL_FREQ)):
        action = planner.plan(goal)
        env.step(action.view(n, 1, 4))
        planner.advance()
        collided |= env.obstacle_hits()[:, 0]
    passed = env.core.positions()[:, 0] >= PASSED_X
    out = float(collided.float().mean()), float(passed.float().mean())
    env.close()
    return out


def run(drones=4096, cylinders=6, duration_sec=8, speed=3.0, device="cuda:0"):
    """avoid.py's course and seed.  Returns (blind collided share, MPPI collided share, MPPI share that passed x >= +2 m)."""
    rng = np.random.default_rng(0)
    field = ObstacleField.random_cylinders(drones, cylinders, (-1.5, -1.5, 1.5, 1.5), (0.15, 0.3), (1.5, 2.5), rng)
    start = np.stack([np.full(drones, -2.5), rng.uniform(-1.0, 1.0, drones), np.full(drones, 1.0)], axis=1)
    blind = avoid.fly(field, start, False, duration_sec, speed, device)
    hit, passed = fly_mppi(field, start, duration_sec, speed, device)
    print(f"[mppi.py] {drones} drones through {cylinders} cylinders each: no rule {100.0 * blind:.1f} % collided; "
          f"MPPI {100.0 * hit:.1f} % collided, {100.0 * passed:.1f} % passed x >= {PASSED_X:+.0f} m")
    return blind, hit, passed


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=4096)
    ap.add_argument("--cylinders", type=int, default=6)
    ap.add_argument("--duration_sec", type=float, default=8)
    a = ap.parse_args()
    run(drones=a.drones, cylinders=a.cylinders, duration_sec=a.duration_sec)

#!/usr/bin/env python3
"""Obstacle-avoidance demo: N drones (`VectorVelocityAviary`: velocity commands tracked by the embedded DSLPID controllers), each in an
aviary of its own with a random course of cylinders, fly along +x -- once blindly and once steered by a rule on top of the obstacle
queries: repulsion along the `clearance()` normal of the nearest cylinder, and a side step towards the freer side of a forward
`range_scan()` fan.  The rule is a handful of torch operations on the device; `obstacle_hits()` counts who touched a cylinder.

Usage:  python examples/avoid.py [--drones 4096]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd.envs import VectorVelocityAviary  # noqa: E402
from gym_pybullet_drones_amd.obstacles import ObstacleField, fan  # noqa: E402

LOOK = 1.5          # m: range of the forward fan
INFLUENCE = 0.5     # m: clearance below which the nearest cylinder pushes


def avoidance_rule(env, rays, left, right):
    """(E, 2) correction of the horizontal velocity command: slow down and step to the freer side of the fan in proportion to how
    close the nearest return is, and move away from the nearest obstacle when it is closer than INFLUENCE."""
    near = 1.0 - env.range_scan(rays, LOOK, frame="world")[:, 0, :] / LOOK          # (E, R): 0 nothing in sight .. 1 touching
    ahead = near.max(dim=1).values
    side = torch.where((near * left).sum(dim=1) > (near * right).sum(dim=1), -1.0, 1.0)
    c = env.clearance()
    push = ((INFLUENCE - c.dist[:, 0]) / INFLUENCE).clamp(0.0, 1.0)
    away = c.normal[:, 0, :2] * (2.0 * push).unsqueeze(-1)
    return torch.stack([-0.5 * ahead, 1.5 * side * ahead], dim=1) + away


def fly(field, start, with_rule, duration_sec, speed, device):
    n = len(start)
    env = VectorVelocityAviary(n, 1, initial_xyzs=start[:, None, :], pyb_freq=240, ctrl_freq=48, device=device)
    env.reset()
    env.set_obstacles(field)
    rays = torch.as_tensor(fan(7, math.pi / 2), device=env.device)                  # +-45 degrees about the direction of travel
    left, right = (rays[:, 1] > 1e-6).float(), (rays[:, 1] < -1e-6).float()
    z0 = torch.as_tensor(start[:, 2], dtype=torch.float32, device=env.device)
    collided = torch.zeros(n, dtype=torch.bool, device=env.device)
    action = torch.zeros((n, 1, 4), dtype=torch.float32, device=env.device)
    action[..., 3] = speed
    for _ in range(int(duration_sec * env.CTRL_FREQ)):
        pos = env.core.positions()
        v = torch.zeros((n, 3), dtype=torch.float32, device=env.device)
        v[:, 0] = 1.0
        v[:, 2] = z0 - pos[:, 2]                                                    # hold the height
        if with_rule:
            v[:, :2] += avoidance_rule(env, rays, left, right)
        action[:, 0, :3] = v
        env.step(action)
        collided |= env.obstacle_hits()[:, 0]
    share = float(collided.float().mean())
    env.close()
    return share


def run(drones=4096, cylinders=6, duration_sec=8, speed=3.0, device="cuda:0"):
    """`speed`: the command as a multiple of the airframe's SPEED_LIMIT (0.25 m/s for the CF2X).  Returns the share of drones that
    touched a cylinder without the rule and with it."""
    rng = np.random.default_rng(0)
    field = ObstacleField.random_cylinders(drones, cylinders, (-1.5, -1.5, 1.5, 1.5), (0.15, 0.3), (1.5, 2.5), rng)
    start = np.stack([np.full(drones, -2.5), rng.uniform(-1.0, 1.0, drones), np.full(drones, 1.0)], axis=1)
    out = {}
    for with_rule in (False, True):
        out[with_rule] = fly(field, start, with_rule, duration_sec, speed, device)
        print(f"[avoid.py] {drones} drones through {cylinders} cylinders each, {'repulsion + forward scan' if with_rule else 'no rule'}: "
              f"{100.0 * out[with_rule]:.1f} % collided")
    return out[False], out[True]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=4096)
    ap.add_argument("--cylinders", type=int, default=6)
    ap.add_argument("--duration_sec", type=float, default=8)
    a = ap.parse_args()
    run(drones=a.drones, cylinders=a.cylinders, duration_sec=a.duration_sec)

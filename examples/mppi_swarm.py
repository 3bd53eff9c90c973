#!/usr/bin/env python3
"""Sampling-based MPC for drones that share one airspace: N drones on a circle of radius 2 m at one height, each sent to the antipodal
point, so that every straight line passes through the centre.  Flown at 48 Hz on velocity commands, twice from the same starts:
once with `VectorAviary.mppi` -- every drone plans as if it were alone -- and once with `VectorAviary.mppi_swarm`, where every plan
also keeps the drone away from where its nearest peers last published they would be and publishes its own path in turn
(`gpd_mppi_peers`: one launch per plan for all drones, no trajectory in memory).  The physics of the single-drone aviaries knows no
contact, so a collision is counted, not suffered: per step one neighbour search over all drones.  Keeping apart costs time: the
drones that see each other go round the crowd at the centre, and some are still on their way when the blind ones have long arrived.

Usage:  python examples/mppi_swarm.py [--drones 64]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd.envs import VectorVelocityAviary  # noqa: E402
from gym_pybullet_drones_amd.mppi import MPPICost  # noqa: E402
from gym_pybullet_drones_amd.neighbors import WorldSearch  # noqa: E402

RADIUS = 2.0        # m: the circle
HEIGHT = 1.0        # m
SPEED = 3.0         # the largest speed fraction a sample may command (x SPEED_LIMIT: 0.75 m/s on the cf2x)
ARRIVED = 0.3       # m: "at the goal"


def fly(start, goal, swarm, duration_sec, device, horizon=24, samples=256, k=8, seed=0, sigma=(0.4, 0.4, 0.15, 0.5), lam=0.02, cost=None,
        w_peer=1000.0):
    """(share of drones that ever came closer than 2 COLLISION_R to another, share that ended within ARRIVED of its goal)"""
    n = len(start)
    env = VectorVelocityAviary(n, 1, initial_xyzs=start[:, None, :], pyb_freq=240, ctrl_freq=48, device=device)
    env.reset()
    core = env.core
    cost = MPPICost(w_pos=1.0, w_vel=0.1, w_tilt=0.5, w_rate=0.002, w_term=4.0) if cost is None else cost
    common = dict(sigma=sigma, lam=lam, cost=cost, seed=seed, act_lo=(-1.0, -1.0, -1.0, 0.0), act_hi=(1.0, 1.0, 1.0, SPEED))
    if swarm:
        peer_dist = 2.0 * core.P.COLLISION_R + 0.3
        # two drones at the largest commanded speed close this much within the horizon
        reach = peer_dist + 2.0 * SPEED * core.P.SPEED_LIMIT * horizon / env.CTRL_FREQ
        planner = env.mppi_swarm(horizon, samples, k=k, radius=reach, w_peer=w_peer, peer_dist=peer_dist, **common)
    else:
        planner = env.mppi(horizon, samples, **common)
    g = torch.as_tensor(goal, dtype=torch.float32, device=env.device)
    touch = WorldSearch(env.device, n, 0, n, 2.0 * core.P.COLLISION_R, 1, (-RADIUS - 1.0, -RADIUS - 1.0, RADIUS + 1.0, RADIUS + 1.0), rel=False)
    collided = torch.zeros(n, dtype=torch.bool, device=env.device)
    for _ in range(int(duration_sec * env.CTRL_FREQ)):
        env.step(planner.plan(g).view(n, 1, 4))
        planner.advance()
        collided |= touch(core.kin_P, core._stream()).count > 0
    arrived = (core.positions() - g).norm(dim=1) < ARRIVED
    out = float(collided.float().mean()), float(arrived.float().mean())
    env.close()
    return out


def run(drones=64, duration_sec=20, device="cuda:0", **planner):
    """Returns (hit_blind, goal_blind, hit_swarm, goal_swarm): for the flight blind to the peers and for the one that sees them, the
    share of drones that ever came closer than 2 COLLISION_R to another and the share that ended within 0.3 m of its goal."""
    phi = 2.0 * np.pi * np.arange(drones) / drones
    start = np.stack([RADIUS * np.cos(phi), RADIUS * np.sin(phi), np.full(drones, HEIGHT)], axis=1)
    goal = start * np.array([-1.0, -1.0, 1.0])
    hit_blind, goal_blind = fly(start, goal, False, duration_sec, device, **planner)
    hit_swarm, goal_swarm = fly(start, goal, True, duration_sec, device, **planner)
    print(f"[mppi_swarm.py] {drones} drones across a circle of {RADIUS:.0f} m: blind to each other {100.0 * hit_blind:.1f} % collided "
          f"({100.0 * goal_blind:.1f} % at the goal); with the peers' paths in the cost {100.0 * hit_swarm:.1f} % collided "
          f"({100.0 * goal_swarm:.1f} % at the goal)")
    return hit_blind, goal_blind, hit_swarm, goal_swarm


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=64)
    ap.add_argument("--duration_sec", type=float, default=20)
    a = ap.parse_args()
    run(drones=a.drones, duration_sec=a.duration_sec)

#!/usr/bin/env python3
"""Sampling-based MPC on airframes that are not the nominal one: N drones, each in an aviary of its own, each with its own mass (+-25 %)
and rotor constant KF (+-15 %) and with the drag term on (`VectorCtrlAviary(randomize=..., physics=Physics.PYB_DRAG)`), fly on thrust and
body-rate commands at 48 Hz over the 240 Hz rate loop to a goal 1 m away and hold it.  The heaviest drone with the weakest rotors hovers
at the thrust command (s_m / s_kf) g = 1.47 g = 14.4 m/s^2, far inside the controller's clip of 40.9 m/s^2.

The same flight three times from the same seeds:
  model="nominal"          the planner's model is the nominal airframe without drag: a drone 20 % heavier is planned for as if it
                           hovered at g, and hangs below the goal
  model="aviary"           the planner's model is the aviary's own: every drone's row of the plant table, and the drag term
  model="aviary", plant=   the planner believes the opposite of the truth (a heavy drone light, weak rotors strong): what a wrong
                           identification costs -- and where a right one (examples/sysid.py) goes
Printed: the population's mean distance to the goal over the last second of each flight.

Usage:  python examples/mppi_randomized.py [--drones 128]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd._native import SCALE_FIELDS  # noqa: E402
from gym_pybullet_drones_amd.control import VectorCTBR  # noqa: E402
from gym_pybullet_drones_amd.envs import VectorCtrlAviary  # noqa: E402
from gym_pybullet_drones_amd.mppi import MPPICost  # noqa: E402
from gym_pybullet_drones_amd.utils.enums import Physics  # noqa: E402

RANGES = {"mass": 0.25, "kf": 0.15}
GOAL = (0.8, 0.0, 0.6)          # relative to the start: 1 m away


def fly(drones, model, wrong, duration_sec, device, horizon=24, samples=256, sigma=(2.0, 2.0, 2.0, 0.5), lam=0.05, seed=0):
    """the mean distance to the goal over the last second; `wrong`: plan on the mirrored belief 2 - s in place of the truth s"""
    start = np.zeros((drones, 1, 3))
    start[:, 0, 2] = 1.0
    env = VectorCtrlAviary(drones, 1, initial_xyzs=start, physics=Physics.PYB_DRAG, pyb_freq=240, ctrl_freq=48, randomize=RANGES, device=device)
    env.reset(seed=seed)
    ctrl = VectorCTBR(drones, device=env.device)
    cost = MPPICost(w_pos=1.0, w_vel=0.05, w_tilt=0.5, w_rate=0.002, w_term=4.0)
    belief = None
    if wrong:
        truth = env.core.plant_view()[:, :, 0]
        belief = {k: 2.0 - truth[SCALE_FIELDS.index(k)] for k in RANGES}
    planner = env.mppi_ctbr(ctrl, horizon, samples, sigma=sigma, lam=lam, cost=cost, seed=seed, model=model, plant=belief)
    goal = torch.as_tensor(start[:, 0] + np.asarray(GOAL), dtype=torch.float32, device=env.device)
    steps, last = int(duration_sec * env.CTRL_FREQ), int(env.CTRL_FREQ)
    dist = torch.zeros((), device=env.device)
    for t in range(steps):
        env.rollout_ctbr(ctrl, planner.plan(goal), 1, mode="cmd", last_only=True)
        planner.advance()
        if t >= steps - last:
            dist += (env.core.positions()[:, :3] - goal).norm(dim=1).mean()
    out = float(dist) / last
    env.close()
    return out


def run(drones=128, duration_sec=6, device="cuda:0", **planner):
    """Returns the mean distance to the goal over the last second [m] of (model="nominal", model="aviary", a wrong belief)."""
    nominal = fly(drones, "nominal", False, duration_sec, device, **planner)
    aviary = fly(drones, "aviary", False, duration_sec, device, **planner)
    wrong = fly(drones, "aviary", True, duration_sec, device, **planner)
    print(f"[mppi_randomized.py] {drones} drones, mass +-{100 * RANGES['mass']:.0f} %, KF +-{100 * RANGES['kf']:.0f} %, drag on; mean distance "
          f"to the goal over the last second: planned on the nominal airframe {nominal:.3f} m, on the aviary's own model {aviary:.3f} m, "
          f"on a wrong belief {wrong:.3f} m")
    return nominal, aviary, wrong


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=128)
    ap.add_argument("--duration_sec", type=float, default=6)
    a = ap.parse_args()
    run(drones=a.drones, duration_sec=a.duration_sec)

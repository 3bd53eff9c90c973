#!/usr/bin/env python3
"""The hover task flown on thrust and body-rate commands: N single-drone aviaries, `VectorCTBRAviary.step()` closed-loop -- one launch per
step does the rate loop inside the physics sub-steps, the reward, the episode ends and the auto-reset.  The commands come from the
controller's own outer loop (`VectorCTBR.compute` on the core's state, the reference's `CTBRControl.computeControl`), mapped into the
aviary's [-1, 1] action space; beside it the idle action a = 0 (the hover command: the drone stays where its episode started).  Prints
the mean episode return, the share of episodes ended by the box (out of bounds or tilted, before the clock) and the mean episode length.

Usage:  python examples/ctbr_task.py [--drones 128] [--duration_sec 9]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd.envs import VectorCTBRAviary  # noqa: E402

EPISODE_SEC = 4.0


def fly(start, controlled, duration_sec, device):
    """-> (mean return, share of episodes ended by the box, mean length in steps) over the episodes that finished"""
    n = len(start)
    env = VectorCTBRAviary(n, initial_xyzs=start[:, None, :], episode_len_sec=EPISODE_SEC, device=device)
    env.reset()
    core, target = env.core, env.core.target.expand(n, 3).contiguous()
    full = int(EPISODE_SEC * env.CTRL_FREQ) + 1            # steps of an episode that only the clock ends
    ret, length = torch.zeros(n, device=env.device), torch.zeros(n, device=env.device)
    sums = torch.zeros(4, device=env.device)               # episodes, their returns, their lengths, those the box ended
    idle = torch.zeros((n, 1, 4), device=env.device)
    for _ in range(int(duration_sec * env.CTRL_FREQ)):
        if controlled:
            cmd = env.ctrl.compute(core.positions(), core.quaternions(), core.velocities(), target)
            action = env.action_of(cmd).clamp(-1.0, 1.0).unsqueeze(1)
        else:
            action = idle
        _, reward, terminated, truncated, _ = env.step(action)
        ret += reward
        length += 1.0
        done = (terminated | truncated).float()
        early = done * (length < full).float() * (~terminated).float()
        sums += torch.stack([done.sum(), (done * ret).sum(), (done * length).sum(), early.sum()])
        ret *= 1.0 - done
        length *= 1.0 - done
    episodes, returns, lengths, boxed = sums.tolist()
    env.close()
    episodes = max(episodes, 1.0)
    return returns / episodes, boxed / episodes, lengths / episodes


def run(drones=128, duration_sec=9.0, device="cuda:0"):
    """Returns ((return, boxed share, length) of the controller, the same of the idle action)."""
    rng = np.random.default_rng(0)
    start = np.stack([rng.uniform(-0.5, 0.5, drones), rng.uniform(-0.5, 0.5, drones), rng.uniform(0.2, 0.6, drones)], axis=1)
    out = {}
    for controlled in (True, False):
        out[controlled] = fly(start, controlled, duration_sec, device)
        r, b, l = out[controlled]
        print(f"[ctbr_task.py] {drones} aviaries, {duration_sec:g} s, {'outer loop -> actions' if controlled else 'idle action a = 0'}: "
              f"mean episode return {r:.2f}, ended by the box {100.0 * b:.1f} %, mean episode length {l:.1f} steps")
    return out[True], out[False]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--drones", type=int, default=128)
    ap.add_argument("--duration_sec", type=float, default=9.0)
    a = ap.parse_args()
    run(drones=a.drones, duration_sec=a.duration_sec)

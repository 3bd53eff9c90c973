#!/usr/bin/env python3
"""Analytic policy gradients on thrust and body-rate commands: `.backward()` through `rollout_diff_ctbr`
(gym_pybullet_drones_amd/diff.py) -- the two halves of examples/apg.py on the action space of agile flight, the rate loop closed inside
every physics sub-step.

(a) Gradient-based trajectory optimisation: Adam on the open-loop command sequences (thrust [m/s^2] | body rates [rad/s]) of E drones
    that start up to 0.3 m away from the waypoint -- one taped K-step launch forward, one reverse-sweep launch backward per iteration.
(b) A small torch MLP from obs12 to a command, trained by back-propagation through the flight: the policy runs as torch operations
    between K = 1 steps, `kin_K` of one call is `kin0` of the next, and the loss's gradient reaches the weights through every step.

Usage:  python examples/apg_ctbr.py [--num_envs 4096] [--horizon 24]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd.control import VectorCTBR  # noqa: E402
from gym_pybullet_drones_amd.envs import VectorCtrlAviary  # noqa: E402

WAYPOINT = (0.0, 0.0, 1.0)
HOVER = 9.8             # the thrust command [m/s^2] that holds a level drone


def tracking_loss(pos, vel, target):
    """mean |p - target|^2 + 0.01 mean |v|^2"""
    return ((pos - target) ** 2).sum(-1).mean() + 0.01 * (vel ** 2).sum(-1).mean()


def command(u):
    """a network's or an optimiser's unit-scale output [.., 4] -> thrust around hover (+-5 m/s^2) | body rates (+-2 rad/s)"""
    return torch.cat([HOVER + 5.0 * u[..., 0:1], 2.0 * u[..., 1:4]], dim=-1)


def run(num_envs=4096, horizon=24, traj_iters=40, policy_iters=40, device="cuda:0", seed=0, verbose=True):
    rng = np.random.default_rng(seed)
    start = np.array(WAYPOINT) + rng.uniform(-0.3, 0.3, size=(num_envs, 1, 3))
    env = VectorCtrlAviary(num_envs, initial_xyzs=start, pyb_freq=240, ctrl_freq=48, device=device)
    env.reset()
    core, dev = env.core, env.device
    ctrl = VectorCTBR(num_envs, device=dev)
    kin0 = core.kin_store.clone()                              # the plane layout of the state (diff.pack_kin / unpack_kin)
    target = torch.tensor(WAYPOINT, device=dev)

    # (a) open-loop command sequences
    u = torch.zeros((horizon, num_envs, 4), device=dev, requires_grad=True)
    opt = torch.optim.Adam([u], lr=0.05)
    traj = []
    for _ in range(traj_iters):
        opt.zero_grad()
        obs, _ = core.rollout_diff_ctbr(ctrl, command(u), kin0)
        loss = tracking_loss(obs[..., 0:3], obs[..., 6:9], target)
        loss.backward()
        opt.step()
        traj.append(float(loss.detach()))
    if verbose:
        print(f"[apg_ctbr.py] trajectory optimisation, {num_envs} drones x {horizon} steps: loss {traj[0]:.4f} -> {traj[-1]:.4f}")

    # (b) a closed-loop policy from obs12 to a command, back-propagated through K = 1 steps
    torch.manual_seed(seed)
    policy = torch.nn.Sequential(torch.nn.Linear(12, 32), torch.nn.Tanh(), torch.nn.Linear(32, 4), torch.nn.Tanh()).to(dev)
    opt = torch.optim.Adam(policy.parameters(), lr=1e-2)
    obs0 = torch.cat([torch.tensor(start[:, 0], dtype=torch.float32, device=dev), torch.zeros((num_envs, 9), device=dev)], dim=1)
    hist = []
    for _ in range(policy_iters):
        opt.zero_grad()
        kin, o, loss = kin0, obs0, 0.0
        for _ in range(horizon):
            cmd = command(policy(torch.cat([o[:, 0:3] - target, o[:, 3:12]], dim=1)))
            obs, kin = core.rollout_diff_ctbr(ctrl, cmd.unsqueeze(0), kin)
            o = obs[0]
            loss = loss + tracking_loss(o[:, 0:3], o[:, 6:9], target) / horizon
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    if verbose:
        print(f"[apg_ctbr.py] MLP policy through {horizon} differentiable steps: loss {hist[0]:.4f} -> {hist[-1]:.4f}")
    return traj, hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=24)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    run(args.num_envs, args.horizon, device=args.device)

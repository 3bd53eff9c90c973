#!/usr/bin/env python3
"""Analytic policy gradients: `.backward()` through the rollout kernel (`rollout_diff`, gym_pybullet_drones_amd/diff.py).

(a) Gradient-based trajectory optimisation: Adam on the open-loop RPM sequences of E drones that start up to 0.3 m away from the
    hover target -- one taped K-step launch forward, one reverse-sweep launch backward per iteration.
(b) A small torch MLP trained by back-propagation through the physics: the policy runs as torch operations between K = 1 steps,
    `kin_K` of one call is `kin0` of the next, and the loss's gradient reaches the weights through every step.

Usage:  python examples/apg.py [--num_envs 4096] [--horizon 30]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd.diff import unpack_kin  # noqa: E402
from gym_pybullet_drones_amd.envs import VectorHoverAviary  # noqa: E402
from gym_pybullet_drones_amd.utils.enums import ActionType  # noqa: E402

TARGET = (0.0, 0.0, 1.0)


def tracking_loss(pos, vel, target):
    """mean |p - target|^2 + 0.01 mean |v|^2"""
    return ((pos - target) ** 2).sum(-1).mean() + 0.01 * (vel ** 2).sum(-1).mean()


def run(num_envs=4096, horizon=30, traj_iters=40, policy_iters=40, device="cuda:0", seed=0, verbose=True):
    rng = np.random.default_rng(seed)
    start = np.array(TARGET) + rng.uniform(-0.3, 0.3, size=(num_envs, 1, 3))
    env = VectorHoverAviary(num_envs, act=ActionType.RPM, ctrl_freq=30, initial_xyzs=start, auto_reset=False, device=device)
    env.reset()
    core, dev = env.core, env.device
    kin0 = core.kin_store.clone()                              # the plane layout of the state (diff.pack_kin / unpack_kin)
    target = torch.tensor(TARGET, device=dev)

    # (a) open-loop sequences
    actions = torch.zeros((horizon, num_envs, 1, 4), device=dev, requires_grad=True)
    opt = torch.optim.Adam([actions], lr=0.1)
    traj = []
    for _ in range(traj_iters):
        opt.zero_grad()
        obs, _, _, _, _ = env.rollout_diff(actions, kin0)
        loss = tracking_loss(obs[..., 0:3], obs[..., 6:9], target)
        loss.backward()
        opt.step()
        traj.append(float(loss.detach()))
    if verbose:
        print(f"[apg.py] trajectory optimisation, {num_envs} drones x {horizon} steps: loss {traj[0]:.4f} -> {traj[-1]:.4f}")

    # (b) a closed-loop policy, back-propagated through K = 1 steps
    torch.manual_seed(seed)
    policy = torch.nn.Sequential(torch.nn.Linear(13, 32), torch.nn.Tanh(), torch.nn.Linear(32, 4), torch.nn.Tanh()).to(dev)
    opt = torch.optim.Adam(policy.parameters(), lr=1e-2)
    hist = []
    for _ in range(policy_iters):
        opt.zero_grad()
        kin, loss = kin0, 0.0
        for _ in range(horizon):
            pos, quat, vel, rates = unpack_kin(kin, num_envs)
            a = policy(torch.cat([pos - target, quat, vel, rates], dim=1))
            obs, _, kin, _, _ = core.rollout_diff(a.unsqueeze(0), kin)
            loss = loss + tracking_loss(obs[0, :, 0:3], obs[0, :, 6:9], target) / horizon
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    if verbose:
        print(f"[apg.py] MLP policy through {horizon} differentiable steps: loss {hist[0]:.4f} -> {hist[-1]:.4f}")
    return traj, hist


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    run(args.num_envs, args.horizon, device=args.device)

#!/usr/bin/env python3
"""What one MPPI plan over thrust and body-rate commands costs, and what it is measured against.

    python profiles/mppi_ctbr_bench.py [--out profiles/mppi_ctbr_mi355x.json]

The workload of profiles/mppi_bench.py on CTBR commands: 4 096 drones (48 Hz commands over 240 Hz physics, the body-rate loop in every
sub-step), 256 samples each, a horizon of 24 steps, 6 cylinders per aviary (the course of examples/avoid.py).  Timed with device events
in ONE process, in turns, each until it has run for at least 0.25 s after warm-up:
  fused      `gpd_mppi_ctbr` through `mppi.CTBRMPPI.plan`: one launch
  composed   the same plan from the entries the library had before: the state tiled 256 times into a core of 1 048 576 aviaries,
             torch.randn noise and the clamp, ONE `gpd_rollout_ctbr` of 24 steps in "cmd" mode with observations out, `gpd_obstacles`
             once per step on that step's positions, the cost and the softmax update in torch
  fused_vel  `gpd_mppi` over velocity commands on the same course (profiles/mppi_bench.py's planner), for scale
No time is a pass condition.  The two ways draw different noise, so they are compared without any (sigma = 0: the costs of the nominal)
before either is timed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd import engine, mppi, obstacles as ob  # noqa: E402
from gym_pybullet_drones_amd.control import VectorCTBR  # noqa: E402
from gym_pybullet_drones_amd.utils.enums import DroneModel  # noqa: E402

N, M, H, CYLINDERS, MIN_SECONDS = 4096, 256, 24, 6, 0.25
SIGMA, LAM, AHEAD = (2.0, 3.0, 3.0, 0.5), 0.05, 1.5
COST = mppi.MPPICost(w_pos=1.0, w_vel=0.05, w_tilt=0.5, w_rate=0.002, w_term=4.0, w_obs=300.0, obst_margin=0.35)
VEL = dict(sigma=(0.4, 0.4, 0.15, 0.5), lam=0.05, lo=(-1.0, -1.0, -1.0, 0.0), hi=(1.0, 1.0, 1.0, 3.0),
           cost=mppi.MPPICost(w_pos=0.3, w_vel=0.05, w_tilt=0.5, w_rate=0.002, w_term=4.0, w_obs=300.0, obst_margin=0.35))


def make_core(n, dev, start, act_code=mppi.ACT_DIRECT_RPM):
    return engine.SimCore(drone_model=DroneModel.CF2X, num_envs=n, drones_per_env=1, physics=0, pyb_freq=240, ctrl_freq=48, act_code=act_code,
                          task=engine.TASK_NONE, initial_xyzs=start[:, None, :], auto_reset=False, track_rpm=False, device=dev)


class Composed:
    """the plan from gpd_rollout_ctbr + gpd_obstacles + torch"""

    def __init__(self, small, ctrl, field, goal, dev):
        self.small, self.dev = small, dev
        rec = np.repeat(field.records(), M, axis=0)                                   # [N * M, CYLINDERS, 8]: every sample its drone's list
        tiled = ob.ObstacleField(N * M)
        for m in range(rec.shape[1]):
            tiled.cylinder(rec[:, m, 0:3], rec[:, m, 4], rec[:, m, 6])
        self.big = make_core(N * M, dev, np.zeros((N * M, 3)))
        self.ctrl = VectorCTBR(N * M, device=dev, k_rate=ctrl.k_rate, thrust_max=ctrl.thrust_max, rate_max=ctrl.rate_max)
        self.query = ob.FieldQuery(tiled, dev, N * M, 1, small.P.COLLISION_R)
        self.pos4 = torch.zeros((N * M, 4), device=dev)
        self.goal = goal.repeat_interleave(M, dim=0)
        self.sigma = torch.tensor(SIGMA, device=dev)
        r = ctrl.rate_max
        self.lo, self.hi = torch.tensor((0.0, -r, -r, -r), device=dev), torch.tensor((ctrl.thrust_max, r, r, r), device=dev)
        self.radius = small.P.COLLISION_R

    def plan(self, u, sigma_scale=1.0):
        """u [H, N, 4] -> (u_out, costs [N, M])"""
        s, b = self.small, self.big
        for src, dst in ((s.kin_P, b.kin_P), (s.kin_Q, b.kin_Q), (s.kin_V, b.kin_V)):
            dst[:N * M] = src[:N].repeat_interleave(M, dim=0)
        b.kin_W[:N * M] = s.kin_W[:N].repeat_interleave(M)
        ut = u.repeat_interleave(M, dim=1)                                            # [H, N * M, 4]
        a = torch.minimum(torch.maximum(ut + (sigma_scale * self.sigma) * torch.randn_like(ut), self.lo), self.hi)
        obs = b.rollout_ctbr(self.ctrl, a, H, mode="cmd")                              # [H, N * M, 12]
        S = torch.zeros(N * M, device=self.dev)
        for h in range(H):
            o = obs[h]
            self.pos4[:, :3] = o[:, 0:3]
            d = self.query.clearance(self.pos4, b._stream()).dist
            wp = COST.w_pos * (COST.w_term if h == H - 1 else 1.0)
            S += wp * ((o[:, 0:3] - self.goal) ** 2).sum(-1) + COST.w_vel * (o[:, 6:9] ** 2).sum(-1) + COST.w_rate * (o[:, 9:12] ** 2).sum(-1) \
                + COST.w_tilt * (1.0 - torch.cos(o[:, 3]) * torch.cos(o[:, 4])) + COST.w_obs * (COST.obst_margin - (d - self.radius)).clamp_min(0.0) ** 2
        S = S.view(N, M)
        w = torch.softmax(-S / LAM, dim=1)
        du = (a - ut).view(H, N, M, 4)
        return u + (w[None, :, :, None] * du).sum(dim=2), S


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    field = ob.ObstacleField.random_cylinders(N, CYLINDERS, (-1.5, -1.5, 1.5, 1.5), (0.15, 0.3), (1.5, 2.5), rng)
    start = np.stack([rng.uniform(-2.5, 1.5, N), rng.uniform(-1.0, 1.0, N), np.full(N, 1.0)], axis=1)          # somewhere along the course
    small, ctrl = make_core(N, dev, start), VectorCTBR(N, device=dev)
    goal = torch.as_tensor(np.stack([np.minimum(3.5, start[:, 0] + AHEAD), start[:, 1], start[:, 2]], axis=1), dtype=torch.float32, device=dev)
    planner = mppi.CTBRMPPI(small, ctrl, H, M, SIGMA, LAM, cost=COST, seed=1, field=field)
    for _ in range(10):                                       # a moving, tilted state: ten planned steps
        small.rollout_ctbr(ctrl, planner.plan(goal), 1, mode="cmd", last_only=True)
        planner.advance()
    composed = Composed(small, ctrl, field, goal, dev)
    u = planner.nominal.clone()
    # without noise both ways score the nominal: the same costs
    quiet = mppi.CTBRMPPI(small, ctrl, H, M, (0.0,) * 4, LAM, cost=COST, seed=1, field=field)
    quiet.nominal[:] = u
    quiet.plan(goal)
    _, S = composed.plan(u, sigma_scale=0.0)
    agree = float(((quiet.costs - S).abs() / S.abs().clamp_min(1.0)).max())
    assert agree < 1e-4, agree
    # gpd_mppi over velocity commands on the same course, for scale (the planner profiles/mppi_bench.py times)
    vel_core = make_core(N, dev, start, act_code=mppi.ACT_VEL)
    vel = mppi.MPPI(vel_core, H, M, VEL["sigma"], VEL["lam"], cost=VEL["cost"], seed=1, field=field, act_lo=VEL["lo"], act_hi=VEL["hi"])
    vel.reset(value=(1.0, 0.0, 0.0, 3.0))
    vel_goal = torch.as_tensor(np.stack([np.full(N, 3.5), start[:, 1], start[:, 2]], axis=1), dtype=torch.float32, device=dev)
    for _ in range(10):
        vel_core.step(vel.plan(vel_goal).contiguous())
        vel.advance()
    jobs = {"fused": (lambda: planner.plan(goal), 20), "composed": (lambda: composed.plan(u), 1), "fused_vel": (lambda: vel.plan(vel_goal), 20)}
    for fn, _ in jobs.values():
        fn()
    torch.cuda.synchronize()
    spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)
    while min(spent.values()) < MIN_SECONDS:                 # in turns: what drifts, drifts for all
        for name, (fn, calls) in jobs.items():
            if spent[name] < MIN_SECONDS:
                spent[name] += timed(fn, calls)
                done[name] += calls
    per = {k: spent[k] / done[k] for k in jobs}
    res = {"device": torch.cuda.get_device_name(0), "drones": N, "samples": M, "horizon": H, "substeps": small.S, "cylinders_per_aviary": CYLINDERS,
           "act": "ctbr", "costs_agree_without_noise": agree, "per_plan_us": {k: v * 1e6 for k, v in per.items()},
           "sample_steps_per_s": {k: N * M * H / v for k, v in per.items()}, "fused_speedup": per["composed"] / per["fused"],
           "ctbr_over_vel": per["fused"] / per["fused_vel"], "effective_sample_size_mean": float(planner.stats[:, 2].mean()), "calls": done,
           "seconds_timed": {k: round(v, 3) for k, v in spent.items()}}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()

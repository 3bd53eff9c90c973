#!/usr/bin/env python3
"""What one MPPI plan against the peers' published paths costs, and what it is measured against.

    python profiles/mppi_swarm_bench.py [--out profiles/mppi_swarm_mi355x.json]

4 096 drones in ONE airspace of 40 m x 40 m x 2 m (about nine peers within the search radius of 1.2 m), velocity commands at 48 Hz over
240 Hz physics, 256 samples each, a horizon of 24 steps, the 8 nearest peers, 6 cylinders shared by all.  Timed with device events in
ONE process, in turns, each until it has run for at least 0.25 s after warm-up:
  swarm        `gpd_mppi_peers` with path_out through `mppi.SwarmMPPI.plan`: the neighbour search, one launch, the table swap
  swarm_bare   the launch alone, without path_out (the lists and the table as they are)
  swarm_launch the launch alone, with path_out
  blind        `gpd_mppi` at the same shape through `mppi.MPPI.plan`: the parent's planner; swarm_launch / blind is the price of the
               peer term and the path
  composed     the same plan from the entries the library had before: the state tiled 256 times into a core of 1 048 576 aviaries,
               torch.randn noise and the clamp, ONE `gpd_rollout` of 24 steps with observations out, `gpd_obstacles` once per step, the
               peers' rows gathered and the hinge, the cost and the softmax update in torch (as profiles/mppi_bench.py composes its own)
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

from gym_pybullet_drones_amd import _native, engine, mppi, obstacles as ob  # noqa: E402
from gym_pybullet_drones_amd.utils.enums import DroneModel  # noqa: E402

N, M, H, K, CYLINDERS, MIN_SECONDS = 4096, 256, 24, 8, 6, 0.25
SIGMA, LAM, SPEED = (0.4, 0.4, 0.15, 0.5), 0.05, 3.0
LO, HI = (-1.0, -1.0, -1.0, 0.0), (1.0, 1.0, 1.0, SPEED)
COST = mppi.MPPICost(w_pos=0.3, w_vel=0.05, w_tilt=0.5, w_rate=0.002, w_term=4.0, w_obs=300.0, obst_margin=0.35)
W_PEER, SIDE = 300.0, 40.0


def make_core(n, dev, start):
    return engine.SimCore(drone_model=DroneModel.CF2X, num_envs=n, drones_per_env=1, physics=0, pyb_freq=240, ctrl_freq=48, act_code=mppi.ACT_VEL,
                          task=engine.TASK_NONE, initial_xyzs=start[:, None, :], auto_reset=False, track_rpm=False, device=dev)


class Composed:
    """the plan from gpd_rollout + gpd_obstacles + torch"""

    def __init__(self, small, field, goal, peer_dist, dev):
        self.small, self.dev, self.peer_dist = small, dev, peer_dist
        self.big = make_core(N * M, dev, np.zeros((N * M, 3)))
        self.query = ob.FieldQuery(field, dev, N * M, 1, small.P.COLLISION_R)
        self.pos4 = torch.zeros((N * M, 4), device=dev)
        self.goal = goal.repeat_interleave(M, dim=0)
        self.sigma, self.lo, self.hi = (torch.tensor(v, device=dev) for v in (SIGMA, LO, HI))
        self.radius = small.P.COLLISION_R

    def plan(self, u, idx, table, sigma_scale=1.0):
        """u [H, N, 4], idx [N, K], table [H, N, 4] -> (u_out, costs [N, M])"""
        s, b = self.small, self.big
        for src, dst in ((s.kin_P, b.kin_P), (s.kin_Q, b.kin_Q), (s.kin_V, b.kin_V)):
            dst[:N * M] = src[:N].repeat_interleave(M, dim=0)
        b.kin_W[:N * M] = s.kin_W[:N].repeat_interleave(M)
        b.pid[:, :N * M] = s.pid[:, :N].repeat_interleave(M, dim=1)
        ut = u.repeat_interleave(M, dim=1)                                            # [H, N * M, 4]
        a = torch.minimum(torch.maximum(ut + (sigma_scale * self.sigma) * torch.randn_like(ut), self.lo), self.hi)
        obs = b.rollout(a, update_latest=False)[0]                                    # [H, N * M, 12]
        live, rows = (idx >= 0)[:, None, :], idx.clamp_min(0).long()
        S = torch.zeros(N * M, device=self.dev)
        for h in range(H):
            o = obs[h]
            self.pos4[:, :3] = o[:, 0:3]
            d = self.query.clearance(self.pos4, b._stream()).dist
            wp = COST.w_pos * (COST.w_term if h == H - 1 else 1.0)
            S += wp * ((o[:, 0:3] - self.goal) ** 2).sum(-1) + COST.w_vel * (o[:, 6:9] ** 2).sum(-1) + COST.w_rate * (o[:, 9:12] ** 2).sum(-1) \
                + COST.w_tilt * (1.0 - torch.cos(o[:, 3]) * torch.cos(o[:, 4])) + COST.w_obs * (COST.obst_margin - (d - self.radius)).clamp_min(0.0) ** 2
            gap = (o[:, 0:3].view(N, M, 1, 3) - table[h, :, :3][rows][:, None]).norm(dim=-1)          # [N, M, K]
            S += W_PEER * (((self.peer_dist - gap).clamp_min(0.0) ** 2) * live).sum(-1).view(-1)
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


def launch(p, goal, path):
    """the entry alone on the planner's tensors as they are (nothing swapped, nothing counted)"""
    c, r = p.core, p._r
    r.pos, r.path_out = p._paths[0].data_ptr(), (p._paths[1].data_ptr() if path else None)
    obst, n_obst, ld = p._obst
    _native.call("gpd_mppi_peers", p.device, c._stream(), c._params, None, c._state, p._cfg, p._q, r, p._u[0], N * 4, goal, 0, obst, n_obst, ld,
                 p._u[1], p.costs, p.stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    field = ob.ObstacleField()
    for _ in range(CYLINDERS):
        field.cylinder((rng.uniform(-SIDE / 2, SIDE / 2), rng.uniform(-SIDE / 2, SIDE / 2), 1.0), rng.uniform(0.5, 1.5), 2.0)
    start = np.stack([rng.uniform(-SIDE / 2, SIDE / 2, N), rng.uniform(-SIDE / 2, SIDE / 2, N), rng.uniform(1.0, 3.0, N)], axis=1)
    goal_np = start + np.concatenate([rng.uniform(-3.0, 3.0, (N, 2)), np.zeros((N, 1))], axis=1)
    small, blind_core = make_core(N, dev, start), make_core(N, dev, start)
    goal = torch.zeros((N, 4), device=dev)
    goal[:, :3] = torch.as_tensor(goal_np, dtype=torch.float32)
    kw = dict(cost=COST, seed=1, field=field, act_lo=LO, act_hi=HI)
    peer_dist = 2.0 * small.P.COLLISION_R + 0.3
    reach = peer_dist + 2.0 * SPEED * small.P.SPEED_LIMIT * H / 48.0
    planner = mppi.SwarmMPPI(small, H, M, SIGMA, LAM, k=K, radius=reach, w_peer=W_PEER, peer_dist=peer_dist, **kw)
    blind = mppi.MPPI(blind_core, H, M, SIGMA, LAM, **kw)
    for p, core in ((planner, small), (blind, blind_core)):
        for _ in range(10):                                   # a moving, tilted state: ten planned steps
            core.step(p.plan(goal[:, :3]).contiguous())
            p.advance()
    composed = Composed(small, field, goal[:, :3], peer_dist, dev)
    u = planner.nominal.clone()
    # without noise both ways score the nominal against the same lists and table: the same costs
    quiet = mppi.SwarmMPPI(small, H, M, (0.0,) * 4, LAM, k=K, radius=reach, w_peer=W_PEER, peer_dist=peer_dist, **kw)
    quiet.nominal[:] = u
    quiet.plan(goal[:, :3])
    idx, table = quiet._idx.clone(), quiet._paths[1].clone()                         # what that launch read
    _, S = composed.plan(u, idx, table, sigma_scale=0.0)
    agree = float(((quiet.costs - S).abs() / S.abs().clamp_min(1.0)).max())
    assert agree < 1e-4, agree
    peers_mean = float((idx >= 0).sum(dim=1).float().mean())
    jobs = {"swarm": (lambda: planner.plan(goal[:, :3]), 20), "swarm_bare": (lambda: launch(planner, goal, False), 20),
            "swarm_launch": (lambda: launch(planner, goal, True), 20), "blind": (lambda: blind.plan(goal[:, :3]), 20),
            "composed": (lambda: composed.plan(u, idx, table), 1)}
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
    res = {"device": torch.cuda.get_device_name(0), "drones": N, "samples": M, "horizon": H, "substeps": small.S, "k": K, "peers_mean": peers_mean,
           "cylinders_shared": CYLINDERS, "act": "vel", "costs_agree_without_noise": agree, "per_plan_us": {k: v * 1e6 for k, v in per.items()},
           "sample_steps_per_s": {k: N * M * H / v for k, v in per.items()}, "peer_term_over_blind": per["swarm_bare"] / per["blind"],
           "with_path_over_blind": per["swarm_launch"] / per["blind"], "fused_speedup": per["composed"] / per["swarm"],
           "effective_sample_size_mean": float(planner.stats[:, 2].mean()), "calls": done, "seconds_timed": {k: round(v, 3) for k, v in spent.items()}}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()

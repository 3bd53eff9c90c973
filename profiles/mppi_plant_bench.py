#!/usr/bin/env python3
"""What planning on the aviary's own model costs over planning on the nominal one.

    python profiles/mppi_plant_bench.py [--out profiles/mppi_plant_mi355x.json]

The workload of profiles/mppi_bench.py: 4 096 drones at 48 Hz over 240 Hz physics, 256 samples each, a horizon of 24 steps, 6 cylinders
per aviary, for RPM, VEL and CTBR actions.  Per action type five planners on the same state, nominal and course:
  own          `gpd_mppi` (RPM, VEL) / `gpd_mppi_ctbr`: the unchanged entries, the baseline
  plain        `gpd_mppi_plant` without a table and without flags (the same model through the new kernel)
  table        `gpd_mppi_plant` with a per-drone plant table (mass and KF +-20 %, the others +-10 %), no flags
  flags        `gpd_mppi_plant` with GPD_PHYS_GND | GPD_PHYS_DRAG, no table
  both         `gpd_mppi_plant` with the table and the flags
and, for VEL, `composed`: the plan of `both` from the entries the library had before -- the state, the last RPMs and the table tiled
256 times into a core of 1 048 576 aviaries, torch.randn noise and the clamp, ONE `gpd_rollout_plant` of 24 steps with observations
out, `gpd_obstacles` once per step, the cost and the softmax update in torch.
Timed with device events in ONE process, the entries in turns, every window at least 0.25 s after warm-up, five windows each: the
median.  No time is a pass condition.  Before anything is timed, `both` and `composed` are compared without noise (sigma = 0: the costs
of the nominal).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd import _native, engine, mppi, obstacles as ob  # noqa: E402
from gym_pybullet_drones_amd.control import VectorCTBR  # noqa: E402
from gym_pybullet_drones_amd.utils.enums import DroneModel  # noqa: E402

N, M, H, CYLINDERS, MIN_SECONDS, WINDOWS = 4096, 256, 24, 6, 0.25, 5
FLAGS = 1 | 2             # GPD_PHYS_GND | GPD_PHYS_DRAG
LAM = 0.05
COST = mppi.MPPICost(w_pos=1.0, w_vel=0.05, w_tilt=0.5, w_rate=0.002, w_term=4.0, w_obs=300.0, obst_margin=0.35)
ACTS = {"rpm": dict(code=mppi.ACT_RPM, sigma=(0.3, 0.3, 0.3, 0.3), lo=None, hi=None),
        "vel": dict(code=mppi.ACT_VEL, sigma=(0.4, 0.4, 0.15, 0.5), lo=(-1.0, -1.0, -1.0, 0.0), hi=(1.0, 1.0, 1.0, 3.0)),
        "ctbr": dict(code=mppi.ACT_DIRECT_RPM, sigma=(2.0, 3.0, 3.0, 0.5), lo=None, hi=None)}


def make_core(n, dev, start, code, flags):
    return engine.SimCore(drone_model=DroneModel.CF2X, num_envs=n, drones_per_env=1, physics=flags, pyb_freq=240, ctrl_freq=48, act_code=code,
                          task=engine.TASK_NONE, initial_xyzs=start[:, None, :], auto_reset=False, track_rpm=True, device=dev)


class Composed:
    """the VEL plan on the table and the flags from gpd_rollout_plant + gpd_obstacles + torch"""

    def __init__(self, small, scales, field, goal, dev, a):
        self.small, self.dev, self.a = small, dev, a
        rec = np.repeat(field.records(), M, axis=0)
        tiled = ob.ObstacleField(N * M)
        for m in range(rec.shape[1]):
            tiled.cylinder(rec[:, m, 0:3], rec[:, m, 4], rec[:, m, 6])
        self.big = make_core(N * M, dev, np.zeros((N * M, 3)), a["code"], FLAGS)
        self.big.set_plant(scales.repeat_interleave(M, dim=1))
        self.query = ob.FieldQuery(tiled, dev, N * M, 1, small.P.COLLISION_R)
        self.pos4 = torch.zeros((N * M, 4), device=dev)
        self.goal = goal.repeat_interleave(M, dim=0)
        self.sigma, self.lo, self.hi = (torch.tensor(v, device=dev) for v in (a["sigma"], a["lo"], a["hi"]))
        self.radius = small.P.COLLISION_R

    def plan(self, u, sigma_scale=1.0):
        s, b = self.small, self.big
        for src, dst in ((s.kin_P, b.kin_P), (s.kin_Q, b.kin_Q), (s.kin_V, b.kin_V)):
            dst[:N * M] = src[:N].repeat_interleave(M, dim=0)
        b.kin_W[:N * M] = s.kin_W[:N].repeat_interleave(M)
        b.pid[:, :N * M] = s.pid[:, :N].repeat_interleave(M, dim=1)
        b.last_rpm[:, :N * M] = s.last_rpm[:, :N].repeat_interleave(M, dim=1)
        ut = u.repeat_interleave(M, dim=1)
        a = torch.minimum(torch.maximum(ut + (sigma_scale * self.sigma) * torch.randn_like(ut), self.lo), self.hi)
        obs = b.rollout(a, update_latest=False)[0]
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
    ap.add_argument("--no-composed", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    field = ob.ObstacleField.random_cylinders(N, CYLINDERS, (-1.5, -1.5, 1.5, 1.5), (0.15, 0.3), (1.5, 2.5), rng)
    start = np.stack([rng.uniform(-2.5, 1.5, N), rng.uniform(-1.0, 1.0, N), np.full(N, 0.4)], axis=1)     # low: the ground effect acts
    goal = torch.as_tensor(np.stack([np.minimum(3.5, start[:, 0] + 1.5), start[:, 1], start[:, 2]], axis=1), dtype=torch.float32, device=dev)
    r = np.array([0.2, 0.1, 0.1, 0.1, 0.2, 0.1, 0.1, 0.1, 0.1])[:, None]
    scales = torch.as_tensor(1.0 + r * rng.uniform(-1.0, 1.0, (len(_native.SCALE_FIELDS), N)), dtype=torch.float32, device=dev)
    jobs, extra = {}, {}
    for act, a in ACTS.items():
        bare, flagged = make_core(N, dev, start, a["code"], 0), make_core(N, dev, start, a["code"], FLAGS)
        ctrl = VectorCTBR(N, device=dev) if act == "ctbr" else None

        def make(core, **m):
            kw = dict(cost=COST, seed=1, field=field, act_lo=a["lo"], act_hi=a["hi"], **m)
            return mppi.MPPI(core, H, M, a["sigma"], LAM, **kw) if ctrl is None else mppi.CTBRMPPI(core, ctrl, H, M, a["sigma"], LAM, **kw)
        own = make(bare)
        for _ in range(10):                                   # a moving, tilted state and the last RPMs: ten planned steps on both cores
            u0 = own.plan(goal).contiguous()
            for core in (bare, flagged):
                if ctrl is None:
                    core.step(u0)
                else:
                    core.rollout_ctbr(ctrl, u0, 1, mode="cmd", last_only=True)
            own.advance()
        flagged.set_state(kin=bare.kin[:, :N].clone(), last_rpm=bare.last_rpm[:, :N].clone(), pid=None if bare.pid is None else bare.pid[:, :N].clone())
        planners = {"own": own, "plain": make(bare, model="aviary"), "table": make(bare, model="aviary", plant=scales),
                    "flags": make(flagged, model="aviary"), "both": make(flagged, model="aviary", plant=scales)}
        u = own.nominal.clone()
        for name, pl in planners.items():
            pl.nominal[:] = u
            jobs[f"{act}_{name}"] = ((lambda pl=pl: pl.plan(goal)), 20)
        if act == "vel" and not args.no_composed:
            composed = Composed(flagged, scales, field, goal, dev, a)
            quiet = make(flagged, model="aviary", plant=scales)
            quiet._q.sigma[:] = (0.0,) * 4
            quiet.nominal[:] = u
            quiet.plan(goal)
            _, S = composed.plan(u, sigma_scale=0.0)
            extra["costs_agree_without_noise"] = float(((quiet.costs - S).abs() / S.abs().clamp_min(1.0)).max())
            assert extra["costs_agree_without_noise"] < 1e-4, extra
            jobs["vel_composed"] = ((lambda: composed.plan(u)), 1)
    for fn, _ in jobs.values():
        fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in jobs}
    for _ in range(WINDOWS):                                   # in turns: what drifts, drifts for all
        for name, (fn, calls) in jobs.items():
            spent = done = 0
            while spent < MIN_SECONDS:
                spent += timed(fn, calls)
                done += calls
            windows[name].append(spent / done)
    per = {k: statistics.median(v) for k, v in windows.items()}
    ratio = {f"{act}_{name}": per[f"{act}_{name}"] / per[f"{act}_own"] for act in ACTS for name in ("plain", "table", "flags", "both")}
    res = {"device": torch.cuda.get_device_name(0), "drones": N, "samples": M, "horizon": H, "substeps": 5, "cylinders_per_aviary": CYLINDERS,
           "physics_flags": FLAGS, "windows": WINDOWS, "window_seconds_at_least": MIN_SECONDS, "per_plan_us_median": {k: v * 1e6 for k, v in per.items()},
           "per_plan_us_spread": {k: [min(v) * 1e6, max(v) * 1e6] for k, v in windows.items()}, "over_own_entry": ratio, **extra}
    if "vel_composed" in per:
        res["fused_speedup_vel_both"] = per["vel_composed"] / per["vel_both"]
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()

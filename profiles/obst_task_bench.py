#!/usr/bin/env python3
"""What one step of the obstacle task costs as ONE launch, against the only correct way to do the same step with the entries the
library had before, and against the physics alone.

    python profiles/obst_task_bench.py [--out profiles/obst_task_mi355x.json]

The shape: single drones on velocity commands (VEL, 48 Hz control over 240 Hz physics: 5 sub-steps), ONE shared list of 64 obstacles
(21 spheres, 21 boxes, 21 cylinders, a floor), 16 rays in the body frame, contact ends the episode and the aviary restarts; 65 536 and
4 096 aviaries; K = 1 and K = 20 steps per call.  Legs, timed with device events in ONE process, in turns, each until it has run for at
least 0.25 s after warm-up:
  fused      `gpd_rollout_obst`: one launch for the K steps
  composed   per step `gpd_step` without auto-reset, `gpd_obstacles` (clearance, hit), elementwise torch (reward, termination), a masked
             `gpd_reset`, `gpd_obstacles` again (clearance and scan of the pose that is observed) -- the K steps captured in ONE hipGraph
             and replayed: no host time between the launches
  rollout    `gpd_rollout` alone at the same shape: the physics share
No time is a pass condition.  The fused kernel maps a group of G = 16 lanes to a drone (csrc/obst_task.inc).  `alternative_mapping` in the
JSON holds what the variant build of profiles/obst_task_variant.patch measured once on the same legs -- a ray loop per lane with the
group capped at 16, 4 and 1 lanes (GPD_OBST_GSHIFT_MAX = 4, 2, 0), the last being a lane per drone -- and is carried over when the file is rewritten (the shipped library has one mapping and no switch).
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd import _native, engine, obstacles as ob  # noqa: E402

M_KIND, RAYS, MAX_RANGE, RADIUS, MIN_SECONDS = 21, 16, 5.0, 0.06, 0.25
HIT_REWARD, PROX_MARGIN, PROX_WEIGHT = -10.0, 0.5, 1.0
SIZES, STEPS = (65536, 4096), (1, 20)


def scene(n):
    rng = np.random.default_rng(1)
    side = 64.0 * math.sqrt(n / 65536)                      # the same density of drones at both sizes
    f = ob.ObstacleField()
    centre = lambda: rng.uniform([0, 0, 0.3], [side, side, 2.7])          # noqa: E731
    for _ in range(M_KIND):
        f.sphere(centre(), rng.uniform(0.5, 2.0) * side / 64.0)
    for _ in range(M_KIND):
        f.box(centre(), rng.uniform(0.5, 2.0, 3) * side / 64.0)
    for _ in range(M_KIND):
        f.cylinder(centre(), rng.uniform(0.5, 1.5) * side / 64.0, rng.uniform(0.5, 1.5))
    f.floor(0.0)
    start = rng.uniform([0, 0, 0.5], [side, side, 2.5], (n, 3))
    return f, start, rng


def core_of(n, start, auto_reset, dev):
    return engine.SimCore(num_envs=n, drones_per_env=1, physics=0, pyb_freq=240, ctrl_freq=48, act_code=2, task=engine.TASK_NONE,
                          initial_xyzs=start[:, None, :], auto_reset=auto_reset, track_rpm=False, device=dev)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def legs(n, K, dev):
    field, start, rng = scene(n)
    table = field.table(dev)
    rays = torch.as_tensor(ob.fan(RAYS, math.pi), device=dev)
    act = rng.normal(size=(K, n, 4)).astype(np.float32)
    act[..., 3] = rng.uniform(0.5, 1.0, (K, n))
    act = torch.as_tensor(act, device=dev)
    task = _native.GpdObstTask(collision_radius=RADIUS, hit_terminates=1, hit_reward=HIT_REWARD, prox_margin=PROX_MARGIN,
                               prox_weight=PROX_WEIGHT, n_rays=RAYS, ray_frame=ob.FRAMES["body"], max_range=MAX_RANGE)
    fused_core, comp_core, roll_core = core_of(n, start, True, dev), core_of(n, start, False, dev), core_of(n, start, True, dev)
    q = ob.FieldQuery(field, dev, n, 1, RADIUS)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)      # noqa: E731
    r, hr, pm, pw = f32(RADIUS), f32(HIT_REWARD), f32(PROX_MARGIN), f32(PROX_WEIGHT)
    kept = {}

    def composed_steps():
        c = comp_core
        for t in range(K):
            _, rew, term, trunc = c.step(act[t])
            cl = q.clearance(c.kin_P, c._stream())
            hinge = torch.clamp_min(pm - (cl.dist - r), 0.0)
            kept["reward"] = torch.where(cl.hit, rew + hr, rew) - pw * hinge
            kept["terminated"] = term | cl.hit
            c.reset(mask=kept["terminated"] | trunc)
            q.clearance(c.kin_P, c._stream())
            q.scan(c.kin_P, c.kin_Q, rays, MAX_RANGE, "body", False, c._stream())

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        composed_steps()                                    # (allocations and first launches outside the capture)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        composed_steps()
    # the two ways agree before either is timed: the same state in, the same rows out
    state = fused_core.get_state()
    comp_core.set_state(kin=state["kin"], pid=state["pid"], step_counter=state["step_counter"])
    rows = fused_core.rollout_obst(task, table, len(field), 1, rays, act)[0]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rows[K - 1, :, :12], comp_core.obs12) and torch.equal(rows[K - 1, :, 12:16], q._clear4)
    assert torch.equal(rows[K - 1, :, 16:16 + RAYS], q._scans[(RAYS, False)][0])
    jobs = {"fused": lambda: fused_core.rollout_obst(task, table, len(field), 1, rays, act), "composed": graph.replay,
            "rollout": lambda: roll_core.rollout(act, update_latest=False)}
    calls = max(1, 200 // K)
    for fn in jobs.values():
        fn()
    torch.cuda.synchronize()
    spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)
    while min(spent.values()) < MIN_SECONDS:                 # in turns: what drifts, drifts for all of them
        for name, fn in jobs.items():
            if spent[name] < MIN_SECONDS:
                spent[name] += timed(fn, calls)
                done[name] += calls
    us = {k: spent[k] / done[k] * 1e6 for k in jobs}
    return {"aviaries": n, "steps_per_call": K, "per_call_us": us, "per_step_us": {k: v / K for k, v in us.items()},
            "composed_over_fused": us["composed"] / us["fused"], "physics_share_of_fused": us["rollout"] / us["fused"],
            "launches_composed_per_step": 5, "calls": done, "seconds_timed": {k: round(v, 3) for k, v in spent.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "act": "VEL", "ctrl_hz": 48, "pyb_hz": 240, "obstacles": 3 * M_KIND + 1, "rays": RAYS,
           "ray_frame": "body", "mapping": "a group of G = 16 lanes per drone (the smallest power of two >= n_rays), one ray per lane",
           "shapes": [legs(n, K, dev) for n in SIZES for K in STEPS]}
    if a.out and os.path.exists(a.out):                      # (the other mappings were measured once, with a variant build: kept)
        res["alternative_mapping"] = json.load(open(a.out)).get("alternative_mapping")
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What a control step costs with the adaptive controller in the rollout kernel, and what it is measured against.

    python profiles/mrac_bench.py [--out profiles/mrac_mi355x.json] [--only pid_rollout] [--parent-pid-us X] [--reference-us Y]

65 536 single-drone aviaries, Physics.DYN, 240 Hz physics / 120 Hz control, K = 20 control steps per launch, observation rows of
every step stored.  Timed with device events in ONE process, in turns, each until it has run for at least 0.25 s after warm-up:
  pid_rollout        the yardstick: `ActionType.PID` through `gpd_rollout` (DSLPID, a controller with per-drone state in the loop)
  mrac_rollout       `gpd_rollout_mrac`
  mrac_rollout_plant ... with a per-drone plant table (mass x U(0.75, 1.25))
  mrac_unfused_graph 20 x (`gpd_step` + `gpd_mrac`) replayed from one hipGraph
  gpd_mrac           the controller call alone, n = 65 536
and, with the wall clock, `MRAC.computeControl` of the drop-in class per call (a launch and a stream wait each).
`--only NAME` times one variant: `--only pid_rollout` in a checkout of the parent commit gives the yardstick the bar is stated
against; its figure goes back in through `--parent-pid-us`, which records it and the ratio `mrac_over_parent_pid`.  `--reference-us`
records a figure for the reference's own class per call, measured wherever the reference is installed (on a CPU; not reproducible
from this tree, recorded for scale only).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd.envs import VectorAviary, VectorCtrlAviary  # noqa: E402
from gym_pybullet_drones_amd.utils.enums import ActionType, DroneModel, Physics  # noqa: E402

N, K, MIN_SECONDS = 65536, 20, 0.25
START, TARGET = np.array([[0.0, 0.0, 0.5]]), [0.3, -0.2, 1.0]


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
    ap.add_argument("--only", default=None)
    ap.add_argument("--parent-pid-us", type=float, default=None, help="us per control step of `--only pid_rollout` in a checkout of the parent commit")
    ap.add_argument("--reference-us", type=float, default=None, help="the reference's own MRAC.computeControl per call on a CPU (for scale)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(drone_model=DroneModel.CF2X, initial_xyzs=START, physics=Physics.DYN, pyb_freq=240, ctrl_freq=120, device=dev)
    jobs = {}
    pid = VectorAviary(N, num_drones=1, act=ActionType.PID, task="none", auto_reset=False, **kw)
    pid.reset()
    waypoint = torch.tensor(TARGET, dtype=torch.float32, device=dev).repeat(N, 1)
    jobs["pid_rollout"] = (lambda: pid.core.rollout(waypoint, num_steps=K, update_latest=False), 10, K)
    if a.only != "pid_rollout":
        from gym_pybullet_drones_amd.control import MRAC, VectorMRAC
        target = torch.tensor(TARGET + [0.0] * 9, dtype=torch.float32, device=dev).repeat(N, 1)

        def fleet(plant):
            env = VectorCtrlAviary(N, **kw)
            if plant:
                env.set_physical_params(mass=0.75 + 0.5 * torch.rand(N, device=dev))
            env.reset()
            return env, VectorMRAC(N, device=dev)
        e1, c1 = fleet(False)
        jobs["mrac_rollout"] = (lambda: e1.core.rollout_mrac(c1, target, K), 10, K)
        e2, c2 = fleet(True)
        jobs["mrac_rollout_plant"] = (lambda: e2.core.rollout_mrac(c2, target, K), 10, K)
        e3, c3 = fleet(False)
        rpm0 = torch.zeros((N, 4), dtype=torch.float32, device=dev)

        def pair(rpm):
            obs, _, _, _ = e3.core.step(rpm)
            return c3.compute(1 / 120, obs[:, 0:3], e3.core.quaternions(), obs[:, 6:9], obs[:, 9:12], target[:, 0:3])[0]
        pair(rpm0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            r = rpm0
            for _ in range(K):
                r = pair(r)
            rpm0.copy_(r)
        jobs["mrac_unfused_graph"] = (graph.replay, 10, K)
        e4, c4 = fleet(False)
        o = e4.core.obs12
        pos, quat, vel, angv = o[:, 0:3].contiguous(), e4.core.quaternions().contiguous(), o[:, 6:9].contiguous(), o[:, 9:12].contiguous()
        tpos = target[:, 0:3].contiguous()
        jobs["gpd_mrac"] = (lambda: c4.compute(1 / 120, pos, quat, vel, angv, tpos), 50, 1)
    if a.only:
        jobs = {a.only: jobs[a.only]}
    for fn, _, _ in jobs.values():                              # warm-up
        fn()
    torch.cuda.synchronize()
    spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)
    while min(spent.values()) < MIN_SECONDS:                    # in turns: what drifts, drifts for all of them
        for name, (fn, calls, _) in jobs.items():
            if spent[name] < MIN_SECONDS:
                spent[name] += timed(fn, calls)
                done[name] += calls
    res = {"method": "HIP events, >= 0.25 s per variant after warm-up, the variants in turns in one process",
           "device": torch.cuda.get_device_name(0), "drones": N, "steps_per_launch": K, "pyb_freq": 240, "ctrl_freq": 120,
           "us_per_control_step": {k: spent[k] / (done[k] * jobs[k][2]) * 1e6 for k in jobs}, "launches": done,
           "seconds_timed": {k: round(v, 3) for k, v in spent.items()}}
    u = res["us_per_control_step"]
    if "mrac_rollout" in u and "pid_rollout" in u:
        res["mrac_over_pid"] = u["mrac_rollout"] / u["pid_rollout"]
        res["bar"] = "mrac_rollout <= 2 x the parent commit's pid_rollout per control step"
    if a.parent_pid_us is not None and "mrac_rollout" in u:
        res["parent_commit_pid_rollout_us_per_control_step"] = a.parent_pid_us
        res["mrac_over_parent_pid"] = u["mrac_rollout"] / a.parent_pid_us
    if not a.only:
        one = MRAC(DroneModel.CF2X, device=dev)
        args = (1 / 120, np.array([0, 0, 0.5]), np.array([0, 0, 0, 1.0]), np.zeros(3), np.zeros(3), np.array(TARGET))
        for _ in range(50):
            one.computeControl(*args)
        t0 = time.perf_counter()
        for _ in range(2000):
            one.computeControl(*args)
        res["dropin_computeControl_us_per_call"] = (time.perf_counter() - t0) / 2000 * 1e6
        if a.reference_us is not None:
            res["reference_computeControl_us_per_call_cpu"] = a.reference_us
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

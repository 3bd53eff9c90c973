#!/usr/bin/env python3
"""What an env step on thrust and body-rate commands costs as ONE launch (`gpd_rollout_ctbr_task`), and what it is measured against.

    python profiles/ctbr_task_bench.py [--out profiles/ctbr_task_mi355x.json]

Single-drone aviaries, Physics.DYN, 240 Hz physics / 48 Hz control (5 sub-steps), the hover task with auto-reset and a 0.5 s episode
clock (so that resets happen all the time), a command block per step, rows, rewards and flags of every step stored.  Shapes: 65 536 and
4 096 aviaries, K = 1 and K = 20 steps per call.  Timed with device events in ONE process, the legs of a shape in turns, each until it
has run for at least 0.25 s after warm-up.
  fused            `SimCore.rollout_ctbr_task`: one launch for the K steps, called eagerly (`update_latest=False`: the launch alone, as
                   the composition's graph holds no copy into the latest-step tensors either)
  fused_graph      ... and the same launch replayed from a hipGraph (no host time, as for the composition)
  composed_graph   the same flight from its parts, replayed from ONE hipGraph: per step clone the counters, `gpd_rollout_ctbr` (one
                   step), `gpd_task_eval` on its rows, terminated | truncated, the terminal rows, a masked `gpd_reset`
  ctbr_no_task     beside both: `gpd_rollout_ctbr` alone, no task and no reset
  pid_task         ... and `gpd_rollout` with the task on DSLPID (`ActionType.PID`), the controller the project already closes in the
                   kernel (`update_latest=False` too)
Before anything is timed, `fused` and the composition (eager) fly K steps from the same state and must agree bit for bit.
The one condition: fused (eager) is faster than composed_graph at every shape.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd import _native, engine  # noqa: E402
from gym_pybullet_drones_amd.control import VectorCTBR  # noqa: E402
from gym_pybullet_drones_amd.utils.enums import ACT_RAW_RPM, ActionType, DroneModel  # noqa: E402

S, MIN_SECONDS = 5, 0.25
SHAPES = ((65536, 1), (65536, 20), (4096, 1), (4096, 20))


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def bits(a, b):
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a, b))


def core_of(N, dev, rng, task, act_code=ACT_RAW_RPM):
    xyz = np.stack([rng.uniform(-1.0, 1.0, N), rng.uniform(-1.0, 1.0, N), rng.uniform(0.5, 1.5, N)], axis=-1).reshape(N, 1, 3)
    core = engine.SimCore(drone_model=DroneModel.CF2X, num_envs=N, drones_per_env=1, physics=0, pyb_freq=240, ctrl_freq=240 // S, act_code=act_code,
                          task=engine.TASK_HOVER if task else engine.TASK_NONE, initial_xyzs=xyz, target_pos=np.array([[0.0, 0.0, 1.0]]),
                          episode_len_sec=0.5, auto_reset=task, track_rpm=True, keep_terminal_obs=task, device=dev)
    core.step_counter.copy_(torch.tensor(rng.integers(0, 24, N) * S, dtype=torch.int32))       # (the episode clocks out of step)
    return core


def shape(N, K, dev):
    """the five legs of one shape, after the agreement check: {name: (callable, calls per timing)}"""
    seed = 100 * K + N % 97
    cmd = np.concatenate([np.random.default_rng(seed).uniform(9.0, 10.6, (K, N, 1)), np.random.default_rng(seed + 1).normal(0.0, 0.3, (K, N, 3))], axis=-1)
    cmd = torch.tensor(cmd, dtype=torch.float32, device=dev)
    ctrl = VectorCTBR(N, device=dev)
    fused, parts, plain = (core_of(N, dev, np.random.default_rng(seed), task) for task in (True, False, False))
    cfg, target = fused._cfg, fused.target
    terminal = torch.zeros((K, N, 12), dtype=torch.float32, device=dev)
    kept = [None] * 4

    def composed():
        obs, rew, term, trunc = [], [], [], []
        for t in range(K):
            counters = parts.step_counter.clone()
            parts.rollout_ctbr(ctrl, cmd[t], 1, mode="cmd", last_only=True)
            r = torch.empty((N,), dtype=torch.float32, device=dev)
            te, tr = torch.empty((N,), dtype=torch.bool, device=dev), torch.empty((N,), dtype=torch.bool, device=dev)
            _native.call("gpd_task_eval", dev, parts._stream(), cfg, parts.obs12, counters, target, r, te, tr)
            mask = te | tr
            torch.where(mask.unsqueeze(1), parts.obs12, terminal[t], out=terminal[t])
            parts.reset(mask=mask)
            obs.append(parts.obs12.clone()), rew.append(r), term.append(te), trunc.append(tr)
        kept[:] = [torch.stack(v) for v in (obs, rew, term, trunc)]

    # ---- the two ways agree bit for bit before either is timed
    got = [x.clone() for x in fused.rollout_ctbr_task(ctrl, cmd)]
    composed()
    same = all(bits(a, b) for a, b in zip(got, kept)) and bits(fused.kin_store, parts.kin_store) and bits(fused.last_rpm, parts.last_rpm) \
        and bits(fused.step_counter, parts.step_counter)
    ends = int((got[2] | got[3]).sum())
    if not same:
        raise SystemExit(f"N={N} K={K}: the fused launch and the composition disagree")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        composed()
    fgraph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(fgraph):
        fused.rollout_ctbr_task(ctrl, cmd, update_latest=False)
    pid = core_of(N, dev, np.random.default_rng(seed), True, act_code=ActionType.PID.code)
    way = torch.tensor(np.random.default_rng(seed + 2).uniform(-0.5, 0.5, (K, N, 3)) + [0.0, 0.0, 1.0], dtype=torch.float32, device=dev)
    few = 200 if K == 1 else 20
    return {"fused": (lambda: fused.rollout_ctbr_task(ctrl, cmd, update_latest=False), few), "fused_graph": (fgraph.replay, few),
            "composed_graph": (graph.replay, 5 if K > 1 else 50), "ctbr_no_task": (lambda: plain.rollout_ctbr(ctrl, cmd, K, mode="cmd"), few),
            "pid_task": (lambda: pid.rollout(way, update_latest=False), few)}, ends


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda:0")
    res = {"method": f"HIP events, >= {MIN_SECONDS} s per leg after warm-up, the legs of a shape in turns in one process; fused and composed agree bit for bit first",
           "device": torch.cuda.get_device_name(0), "pyb_freq": 240, "ctrl_freq": 240 // S, "substeps": S, "shapes": {}}
    for N, K in SHAPES:
        jobs, ends = shape(N, K, dev)
        for fn, _ in jobs.values():                              # warm-up
            fn()
        torch.cuda.synchronize()
        spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)
        while min(spent.values()) < MIN_SECONDS:                # in turns: what drifts, drifts for all of them
            for name, (fn, calls) in jobs.items():
                if spent[name] < MIN_SECONDS:
                    spent[name] += timed(fn, calls)
                    done[name] += calls
        us = {k: spent[k] / (done[k] * K) * 1e6 for k in jobs}
        res["shapes"][f"N{N}_K{K}"] = {"drones": N, "steps_per_call": K, "episode_ends_in_the_checked_call": ends, "bit_for_bit": True,
                                       "us_per_env_step": us, "composed_over_fused": us["composed_graph"] / us["fused"],
                                       "fused_over_ctbr_no_task": us["fused"] / us["ctbr_no_task"]}
        print(f"N={N} K={K}", json.dumps(us), flush=True)
    res["condition"] = "the fused launch is faster than the composition in one hipGraph at every shape"
    res["condition_met"] = all(v["composed_over_fused"] > 1.0 for v in res["shapes"].values())
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

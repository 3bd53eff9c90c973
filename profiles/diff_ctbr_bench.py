#!/usr/bin/env python3
"""What the differentiable rollout on thrust and body-rate commands costs, and what it is measured against.

    python profiles/diff_ctbr_bench.py [--out profiles/diff_ctbr_mi355x.json] [--grad-figures FILE] [--registers FILE]

65 536 single-drone aviaries, Physics.DYN, no task, K = 20 control steps per launch, observation rows of every step stored, at S = 5
(48 Hz control) and S = 1 (240 Hz control) physics sub-steps per step, "cmd" rows (commands) and "pos" rows (targets through the outer
loop).  Timed with device events in ONE process, the variants in turns, each for at least 1 s per round after warm-up, the median of
three rounds; us per CONTROL STEP of all drones:
  rollout_ctbr_<mode>   the yardstick: `gpd_rollout_ctbr` (the kernel this change does not touch) on the same box
  tape_<mode>           `gpd_rollout_tape_ctbr`: the same arithmetic + the 52 B per drone-step tape
  vjp_<mode>            `gpd_rollout_vjp_ctbr`: the reverse sweep, cotangents for every output, without the gains' cotangents
  vjp_gains_<mode>      ... and with them
  rollout_vjp           `gpd_rollout_vjp` on RAW_RPM actions at the same S: the RPM sweep, whose S(S+1)/2 recomputed sub-steps per step
                        the CTBR sweep repeats with a rate loop in front of each (and S adjoint rate loops on top)
No time is a pass condition.  `--grad-figures`: a JSON file of measured gradient errors (tests/test_gpu_diff_ctbr.py prints them),
`--registers`: a JSON file of the kernels' register counts, both to record next to the timings.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from gym_pybullet_drones_amd import diff, engine  # noqa: E402
from gym_pybullet_drones_amd.control import VectorCTBR  # noqa: E402

N, K, MIN_SECONDS, ROUNDS = 65536, 20, 1.0, 3


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def variants(S, dev):
    def core_of(act_code):
        return engine.SimCore(num_envs=N, drones_per_env=1, pyb_freq=240, ctrl_freq=240 // S, act_code=act_code, task=engine.TASK_NONE,
                              auto_reset=False, track_rpm=True, device=dev)
    core, ctrl = core_of(5), VectorCTBR(N, device=dev)
    g = torch.Generator(device=dev).manual_seed(S)
    kin0 = core.kin_store.clone()
    cmd = torch.cat([8.0 + 4.0 * torch.rand((K, N, 1), generator=g, device=dev), torch.rand((K, N, 3), generator=g, device=dev) * 2 - 1], dim=-1).contiguous()
    tgt = torch.zeros((K, N, 12), device=dev)
    tgt[..., 0:3] = torch.rand((K, N, 3), generator=g, device=dev) * 0.6 - 0.3 + torch.tensor([0.0, 0.0, 1.0], device=dev)
    rows = {"cmd": cmd, "pos": tgt.contiguous()}
    obs = torch.empty((K, N, 12), device=dev)
    g_obs, g_kin = torch.randn((K, N, 12), generator=g, device=dev), torch.randn(13 * core.ld, generator=g, device=dev)
    g_gains = torch.empty((12, core.ld), device=dev)
    tapes = {m: torch.empty(diff.tape_floats_ctbr(core, K), device=dev) for m in rows}
    g_rows = {m: torch.empty_like(r) for m, r in rows.items()}
    jobs = {}
    for mode, r in rows.items():
        stride = r.numel() // K

        def rollout(mode=mode, r=r):
            core.kin_store.copy_(kin0)
            core.rollout_ctbr(ctrl, r, K, mode=mode)

        def tape(mode=mode, r=r, stride=stride):
            core.kin_store.copy_(kin0)
            diff.tape_forward_ctbr(core, ctrl.struct(), mode, K, r, stride, obs, tapes[mode])

        def vjp(mode=mode, r=r, stride=stride, gains=None):
            diff.sweep_ctbr(core, ctrl.struct(), mode, K, r, stride, tapes[mode], g_obs, g_kin, g_rows[mode], gains)

        def vjp_gains(vjp=vjp):
            vjp(gains=g_gains)
        tape()                                                 # (the reverse sweeps read these tapes)
        jobs.update({f"rollout_ctbr_{mode}": rollout, f"tape_{mode}": tape, f"vjp_{mode}": vjp, f"vjp_gains_{mode}": vjp_gains})
    # the RPM sweep at the same S, for the recomputation's cost: RAW_RPM actions around hover
    rpm = core_of(5)
    acts = (rpm.P.HOVER_RPM * (1 + 0.05 * (torch.rand((K, N, 4), generator=g, device=dev) * 2 - 1))).contiguous()
    r_tape = torch.empty(diff.tape_floats(rpm, K), device=dev)
    rew, flags = torch.empty((K, N), device=dev), torch.empty((2, K, N), dtype=torch.bool, device=dev)
    diff.tape_forward(rpm, K, acts, N * 4, obs, rew, flags[0], flags[1], r_tape)
    g_act = torch.empty((K, N, 4), device=dev)
    jobs["rollout_vjp"] = lambda: diff.sweep(rpm, K, acts, N * 4, r_tape, g_obs, None, g_kin, g_act)
    return jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grad-figures", default=None)
    ap.add_argument("--registers", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"method": "HIP events, >= 1 s per variant and round after warm-up, the variants in turns in one process, the median of three rounds; "
                     "rollout_ctbr_* and tape_* include the 3.4 MB copy that restores the initial state",
           "device": torch.cuda.get_device_name(0), "drones": N, "steps_per_launch": K, "us_per_control_step": {}, "tape_bytes_per_drone_step": 52}
    for S in (5, 1):
        jobs = variants(S, dev)
        for fn in jobs.values():                               # warm-up
            fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in jobs}
        for _ in range(ROUNDS):
            spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)
            while not all(spent[n] >= MIN_SECONDS for n in jobs):      # in turns: what drifts, drifts for all of them
                for name, fn in jobs.items():
                    if spent[name] < MIN_SECONDS:
                        spent[name] += timed(fn, 10)
                        done[name] += 10
            for k in jobs:
                rounds[k].append(spent[k] / (done[k] * K) * 1e6)
        u = {k: statistics.median(v) for k, v in rounds.items()}
        u["rounds"] = rounds
        for mode in ("cmd", "pos"):
            u[f"tape_over_rollout_ctbr_{mode}"] = u[f"tape_{mode}"] / u[f"rollout_ctbr_{mode}"]
            u[f"vjp_over_rollout_ctbr_{mode}"] = u[f"vjp_{mode}"] / u[f"rollout_ctbr_{mode}"]
            u[f"vjp_gains_over_vjp_{mode}"] = u[f"vjp_gains_{mode}"] / u[f"vjp_{mode}"]
        u["vjp_cmd_over_rollout_vjp"] = u["vjp_cmd"] / u["rollout_vjp"]
        u["recomputed_substeps_per_step"] = S * (S + 1) // 2
        res["us_per_control_step"][f"S={S}"] = u
        print(f"S={S}", json.dumps({k: v for k, v in u.items() if k != "rounds"}), flush=True)
    if a.grad_figures and os.path.exists(a.grad_figures):
        res["gradient_error_vs_float64"] = json.load(open(a.grad_figures))
    elif a.out and os.path.exists(a.out):                      # (new timings keep the figures tests/test_gpu_diff_ctbr.py recorded there)
        kept = json.load(open(a.out))
        res.update({k: kept[k] for k in ("metric", "bound_rule", "gradient_error_vs_float64", "registers") if k in kept})
    if a.registers and os.path.exists(a.registers):
        res["registers"] = json.load(open(a.registers))
    print(json.dumps({k: v for k, v in res.items() if k != "us_per_control_step"}))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

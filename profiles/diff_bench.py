#!/usr/bin/env python3
"""What the differentiable rollout costs, and what it is measured against.

    python profiles/diff_bench.py [--out profiles/diff_mi355x.json] [--grad-figures FILE] [--registers FILE] [--no-torch]

65 536 single-drone HoverAviaries, Physics.DYN, ActionType.RPM, K = 20 env steps per launch, observation rows of every step stored, at
S = 1 (240 Hz control) and S = 8 (30 Hz control) physics sub-steps per step.  Timed with device events in ONE process, in turns, each
until it has run for at least 0.25 s after warm-up; us per ENV STEP:
  rollout          the yardstick: `gpd_rollout` (the kernel this change does not touch) on the same box
  rollout_tape     `gpd_rollout_tape`: the same arithmetic + the 52 B per drone-step tape
  rollout_vjp      `gpd_rollout_vjp`: the reverse sweep (cotangents for every output)
  vjp_table        `gpd_rollout_vjp` on a per-drone plant table (scales within +-20 %): the sweep without the rows' cotangents
  vjp_plant        `gpd_rollout_vjp_plant` on the same table and tape: the sweep that also sums the cotangents of the plant rows
  derive_vjp       `gpd_plant_derive_vjp`: rows -> scale factors (us per CALL / K, to add to vjp_plant)
  torch_autograd   the user's alternative: the float32 torch restatement of tests/helpers/diff_f64.py on the device, forward +
                   `.backward()` for the same gradient (one launch per arithmetic operation; timed for at least 3 passes; `--no-torch`
                   leaves it out)
No time is a pass condition.  `--grad-figures`: a JSON file of measured gradient errors (tests/test_gpu_diff.py and
tests/test_gpu_sysid.py print them), `--registers`: a JSON file of the kernels' register counts (the compiler's
`-Rpass-analysis=kernel-resource-usage` remarks), both to record next to the timings.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))

import diff_f64 as ref  # noqa: E402
from gym_pybullet_drones_amd import _native, diff, engine  # noqa: E402
from gym_pybullet_drones_amd.diff import tape_floats, unpack_kin  # noqa: E402

N, K, MIN_SECONDS = 65536, 20, 0.25


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def variants(S, dev, with_torch=True):
    core = engine.SimCore(num_envs=N, drones_per_env=1, pyb_freq=240, ctrl_freq=240 // S, act_code=0, task=engine.TASK_HOVER,
                          target_pos=[[0.0, 0.0, 1.0]], auto_reset=False, track_rpm=True, device=dev)
    g = torch.Generator(device=dev).manual_seed(S)
    acts = (torch.rand((K, N, 4), generator=g, device=dev) * 2 - 1).contiguous()
    kin0 = core.kin_store.clone()
    tape = torch.empty(tape_floats(core, K), dtype=torch.float32, device=dev)
    obs, rew = torch.empty((K, N, 12), device=dev), torch.empty((K, N), device=dev)
    flags = torch.empty((2, K, N), dtype=torch.bool, device=dev)
    g_obs, g_rew = torch.randn((K, N, 12), generator=g, device=dev), torch.randn((K, N), generator=g, device=dev)
    g_kin, g_act = torch.randn(13 * core.ld, generator=g, device=dev), torch.empty((K, N, 4), device=dev)

    def rollout():
        core.kin_store.copy_(kin0)
        core.rollout(acts, update_latest=False)

    def rollout_tape():
        core.kin_store.copy_(kin0)
        diff.tape_forward(core, K, acts, N * 4, obs, rew, flags[0], flags[1], tape)

    def rollout_vjp():
        diff.sweep(core, K, acts, N * 4, tape, g_obs, g_rew, g_kin, g_act)

    cfg = ref.config("cf2x", "rpm", S, False, "hover")
    c = ref.consts(core.P, N, torch.float32, device=dev)
    target = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(N, 3)
    zero = torch.zeros(N, device=dev)

    def torch_autograd():
        a = acts.clone().requires_grad_(True)
        k0 = tuple(x.clone().requires_grad_(True) for x in unpack_kin(kin0, N))
        o, r, kk = ref.rollout(c, cfg, k0, a, zero, target)
        loss = (g_obs * o).sum() + (g_rew * r).sum() + sum((gk * x).sum() for gk, x in zip(unpack_kin(g_kin, N), kk))
        torch.autograd.grad(loss, (a,) + k0)

    # the same drones with a plant table: a core of its own, so that the nominal variants above keep the uniform kernels
    plant = engine.SimCore(num_envs=N, drones_per_env=1, pyb_freq=240, ctrl_freq=240 // S, act_code=0, task=engine.TASK_HOVER,
                           target_pos=[[0.0, 0.0, 1.0]], auto_reset=False, track_rpm=True, device=dev)
    plant.set_plant(torch.rand((9, N), generator=g, device=dev) * 0.4 + 0.8)
    p_tape = torch.empty_like(tape)
    g_rows = torch.empty((_native.PLANT_ROWS, plant.ld), device=dev)
    g_scales = torch.empty((len(_native.SCALE_FIELDS), plant.ld), device=dev)

    def vjp_table():
        diff.sweep(plant, K, acts, N * 4, p_tape, g_obs, g_rew, g_kin, g_act)

    def vjp_plant():
        diff.sweep(plant, K, acts, N * 4, p_tape, g_obs, g_rew, g_kin, g_act, g_rows=g_rows)

    def derive_vjp():
        diff.derive_vjp(plant, plant.plant_scales, g_rows, g_scales)

    rollout_tape()                                             # (the reverse sweeps read these tapes)
    diff.tape_forward(plant, K, acts, N * 4, obs, rew, flags[0], flags[1], p_tape)
    jobs = {"rollout": (rollout, 10), "rollout_tape": (rollout_tape, 10), "rollout_vjp": (rollout_vjp, 10), "vjp_table": (vjp_table, 10),
            "vjp_plant": (vjp_plant, 10), "derive_vjp": (derive_vjp, 10)}
    if with_torch:
        jobs["torch_autograd"] = (torch_autograd, 1)
    return jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grad-figures", default=None)
    ap.add_argument("--registers", default=None)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"method": "HIP events, >= 0.25 s per variant after warm-up (torch_autograd: >= 3 passes), the variants in turns in one process; "
                     "rollout and rollout_tape include the 3.4 MB copy that restores the initial state",
           "device": torch.cuda.get_device_name(0), "drones": N, "steps_per_launch": K, "us_per_env_step": {}, "tape_bytes_per_drone_step": 52}
    for S in (1, 8):
        jobs = variants(S, dev, not a.no_torch)
        for fn, _ in jobs.values():                            # warm-up
            fn()
        torch.cuda.synchronize()
        spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)

        def enough(name):
            return spent[name] >= MIN_SECONDS and done[name] >= 3
        while not all(enough(n) for n in jobs):                # in turns: what drifts, drifts for all of them
            for name, (fn, calls) in jobs.items():
                if not enough(name):
                    spent[name] += timed(fn, calls)
                    done[name] += calls
        u = {k: spent[k] / (done[k] * K) * 1e6 for k in jobs}
        u["tape_over_rollout"] = u["rollout_tape"] / u["rollout"]
        u["vjp_over_rollout"] = u["rollout_vjp"] / u["rollout"]
        u["vjp_plant_over_vjp_table"] = u["vjp_plant"] / u["vjp_table"]
        if "torch_autograd" in u:
            u["torch_autograd_over_tape_plus_vjp"] = u["torch_autograd"] / (u["rollout_tape"] + u["rollout_vjp"])
        res["us_per_env_step"][f"S={S}"] = u
        print(f"S={S}", json.dumps(u), flush=True)
    if a.grad_figures and os.path.exists(a.grad_figures):
        res["gradient_error_vs_float64"] = json.load(open(a.grad_figures))
    elif a.out and os.path.exists(a.out):                      # (new timings keep the figures tests/test_gpu_diff.py recorded there)
        kept = json.load(open(a.out))
        res.update({k: kept[k] for k in ("metric", "bound_rule", "gradient_error_vs_float64") if k in kept})
    if a.registers and os.path.exists(a.registers):
        res["registers"] = json.load(open(a.registers))
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the differentiable rollout through the DSLPID loop costs, and what it is measured against.

    python profiles/diff_pid_bench.py [--out profiles/diff_pid_mi355x.json] [--grad-figures FILE] [--registers FILE] [--no-torch]

65 536 single-drone HoverAviaries, Physics.DYN, ActionType.VEL, K = 20 env steps per launch at 48 Hz control (S = 5 physics sub-steps
per step), observation rows of every step stored.  Timed with device events in ONE process, in turns, each until it has run for at least
0.25 s after warm-up; us per ENV STEP:
  rollout          the yardstick: `gpd_rollout` (a kernel this feature does not touch) on the same box, alone
  tape_pid         `gpd_rollout_tape_pid`: the same arithmetic + the 88 B per drone-step tape
  vjp_pid          `gpd_rollout_vjp_pid` without the gains' cotangents (cotangents for every output)
  vjp_pid_gains    `gpd_rollout_vjp_pid` with `g_gains [18][ld]`
  torch_autograd   the user's alternative: the float32 torch restatement of tests/helpers/diff_pid_f64.py on the device, forward +
                   `.backward()` for the same gradients (one launch per arithmetic operation; at least 3 passes; `--no-torch` leaves it out)
No time is a pass condition.  `--grad-figures`: a JSON file of measured gradient errors (tests/test_gpu_diff_pid.py prints them),
`--registers`: a JSON file of the kernels' register counts (the compiler's `-Rpass-analysis=kernel-resource-usage` remarks), both to
record next to the timings.
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
import diff_pid_f64 as pref  # noqa: E402
from gym_pybullet_drones_amd import diff, engine  # noqa: E402
from gym_pybullet_drones_amd.diff import unpack_kin, unpack_pid  # noqa: E402

N, K, S, MIN_SECONDS = 65536, 20, 5, 0.25


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def variants(dev, with_torch=True):
    core = engine.SimCore(num_envs=N, drones_per_env=1, pyb_freq=240, ctrl_freq=240 // S, act_code=pref.ACT_CODE["vel"], task=engine.TASK_HOVER,
                          target_pos=[[0.0, 0.0, 1.0]], auto_reset=False, track_rpm=True, device=dev)
    g = torch.Generator(device=dev).manual_seed(S)
    acts = (torch.rand((K, N, 4), generator=g, device=dev) * 2 - 1).contiguous()
    kin0, pid0 = core.kin_store.clone(), core.pid.clone()
    tape = torch.empty(diff.tape_floats_pid(core, K), dtype=torch.float32, device=dev)
    obs, rew = torch.empty((K, N, 12), device=dev), torch.empty((K, N), device=dev)
    flags = torch.empty((2, K, N), dtype=torch.bool, device=dev)
    g_obs, g_rew = torch.randn((K, N, 12), generator=g, device=dev), torch.randn((K, N), generator=g, device=dev)
    g_kin, g_pid = torch.randn(13 * core.ld, generator=g, device=dev), torch.randn((9, core.ld), generator=g, device=dev)
    g_kin_w, g_pid_w = g_kin.clone(), g_pid.clone()
    g_act, g_gains = torch.empty((K, N, 4), device=dev), torch.empty((18, core.ld), device=dev)

    def restore():
        core.kin_store.copy_(kin0)
        core.pid.copy_(pid0)

    def rollout():
        restore()
        core.rollout(acts, update_latest=False)

    def tape_pid():
        restore()
        diff.tape_forward_pid(core, core._params, K, acts, N * 4, obs, rew, flags[0], flags[1], tape)

    def vjp_pid():          # (g_kin / g_pid are in place: a scratch copy is swept, as the binding's backward does)
        g_kin_w.copy_(g_kin)
        g_pid_w.copy_(g_pid)
        diff.sweep_pid(core, core._params, K, acts, N * 4, tape, g_obs, g_rew, g_kin_w, g_pid_w, g_act)

    def vjp_pid_gains():
        g_kin_w.copy_(g_kin)
        g_pid_w.copy_(g_pid)
        diff.sweep_pid(core, core._params, K, acts, N * 4, tape, g_obs, g_rew, g_kin_w, g_pid_w, g_act, g_gains)

    cfg = ref.config("cf2x", "vel", S, False, "hover")
    c = ref.consts(core.P, N, torch.float32, device=dev)
    target = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(N, 3)
    gains0 = torch.as_tensor(pref.DEFAULT_GAINS, dtype=torch.float32, device=dev)

    def torch_autograd():
        a = acts.clone().requires_grad_(True)
        gg = gains0.clone().requires_grad_(True)
        k0 = tuple(x.clone().requires_grad_(True) for x in unpack_kin(kin0, N))
        m0 = tuple(x.clone().requires_grad_(True) for x in unpack_pid(pid0, N))
        pc = pref.pid_consts_of(core.P, gg, torch.float32)
        pc.mixer = pc.mixer.to(dev)
        o, r, kk, mm = pref.rollout(c, pc, cfg, k0, m0, a, target)
        loss = (g_obs * o).sum() + (g_rew * r).sum() + sum((gk * x).sum() for gk, x in zip(unpack_kin(g_kin, N), kk)) + \
            sum((gm * x).sum() for gm, x in zip(unpack_pid(g_pid, N), mm))
        torch.autograd.grad(loss, (a, gg) + k0 + m0)

    tape_pid()                                                 # (the reverse sweeps read this tape)
    jobs = {"rollout": (rollout, 10), "tape_pid": (tape_pid, 10), "vjp_pid": (vjp_pid, 10), "vjp_pid_gains": (vjp_pid_gains, 10)}
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
                     "rollout and tape_pid include the copies that restore the initial state and members, the sweeps the copies of the "
                     "cotangents they overwrite",
           "device": torch.cuda.get_device_name(0), "drones": N, "steps_per_launch": K, "substeps": S, "action_type": "vel",
           "tape_bytes_per_drone_step": 88}
    jobs = variants(dev, not a.no_torch)
    for fn, _ in jobs.values():                                # warm-up
        fn()
    torch.cuda.synchronize()
    spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)

    def enough(name):
        return spent[name] >= MIN_SECONDS and done[name] >= 3
    while not all(enough(n) for n in jobs):                    # in turns: what drifts, drifts for all of them
        for name, (fn, calls) in jobs.items():
            if not enough(name):
                spent[name] += timed(fn, calls)
                done[name] += calls
    u = {k: spent[k] / (done[k] * K) * 1e6 for k in jobs}
    u["tape_over_rollout"] = u["tape_pid"] / u["rollout"]
    u["vjp_over_rollout"] = u["vjp_pid"] / u["rollout"]
    u["gains_over_no_gains"] = u["vjp_pid_gains"] / u["vjp_pid"]
    if "torch_autograd" in u:
        u["torch_autograd_over_tape_plus_vjp_gains"] = u["torch_autograd"] / (u["tape_pid"] + u["vjp_pid_gains"])
    res["us_per_env_step"] = u
    if a.grad_figures and os.path.exists(a.grad_figures):
        res["gradient_error_vs_float64"] = json.load(open(a.grad_figures))
    if a.registers and os.path.exists(a.registers):
        res["registers"] = json.load(open(a.registers))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

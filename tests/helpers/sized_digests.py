"""Prints one JSON line of digests: rollouts and single steps of the shapes `gpd_rollout1_kernel` / `gpd_step_kernel` have compile-time
variants for (csrc/step_rollout.hip: aviary size, physics flags, one sub-step per step as template parameters), plus shapes that take
the generic kernels.  tests/test_gpu_rollout.py runs it twice -- with GPD_ROLLOUT_SIZED=0 (generic kernels only) and without -- and
compares: the variants are the generic kernel bit for bit."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gym_pybullet_drones_amd.envs import VectorAviary          # noqa: E402
from gym_pybullet_drones_amd.utils.enums import ActionType     # noqa: E402

dev = torch.device("cuda", 0)
out = {}
# (drones per aviary, physics flags, action type, sub-steps): sized <8,7>, <2,4>, <1 drone,7>, <any,7>, <2,-1> at 1 and 8 sub-steps,
# <any size, one sub-step>; and generic shapes (3 drones at 30 Hz, 12 drones with the drag term only)
SHAPES = [(8, 7, "rpm", 1), (8, 7, "pid", 1), (2, 4, "rpm", 1), (2, 4, "vel", 1), (1, 7, "one_d_rpm", 1), (1, 7, "pid", 1), (5, 7, "rpm", 1),
          (2, 0, "rpm", 1), (2, 0, "one_d_pid", 8), (2, 7, "rpm", 8), (3, 4, "rpm", 1), (3, 7, "rpm", 8), (12, 2, "pid", 1),
          # ... and with the ground plane (8) / damping (16) bits that `Physics.PYB_*` members add by default (the HI variants)
          (8, 15, "rpm", 1), (2, 12, "vel", 1), (1, 15, "one_d_rpm", 1), (3, 31, "pid", 1), (1, 8, "rpm", 1), (1, 8, "one_d_rpm", 8), (1, 24, "pid", 5),
          (2, 8, "rpm", 8), (2, 24, "one_d_pid", 1),
          # the add-on sets under the sub-step loop
          (1, 15, "rpm", 8), (1, 7, "pid", 5), (2, 12, "rpm", 8), (8, 7, "one_d_rpm", 4), (4, 23, "vel", 8),
          # the any-size <flags 7> variants at larger aviaries: groups of four mates in full waves (16, 64), 31 pad lanes per wave (33)
          (16, 7, "rpm", 1), (33, 7, "rpm", 8), (64, 15, "pid", 1)]
for D, phys, act, S in SHAPES:
    E = 777 if D == 1 else {16: 17, 33: 9, 64: 5}.get(D, 300)          # (the larger aviaries: two workgroups, the last one ragged)
    rng = np.random.default_rng(100 * D + phys)
    xyz = np.zeros((E, D, 3))
    xyz[..., :2] = rng.uniform(-0.3, 0.3, size=(E, D, 2))
    xyz[..., 2] = (0.05 if phys & 8 else 0.4) + 0.3 * np.arange(D) + rng.uniform(-0.02, 0.02, size=(E, D))    # (near the plane when it acts)
    rpy = rng.uniform(-0.1, 0.1, size=(E, D, 3))
    env = VectorAviary(E, D, initial_xyzs=xyz, initial_rpys=rpy, physics=phys, pyb_freq=240, ctrl_freq=240 // S, act=ActionType(act),
                       task="hover" if D == 1 else "multihover", auto_reset=True, track_rpm=True, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    a = torch.rand((20, E, D, env.ACT_DIM), generator=g, device=dev) * 2 - 1
    if act in ("pid", "one_d_pid"):
        a = a * 0.3
        a[..., -1] += 1.0
    if act == "vel":
        a[..., 3] = a[..., 3].abs()
    h = hashlib.sha256()
    for t in (*env.core.rollout(a.contiguous(), update_latest=False), env.core.kin_store):
        h.update(t.cpu().numpy().tobytes())
    for k in range(5):
        for t in env.core.step(a[k].contiguous()):
            h.update(t.cpu().numpy().tobytes())
    out[f"D{D}_flags{phys}_{act}_S{S}"] = h.hexdigest()[:20]
# the compute-wave + store-wave kernel (rollouts that keep terminal observations): its action type / sub-step count variants
for act, S, phys in (("rpm", 1, 0), ("pid", 1, 7), ("one_d_rpm", 8, 8), ("vel", 2, 0)):
    E = 777
    env = VectorAviary(E, 1, physics=phys, pyb_freq=240, ctrl_freq=240 // S, act=ActionType(act), task="hover", auto_reset=True, track_rpm=True,
                       keep_terminal_obs=True, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    a = torch.rand((20, E, 1, env.ACT_DIM), generator=g, device=dev) * 2 - 1
    if act == "pid":
        a = a * 0.3
        a[..., -1] += 1.0
    if act == "vel":
        a[..., 3] = a[..., 3].abs()
    h = hashlib.sha256()
    for t in (*env.core.rollout(a.contiguous(), update_latest=True), env.core.kin_store, env.core.term_obs12):
        h.update(t.cpu().numpy().tobytes())
    out[f"termobs_flags{phys}_{act}_S{S}"] = h.hexdigest()[:20]
print(json.dumps(out))

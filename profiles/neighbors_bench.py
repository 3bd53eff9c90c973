#!/usr/bin/env python3
"""What one `SwarmAviary.neighbors()` call costs at 65 536 drones, and what it is measured against.

    python profiles/neighbors_bench.py [--out profiles/neighbors_mi355x.json]
    rocprofv3 --kernel-trace --stats -d DIR -o nb -- python profiles/neighbors_bench.py --trace-only      (a run of its own)
    python profiles/neighbors_bench.py --merge-stats DIR/.../nb_kernel_stats.csv --out profiles/neighbors_mi355x.json

The world: 65 536 drones uniform in 181 x 181 x 8 m (0.25 drones per cubic metre, 14 neighbours within 2.5 m on average), radius
2.5 m.  Three things are timed with device events in ONE process, in turns, each until it has run for at least 0.25 s after warm-up:
  neighbors   `SwarmAviary.neighbors(2.5, k)` for k = 8 and 16: count + scatter (+ scan) + search, `rel` included
  torch       what a user writes without it: `torch.cdist` in chunks of 4 096 rows + `topk` + the count, the same outputs
  forces      one binning + one downwash sweep of the same swarm (`gpd_swarm_bin` + `gpd_swarm_forces`, 10.5 m cells, no wake
              lists): the same counting sort on coarser cells, for scale
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd.envs import SwarmAviary  # noqa: E402
from gym_pybullet_drones_amd.utils.enums import Physics  # noqa: E402

N, RADIUS, MIN_SECONDS = 65536, 2.5, 0.25


def world():
    rng = np.random.default_rng(1)
    return (rng.uniform(0, 1, (N, 3)) * [181.0, 181.0, 8.0]).astype(np.float32)


def torch_baseline(pos, radius, k, chunk=4096):
    """count / idx / rel of `neighbors()` from all pairs: 4.3e9 distances per call"""
    n = pos.shape[0]
    count = torch.empty(n, dtype=torch.int32, device=pos.device)
    idx = torch.empty((n, k), dtype=torch.int64, device=pos.device)
    dist = torch.empty((n, k), dtype=torch.float32, device=pos.device)
    rows = torch.arange(n, device=pos.device)
    for lo in range(0, n, chunk):
        d = torch.cdist(pos[lo:lo + chunk], pos)
        d[rows[:d.shape[0]], rows[lo:lo + chunk]] = float("inf")          # not its own neighbour
        count[lo:lo + chunk] = (d < radius).sum(dim=1)
        dist[lo:lo + chunk], idx[lo:lo + chunk] = torch.topk(d, k, dim=1, largest=False)
    far = dist >= radius
    rel = torch.cat([pos[idx] - pos[:, None, :], dist[..., None]], dim=-1)
    return count, idx.masked_fill(far, -1), rel.masked_fill(far[..., None], 0.0)


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
    ap.add_argument("--trace-only", action="store_true", help="only the neighbour queries, 50 calls per k (for rocprofv3)")
    ap.add_argument("--merge-stats", default=None, help="kernel_stats.csv of the traced run: adds the per-kernel split to --out")
    a = ap.parse_args()
    if a.merge_stats:
        res = json.load(open(a.out))
        rows = list(csv.DictReader(open(a.merge_stats)))
        keep = ("nbr_world_kernel", "dwg_count_kernel", "dwg_scatter_kernel", "dwg_scan_kernel")
        res["rocprofv3_kernel_stats"] = [{"kernel": r["Name"], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) * 1e-3}
                                         for r in rows if any(s in r["Name"] for s in keep)]
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(res["rocprofv3_kernel_stats"]))
        return
    dev = torch.device("cuda:0")
    xyz = world()
    env = SwarmAviary(N, initial_xyzs=xyz, physics=Physics.PYB_DW, wake_lists=False, rebin_every=1, device=dev)
    env.reset()
    pos = env.core.positions(N).contiguous()
    jobs = {"neighbors_k8": (lambda: env.neighbors(RADIUS, 8), 50), "neighbors_k16": (lambda: env.neighbors(RADIUS, 16), 50)}
    if not a.trace_only:
        jobs["torch_cdist_topk_k8"] = (lambda: torch_baseline(pos, RADIUS, 8), 1)
        jobs["torch_cdist_topk_k16"] = (lambda: torch_baseline(pos, RADIUS, 16), 1)

        def sweep():
            env._since_bin = env.rebin_every                 # (a binning is due: every call sorts, as every neighbour query does)
            env._forces()
        jobs["bin_and_force_sweep"] = (sweep, 50)
        # the two ways agree before either is timed (torch.cdist takes its matrix-multiply route at this size: pairs within its
        # rounding of the radius, or of each other, may come out differently)
        got, (c, i, r) = env.neighbors(RADIUS, 16), torch_baseline(pos, RADIUS, 16)
        assert (got.count != c).float().mean() < 0.01 and (got.idx.long() == i).float().mean() > 0.99
    for fn, _ in jobs.values():                              # warm-up
        fn()
    torch.cuda.synchronize()
    if a.trace_only:
        for fn, calls in jobs.values():
            timed(fn, calls)
        return
    spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)
    while min(spent.values()) < MIN_SECONDS:                 # in turns: what drifts, drifts for all of them
        for name, (fn, calls) in jobs.items():
            if spent[name] < MIN_SECONDS:
                spent[name] += timed(fn, calls)
                done[name] += calls
    res = {"device": torch.cuda.get_device_name(0), "drones": N, "radius_m": RADIUS, "box_m": [181, 181, 8],
           "mean_neighbours": float(env.neighbors(RADIUS, 8).count.float().mean()),
           "per_call_us": {k: spent[k] / done[k] * 1e6 for k in jobs}, "calls": done,
           "seconds_timed": {k: round(v, 3) for k, v in spent.items()}}
    u = res["per_call_us"]
    res["speedup_over_torch"] = {"k8": u["torch_cdist_topk_k8"] / u["neighbors_k8"], "k16": u["torch_cdist_topk_k16"] / u["neighbors_k16"]}
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

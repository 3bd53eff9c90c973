#!/usr/bin/env python3
"""What the obstacle queries cost at 65 536 drones, and what they are measured against.

    python profiles/obstacles_bench.py [--out profiles/obstacles_mi355x.json]

The scene: 65 536 drones uniform in 64 x 64 x 3 m, ONE shared list of 64 obstacles (21 spheres, 21 boxes, 21 cylinders, a floor), a
fan of 16 rays in the body frame, max_range 5 m.  Timed with device events in ONE process, in turns, each until it has run for at
least 0.25 s after warm-up:
  clearance / scan / both   `gpd_obstacles` through `obstacles.FieldQuery` (one launch, one launch, two launches)
  torch_*                   the same query as a user writes it in torch: every shape of a kind at once as [N, M_kind(, R)] temporaries,
                            then the minimum over the obstacles (the scan in chunks of 8 192 drones)
No time is a pass condition; the two ways are compared before either is timed.
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gym_pybullet_drones_amd import _native, obstacles as ob  # noqa: E402

N, M_KIND, RAYS, MAX_RANGE, RADIUS, MIN_SECONDS = 65536, 21, 16, 5.0, 0.06, 0.25
INF = float("inf")


def scene():
    rng = np.random.default_rng(1)
    f = ob.ObstacleField()
    centre = lambda: rng.uniform([0, 0, 0.3], [64, 64, 2.7])          # noqa: E731
    for _ in range(M_KIND):
        f.sphere(centre(), rng.uniform(0.5, 2.0))
    for _ in range(M_KIND):
        f.box(centre(), rng.uniform(0.5, 2.0, 3))
    for _ in range(M_KIND):
        f.cylinder(centre(), rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5))
    f.floor(0.0)
    pos = rng.uniform([0, 0, 0.05], [64, 64, 3.0], (N, 3)).astype(np.float32)
    q = rng.normal(size=(N, 4))
    return f, pos, (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def quat_rotate(q, d):
    """[n, 4] unit quaternions (x, y, z, w) x [R, 3] -> [n, R, 3]"""
    x, y, z, w = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).view(-1, 3, 3)
    return torch.einsum("nij,rj->nri", R, d)


class TorchQuery:
    """the torch restatement on the shared list, the obstacles grouped by kind on the host"""

    def __init__(self, rec, dev):
        t = torch.as_tensor(rec, dtype=torch.float32, device=dev)
        self.groups = {k: (t[rec[:, 3] == k, 0:3], t[rec[:, 3] == k, 4:7], torch.as_tensor(np.flatnonzero(rec[:, 3] == k), device=dev))
                       for k in (ob.SPHERE, ob.BOX, ob.CYLINDER, ob.FLOOR)}

    def clearance(self, p):
        ds, ns, ids = [], [], []
        for k, (c, a, idx) in self.groups.items():
            v = p[:, None, :] - c[None]
            if k == ob.SPHERE:
                ln = v.norm(dim=-1)
                d, n = ln - a[:, 0], v / ln.clamp_min(1e-30)[..., None]
            elif k == ob.BOX:
                q = v.abs() - a
                o = q.clamp_min(0.0)
                out = o.norm(dim=-1)
                d = out + q.max(dim=-1).values.clamp_max(0.0)
                inside = torch.nn.functional.one_hot(q.argmax(dim=-1), 3).float()
                n = torch.where((out > 0)[..., None], o / out.clamp_min(1e-30)[..., None], inside) * torch.where(v < 0, -1.0, 1.0)
            elif k == ob.CYLINDER:
                rho = v[..., :2].norm(dim=-1)
                qr, qz = rho - a[:, 0], v[..., 2].abs() - a[:, 2]
                orr, oz = qr.clamp_min(0.0), qz.clamp_min(0.0)
                out = torch.sqrt(orr * orr + oz * oz)
                d = out + torch.maximum(qr, qz).clamp_max(0.0)
                wr = torch.where(out > 0, orr / out.clamp_min(1e-30), (qr >= qz).float())
                wz = torch.where(out > 0, oz / out.clamp_min(1e-30), (qr < qz).float())
                n = torch.cat([v[..., :2] / rho.clamp_min(1e-30)[..., None] * wr[..., None], (torch.where(v[..., 2] < 0, -1.0, 1.0) * wz)[..., None]], dim=-1)
            else:
                d, n = v[..., 2], torch.tensor([0.0, 0.0, 1.0], device=p.device).expand(v.shape)
            ds.append(d); ns.append(n); ids.append(idx)
        d, n, ids = torch.cat(ds, dim=1), torch.cat(ns, dim=1), torch.cat(ids)
        best, j = d.min(dim=1)
        return torch.cat([n[torch.arange(len(p), device=p.device), j], best[:, None]], dim=1), ids[j], best < RADIUS

    @staticmethod
    def _slab(v, d, a, t0, t1):
        par = d == 0
        inv = 1.0 / torch.where(par, torch.ones_like(d), d)
        ta, tb = (-a - v) * inv, (a - v) * inv
        return (torch.where(par, t0, torch.maximum(t0, torch.minimum(ta, tb))),
                torch.where(par, torch.where(v.abs() > a, torch.full_like(t1, -INF), t1), torch.minimum(t1, torch.maximum(ta, tb))))

    def scan(self, p, q, dirs, chunk=8192):
        out = torch.empty((len(p), len(dirs)), dtype=torch.float32, device=p.device)
        for lo in range(0, len(p), chunk):
            pc = p[lo:lo + chunk]
            d = quat_rotate(q[lo:lo + chunk], dirs)[:, None]                       # [n, 1, R, 3]
            ts = []
            for k, (c, a, _) in self.groups.items():
                v = (pc[:, None, :] - c[None])[:, :, None, :].expand(-1, -1, d.shape[2], -1)      # [n, M, R, 3]
                dd = d.expand_as(v)
                zero, inf = torch.zeros_like(v[..., 0]), torch.full_like(v[..., 0], INF)
                if k == ob.SPHERE:
                    r = a[None, :, None, 0]
                    b, cc = (v * dd).sum(-1), (v * v).sum(-1) - r * r
                    disc = b * b - cc
                    t = torch.where(cc <= 0, zero, torch.where((b < 0) & (disc >= 0), cc / (disc.clamp_min(0).sqrt() - b), inf))
                elif k == ob.BOX:
                    t0, t1 = zero, inf
                    for i in range(3):
                        t0, t1 = self._slab(v[..., i], dd[..., i], a[None, :, None, i], t0, t1)
                    t = torch.where(t0 <= t1, t0, inf)
                elif k == ob.CYLINDER:
                    r = a[None, :, None, 0]
                    aa = (dd[..., :2] ** 2).sum(-1)
                    bb, cc = (v[..., :2] * dd[..., :2]).sum(-1), (v[..., :2] ** 2).sum(-1) - r * r
                    vert = aa == 0
                    sa = torch.where(vert, torch.ones_like(aa), aa)
                    disc = bb * bb - sa * cc
                    rt = disc.clamp_min(0).sqrt()
                    lo_t = torch.where(vert, torch.where(cc > 0, inf, zero), torch.where(disc >= 0, ((-bb - rt) / sa).clamp_min(0), inf))
                    hi_t = torch.where(vert, torch.where(cc > 0, -inf, inf), torch.where(disc >= 0, (-bb + rt) / sa, -inf))
                    t0, t1 = self._slab(v[..., 2], dd[..., 2], a[None, :, None, 2], lo_t, hi_t)
                    t = torch.where(t0 <= t1, t0, inf)
                else:
                    t = torch.where(v[..., 2] <= 0, zero, torch.where(dd[..., 2] < 0, v[..., 2] / (-dd[..., 2]).clamp_min(1e-30), inf))
                ts.append(t)
            out[lo:lo + chunk] = torch.cat(ts, dim=1).min(dim=1).values.clamp_max(MAX_RANGE)
        return out


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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    field, pos, quat = scene()
    pos4 = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    pos4[:, :3] = torch.as_tensor(pos, device=dev)
    quat4 = torch.as_tensor(quat, device=dev)
    dirs = torch.as_tensor(ob.fan(RAYS, math.pi), device=dev)
    q = ob.FieldQuery(field, dev, N, 1, RADIUS)
    tq = TorchQuery(field.records(), dev)
    p3 = pos4[:, :3].contiguous()
    stream = lambda: ctypes.c_void_p(_native.raw_stream(dev))                      # noqa: E731
    jobs = {"clearance": (lambda: q.clearance(pos4, stream()), 50),
            "scan": (lambda: q.scan(pos4, quat4, dirs, MAX_RANGE, "body", False, stream()), 50),
            "both": (lambda: (q.clearance(pos4, stream()), q.scan(pos4, quat4, dirs, MAX_RANGE, "body", False, stream())), 50),
            "torch_clearance": (lambda: tq.clearance(p3), 5),
            "torch_scan": (lambda: tq.scan(p3, quat4, dirs), 1),
            "torch_both": (lambda: (tq.clearance(p3), tq.scan(p3, quat4, dirs)), 1)}
    # the two ways agree before either is timed (fp32 both: grazing rays and near ties may differ)
    c, (ranges, _) = q.clearance(pos4, stream()), q.scan(pos4, quat4, dirs, MAX_RANGE, "body", False, stream())
    c4, near, hit = tq.clearance(p3)
    assert ((c.dist - c4[:, 3]).abs() < 1e-4).float().mean() > 0.999 and (c.nearest.long() == near).float().mean() > 0.99
    assert ((ranges - tq.scan(p3, quat4, dirs)).abs() < 1e-3).float().mean() > 0.99
    for fn, _ in jobs.values():                              # warm-up
        fn()
    torch.cuda.synchronize()
    spent, done = dict.fromkeys(jobs, 0.0), dict.fromkeys(jobs, 0)
    while min(spent.values()) < MIN_SECONDS:                 # in turns: what drifts, drifts for all of them
        for name, (fn, calls) in jobs.items():
            if spent[name] < MIN_SECONDS:
                spent[name] += timed(fn, calls)
                done[name] += calls
    res = {"device": torch.cuda.get_device_name(0), "drones": N, "obstacles": len(field), "rays": RAYS, "max_range_m": MAX_RANGE,
           "share_colliding": float(c.hit.float().mean()), "share_of_rays_hitting": float((ranges < MAX_RANGE).float().mean()),
           "per_call_us": {k: spent[k] / done[k] * 1e6 for k in jobs}, "calls": done, "seconds_timed": {k: round(v, 3) for k, v in spent.items()}}
    u = res["per_call_us"]
    res["speedup_over_torch"] = {k: u["torch_" + k] / u[k] for k in ("clearance", "scan", "both")}
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

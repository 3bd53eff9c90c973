"""Obstacle fields on the device: the binding of `gpd_obstacles` (include/gpd.h) shared by `VectorAviary` and `SwarmAviary` --
`set_obstacles()`, `clearance()`, `range_scan()`, `obstacle_hits()`.

The reference puts bodies into the Bullet world (`BaseAviary._addObstacles`, `envs/BaseAviary.py:958-981`; `BaseRLAviary._addObstacles`,
`envs/BaseRLAviary.py:99-128`) and has no query about them.  Here the world is a list of analytic shapes -- spheres, axis-aligned
boxes, vertical cylinders, a floor -- and a drone learns how far the nearest one is and in which direction, whether it collides
(the drone as a sphere of `COLLISION_R`), and what a fan of range sensors sees, as device tensors with no host synchronisation.
Nothing acts on the integrator: a user combines `hit` into their own termination.
"""
import math

import numpy as np
import torch

from . import _native

NONE, SPHERE, BOX, CYLINDER, FLOOR = -1, 0, 1, 2, 3
MAX_OBSTACLES, MAX_RAYS = 1024, 64
FRAMES = {"world": 0, "level": 1, "body": 2}


class ObstacleField:
    """A list of obstacles, shared by every drone (`num_envs=None`) or one list per aviary (`num_envs=E`: every builder then takes
    one value, used by all aviaries, or E of them).  Builders return the field, so they chain."""

    def __init__(self, num_envs: int = None):
        self.num_envs = None if num_envs is None else int(num_envs)
        if self.num_envs is not None and self.num_envs < 1:
            raise ValueError("num_envs must be positive")
        self._records = []                       # each [8] (shared) or [E, 8]

    def __len__(self):
        return len(self._records)

    def _add(self, kind, centre, size):
        lead = () if self.num_envs is None else (self.num_envs,)
        rec = np.zeros(lead + (8,), dtype=np.float64)
        try:
            rec[..., 0:3] = np.asarray(centre, dtype=np.float64)
            rec[..., 4:7] = np.asarray(size, dtype=np.float64)
        except ValueError as e:
            raise ValueError(f"an obstacle's centre and sizes are 3 values{' or [num_envs, 3]' if lead else ''}: {e}") from None
        rec[..., 3] = np.asarray(kind, dtype=np.float64)
        if not np.isfinite(rec).all() or (rec[..., 4:7] < 0).any():
            raise ValueError("an obstacle's centre and sizes must be finite and its sizes non-negative")
        if len(self._records) >= MAX_OBSTACLES:
            raise ValueError(f"at most {MAX_OBSTACLES} obstacles per list")
        self._records.append(rec)
        return self

    @staticmethod
    def _sizes(*cols):
        cols = np.broadcast_arrays(*[np.asarray(c, dtype=np.float64) for c in cols])
        return np.stack(cols, axis=-1)

    def sphere(self, centre, radius):
        return self._add(SPHERE, centre, self._sizes(radius, 0.0, 0.0))

    def box(self, centre, half_extents):
        """axis-aligned, `half_extents` (hx, hy, hz)"""
        return self._add(BOX, centre, half_extents)

    def cylinder(self, centre, radius, half_height):
        """vertical: the axis is z"""
        return self._add(CYLINDER, centre, self._sizes(radius, 0.0, half_height))

    def floor(self, z=0.0):
        """the half-space below `z`"""
        z = np.asarray(z, dtype=np.float64)
        return self._add(FLOOR, self._sizes(0.0, 0.0, z), (0.0, 0.0, 0.0))

    def none(self, where=None):
        """a record that is skipped; per-aviary fields: `where` [E] bool turns the LAST record into one for those aviaries
        (lists of different lengths)"""
        if where is None:
            return self._add(NONE, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
        if self.num_envs is None or not self._records:
            raise ValueError("none(where) needs a per-aviary field with a record to blank")
        self._records[-1][np.asarray(where, dtype=bool), 3] = NONE
        return self

    @classmethod
    def random_cylinders(cls, num_envs: int, count: int, area, radius_range, height_range, generator=None):
        """A course per aviary: `count` cylinders standing on z = 0, centres uniform in `area` = (x0, y0, x1, y1), radius and HEIGHT
        uniform in their ranges; `generator`: a `numpy.random.Generator` (None: a fresh one)."""
        rng = np.random.default_rng() if generator is None else generator
        x0, y0, x1, y1 = (float(v) for v in area)
        f = cls(num_envs)
        for _ in range(int(count)):
            xy = rng.uniform((x0, y0), (x1, y1), size=(f.num_envs, 2))
            r = rng.uniform(*radius_range, size=f.num_envs)
            h = rng.uniform(*height_range, size=f.num_envs)
            f.cylinder(np.concatenate([xy, 0.5 * h[:, None]], axis=1), r, 0.5 * h)
        return f

    def records(self) -> np.ndarray:
        """[M, 8] or [E, M, 8] float64"""
        if not self._records:
            raise ValueError("the field has no obstacle")
        return np.stack(self._records, axis=-2)

    @property
    def obst_ld(self) -> int:
        return 1 if self.num_envs is None else self.num_envs

    def table(self, device) -> torch.Tensor:
        """The tensor in the entry's layout: shared [M, 8]; per aviary [M * 8, E] field planes (float f of record m of aviary e at
        `[(m * 8 + f), e]`, `obst_ld = E`)."""
        rec = self.records().astype(np.float32)
        if self.num_envs is not None:
            rec = np.ascontiguousarray(rec.transpose(1, 2, 0)).reshape(-1, self.num_envs)
        return torch.as_tensor(rec).to(device).contiguous()


def fan(n_rays: int, fov: float, elevation: float = 0.0) -> np.ndarray:
    """[n_rays, 3] float32 unit directions spread evenly over `fov` radians about +x (the body's nose) at `elevation` radians above
    the horizon; one ray looks straight ahead; `fov = 2 pi` is the full circle without the doubled end."""
    n_rays = int(n_rays)
    if not 1 <= n_rays <= MAX_RAYS:
        raise ValueError(f"n_rays must be in 1..{MAX_RAYS}, got {n_rays}")
    fov = float(fov)
    if not 0.0 <= fov <= 2.0 * math.pi + 1e-9:
        raise ValueError("fov must be in 0..2 pi")
    if n_rays == 1:
        az = np.zeros(1)
    elif fov >= 2.0 * math.pi - 1e-9:
        az = np.arange(n_rays) * (2.0 * math.pi / n_rays)
    else:
        az = np.linspace(-0.5 * fov, 0.5 * fov, n_rays)
    ce, se = math.cos(elevation), math.sin(elevation)
    d = np.stack([ce * np.cos(az), ce * np.sin(az), np.full(n_rays, se)], axis=1)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


class Clearance:
    """What `clearance()` returns (device tensors):
    `normal`  float32 `(..., 3)`: the unit gradient of the nearest obstacle's distance -- the direction AWAY from it
    `dist`    float32: the signed distance to it, negative inside; +inf without any obstacle (or for a drone without a position)
    `nearest` int32: its record, -1 for none
    `hit`     bool: `dist < collision_radius`"""
    __slots__ = ("normal", "dist", "nearest", "hit")

    def __init__(self, normal, dist, nearest, hit):
        self.normal, self.dist, self.nearest, self.hit = normal, dist, nearest, hit


class FieldQuery:
    """One field bound to `n` rows of D-drone aviaries on a device: the table, and the output tensors of the clearance and of each
    (rays, ids) shape, allocated once and reused by every call."""

    def __init__(self, field: ObstacleField, device, n: int, drones_per_env: int, collision_radius: float):
        self.n, self.D, self.device = int(n), int(drones_per_env), device
        if field.num_envs is not None and (self.D < 1 or field.num_envs != self.n // self.D):
            raise ValueError(f"the field has a list for each of {field.num_envs} aviaries; the simulation has {self.n // self.D if self.D else 1}")
        self.n_obst, self.obst_ld = len(field), field.obst_ld
        self.obst = field.table(device)
        self.collision_radius = float(collision_radius)
        f32 = dict(dtype=torch.float32, device=device)
        self._clear4 = torch.zeros((self.n, 4), **f32)
        self._nearest = torch.zeros(self.n, dtype=torch.int32, device=device)
        self._hit = torch.zeros(self.n, dtype=torch.uint8, device=device)
        self._scans = {}

    def clearance(self, pos4, stream) -> Clearance:
        _native.call("gpd_obstacles", self.device, stream, pos4, None, self.n, self.D, self.obst, self.n_obst, self.obst_ld, self.collision_radius,
                     self._clear4, self._nearest, self._hit, None, 0, 0, 0.0, None, None)
        return Clearance(self._clear4[:, :3], self._clear4[:, 3], self._nearest, self._hit.view(torch.bool))

    def hits(self, pos4, stream) -> torch.Tensor:
        _native.call("gpd_obstacles", self.device, stream, pos4, None, self.n, self.D, self.obst, self.n_obst, self.obst_ld, self.collision_radius,
                     None, None, self._hit, None, 0, 0, 0.0, None, None)
        return self._hit.view(torch.bool)          # (the kernel writes 0 / 1: the same bytes)

    def scan(self, pos4, quat4, dirs, max_range, frame, want_ids, stream):
        code = FRAMES.get(frame)
        if code is None:
            raise ValueError(f"frame must be one of {', '.join(FRAMES)}, got {frame!r}")
        max_range = float(max_range)
        if not (max_range > 0.0 and math.isfinite(max_range)):
            raise ValueError(f"max_range must be positive and finite, got {max_range}")
        if not (isinstance(dirs, torch.Tensor) and dirs.device == self.device and dirs.dtype == torch.float32 and dirs.is_contiguous()):
            dirs = torch.as_tensor(np.asarray(dirs.cpu() if isinstance(dirs, torch.Tensor) else dirs, dtype=np.float32)).to(self.device).contiguous()
        if dirs.ndim != 2 or dirs.shape[1] != 3 or not 1 <= dirs.shape[0] <= MAX_RAYS:
            raise ValueError(f"dirs must be [1..{MAX_RAYS}, 3] unit vectors, got {tuple(dirs.shape)}")
        R = dirs.shape[0]
        key = (R, bool(want_ids))
        out = self._scans.get(key)
        if out is None:
            out = self._scans[key] = (torch.zeros((self.n, R), dtype=torch.float32, device=self.device),
                                      torch.zeros((self.n, R), dtype=torch.int32, device=self.device) if want_ids else None)
        _native.call("gpd_obstacles", self.device, stream, pos4, quat4, self.n, self.D, self.obst, self.n_obst, self.obst_ld, self.collision_radius,
                     None, None, None, dirs, R, code, max_range, out[0], out[1])
        return out

"""Obstacle queries at degenerate geometry: scenes on which an exact zero, an exact tie or an exact threshold is the rule and not the
accident -- a lattice of dyadic points around one record of every kind, a corridor with the drone on its centre line, points and rays
exactly at `radius` / `max_range` -- with axis-parallel rays, and the comparison that leaves NOTHING out: on dyadic inputs with axis
rays float32 and float64 take the same side of every test, so classes (inf / 0 / positive, the sign of d) and indices must be
identical and the values agree to a few roundings.  The answers are tests/helpers/obstacles_f64.py's on the float32 inputs.  Shared by
tests/test_host_obstacles.py (the C text on the host) and the two device modules.  Test infrastructure, no GPU needed."""
import collections
import functools

import numpy as np

import obstacles_f64 as y

#: |x32 - x64| / max(1, |x64|) on these scenes: every product and sum of dyadic numbers is exact in float32, what remains is at most a
#: square root, a division and a product, each correctly rounded (6e-8 each); four times that chain
BOUND = 1e-6
#: the radius and the range of the threshold cases (dyadic: both formats agree on which side a point lies)
RADIUS, RANGE = 0.0625, 2.0
#: the non-axis scans: the lattice moved off itself by this much (tests/test_host_obstacles.py holds the caps on it)
SHIFT = (0.0137, 0.0071, 0.0093)
N_YAWS = 37

Scene = collections.namedtuple("Scene", "name obst pos")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def up(x):
    """the float32 one ulp above x"""
    return np.nextafter(np.float32(x), np.float32(np.inf))


def grid(lo, hi, step):
    return lo + step * np.arange(int(round((hi - lo) / step)) + 1)


@functools.lru_cache(maxsize=None)
def lattice():
    """one record of every kind and 1 650 points on a quarter-metre grid around them (y with both zeros): 5.7 % on a surface, 2.5 %
    inside, 90 exact ties of the two nearest records"""
    obst = [y.record(y.SPHERE, (0, 0, 1), (0.5, 0, 0)), y.record(y.BOX, (2, 0, 1), (0.5, 0.25, 1)), y.record(y.CYLINDER, (-2, 0, 1), (0.5, 0, 1)),
            y.record(y.FLOOR)]
    ys = np.array([-0.5, -0.25, -0.0, 0.0, 0.25, 0.5])
    pos = np.stack(np.meshgrid(grid(-3.0, 3.0, 0.25), ys, grid(0.0, 2.5, 0.25), indexing="ij"), axis=-1).reshape(-1, 3)
    return Scene("lattice", _f32(obst), _f32(pos))


@functools.lru_cache(maxsize=None)
def corridor():
    """two walls and two pillars, mirror images in y, over a floor; 68 points on the centre line, 40 of them exactly as far from a
    record as from its mirror image: `nearest` is the lower one"""
    obst = [y.record(y.BOX, (0, 1, 1), (4, 0.25, 1)), y.record(y.BOX, (0, -1, 1), (4, 0.25, 1)), y.record(y.CYLINDER, (1, 0.5, 1), (0.25, 0, 1)),
            y.record(y.CYLINDER, (1, -0.5, 1), (0.25, 0, 1)), y.record(y.FLOOR)]
    pos = np.stack(np.meshgrid(grid(-2.0, 2.0, 0.25), [0.0], [0.25, 0.5, 0.75, 1.0], indexing="ij"), axis=-1).reshape(-1, 3)
    return Scene("corridor", _f32(obst), _f32(pos))


def twins(obst):
    """every solid record duplicated right after itself: the first twin is the answer"""
    rows = []
    for r in obst:
        rows += [r, r] if r[3] in (y.SPHERE, y.BOX, y.CYLINDER) else [r]
    return _f32(rows)


def with_none(obst):
    """a skipped record (with a size that must not be looked at) before every record and after the last"""
    none = _f32(y.record(y.NONE, (0, 0, 1), (9, 9, 9)))
    rows = []
    for r in obst:
        rows += [none, r]
    return _f32(rows + [none])


def padded(obst, n, front=0):
    """`obst` with `front` skipped records before it and skipped records after it up to n"""
    none = _f32(y.record(y.NONE, (0, 0, 1), (9, 9, 9)))
    assert front + len(obst) <= n
    return _f32([none] * front + list(obst) + [none] * (n - front - len(obst)))


def rotated(obst, n):
    """[n, M, 8]: list e is `obst` with its record order rotated by e -- the lanes of a wave hold different kinds at the same m"""
    M = len(obst)
    return _f32([obst[(np.arange(M) + e) % M] for e in range(n)])


@functools.lru_cache(maxsize=None)
def scenes():
    """every scene of the zero-exclusion comparisons: name -> Scene"""
    la, co = lattice(), corridor()
    out = [la, co, Scene("lattice-twins", twins(la.obst), la.pos), Scene("lattice-none", with_none(la.obst), la.pos),
           Scene("corridor-none", with_none(co.obst), co.pos)]
    return {s.name: s for s in out}


def axis_dirs():
    """the six axis directions, and two with negative zeros"""
    return _f32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, -0.0, -0.0], [-0.0, -0.0, -1]])


def per_point(dirs, n):
    """a table of directions [R, 3] as what every one of n points casts: [n, R, 3]"""
    return np.ascontiguousarray(np.broadcast_to(dirs, (n,) + dirs.shape))


Threshold = collections.namedtuple("Threshold", "name record point nearer origin ray")


@functools.lru_cache(maxsize=None)
def thresholds():
    """`(obst, cases)` on the lattice's list.  For every kind of surface `point` lies exactly RADIUS outside it along an axis (no hit at
    radius RADIUS), `nearer` one float32 ulp closer (a hit), and the axis ray `ray` (an index into axis_dirs()) from `origin` enters
    record `record` at exactly RANGE (not seen at max_range RANGE, seen one ulp above)."""
    f = np.float32

    def nearer(p, axis, towards):
        q = np.array(p, dtype=np.float32)
        q[axis] = np.nextafter(q[axis], f(towards))
        return tuple(q)

    r, R = RADIUS, RANGE
    cases = [
        Threshold("sphere", 0, (0, 0.5 + r, 1), nearer((0, 0.5 + r, 1), 1, 0), (0, 0.5 + R, 1), 3),
        Threshold("box-face", 1, (2, -0.25 - r, 1), nearer((2, -0.25 - r, 1), 1, 0), (2, -0.25 - R, 1), 2),
        Threshold("cylinder-wall", 2, (-2, 0.5 + r, 1), nearer((-2, 0.5 + r, 1), 1, 0), (-2, 0.5 + R, 1), 3),
        Threshold("cylinder-cap", 2, (-1.75, 0, 2 + r), nearer((-1.75, 0, 2 + r), 2, 0), (-1.75, 0, 2 + R), 5),
        Threshold("floor", 3, (1, 1, r), nearer((1, 1, r), 2, 0), (1, 1, R), 7),
    ]
    return lattice().obst, cases


def threshold_points():
    """[10, 3]: the five points exactly RADIUS outside, then the five one ulp nearer"""
    _, cases = thresholds()
    return _f32([c.point for c in cases] + [c.nearer for c in cases])


def threshold_origins():
    _, cases = thresholds()
    return _f32([c.origin for c in cases])


# ---- what a scene exists for --------------------------------------------------------------------------------------------------------------
def census(scene, dirs=None):
    """counts of the categories a scene exists for (float64 on the float32 inputs: exact for dyadic numbers)"""
    obst, p = np.asarray(scene.obst, dtype=np.float64), np.asarray(scene.pos, dtype=np.float64)
    dirs = np.asarray(axis_dirs() if dirs is None else dirs, dtype=np.float64)
    kind = obst[:, 3]
    v = p[:, None, :] - obst[None, :, 0:3]                                   # [N, M, 3]
    a = np.broadcast_to(obst[None, :, 4:7], v.shape)
    d, _ = y.sdf(obst, p)
    c = collections.OrderedDict()
    box, cyl, sph, floor = kind == y.BOX, kind == y.CYLINDER, kind == y.SPHERE, kind == y.FLOOR
    # rays parallel to a slab of a box: [N, M, R, 3]
    par = np.broadcast_to((dirs == 0)[None, None], v.shape[:2] + dirs.shape) & box[None, :, None, None]
    inside = (np.abs(v) <= a)[:, :, None, :]
    c["slab_parallel_inside"] = int((par & inside).sum())
    c["slab_parallel_outside"] = int((par & ~inside).sum())
    # vertical rays on a cylinder, by the sign of c = rho^2 - r^2
    n_vert = int(((dirs[:, 0] == 0) & (dirs[:, 1] == 0)).sum())
    cc = v[..., 0] ** 2 + v[..., 1] ** 2 - a[..., 0] ** 2
    for name, m in (("vertical_ray_c_negative", cc < 0), ("vertical_ray_c_zero", cc == 0), ("vertical_ray_c_positive", cc > 0)):
        c[name] = int((m & cyl[None]).sum()) * n_vert
    c["level_ray_above_floor"] = int(((v[..., 2] > 0) & floor[None]).sum()) * int((dirs[:, 2] == 0).sum())
    for name, k in (("sphere", sph), ("box", box), ("cylinder", cyl), ("floor", floor)):
        for where, m in (("inside", d < 0), ("on", d == 0), ("outside", d > 0)):
            if (name, where) != ("floor", "inside"):                         # (no point of these scenes lies below the ground)
                c[f"origin_{where}_{name}"] = int((m & k[None]).sum())
    touching = ((np.abs(v) == a) & (np.abs(v) <= a).all(axis=-1, keepdims=True)).sum(axis=-1)
    for name, count in (("box_face", 1), ("box_edge", 2), ("box_corner", 3)):
        c[name] = int(((touching == count) & box[None]).sum())
    rho = np.hypot(v[..., 0], v[..., 1])
    c["cylinder_axis"] = int(((rho == 0) & cyl[None]).sum())
    c["cylinder_rim"] = int(((rho == a[..., 0]) & (np.abs(v[..., 2]) == a[..., 2]) & cyl[None]).sum())
    c["cylinder_centre"] = int(((v == 0).all(axis=-1) & cyl[None]).sum())
    c["sphere_centre"] = int(((v == 0).all(axis=-1) & sph[None]).sum())
    c["negative_zero_coordinate"] = int((np.signbit(scene.pos) & (scene.pos == 0)).sum())
    c["negative_zero_direction"] = int((np.signbit(dirs) & (dirs == 0)).sum())
    cl = y.clearance(obst, p)
    c["tie_of_the_nearest"] = int((np.isfinite(cl["d"]) & (cl["second"] == cl["d"])).sum())
    sc = y.scan(obst, p, per_point(dirs, len(p)), y.MAX_RANGE)
    c["tie_of_the_first_entry"] = int((np.isfinite(sc["entry"]) & (sc["second"] == sc["entry"])).sum())
    return c


#: what the corridor is for; the lattice is for every category
CORRIDOR_CATEGORIES = ("tie_of_the_nearest", "slab_parallel_inside", "slab_parallel_outside", "level_ray_above_floor",
                       "vertical_ray_c_positive", "origin_outside_box", "origin_outside_cylinder")


# ---- the comparison without exclusions --------------------------------------------------------------------------------------------------
def classes(x, cap=np.inf):
    """0: exactly zero, 1: positive (below the cap), 2: the cap or +inf, -1: negative, 3: NaN"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 3, np.where(x >= cap, 2, np.where(x > 0, 1, np.where(x == 0, 0, -1))))


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def compare_pairs(got, obst, pos, dirs):
    """the host program's per-pair values `d` [N, M], `grad` [N, M, 3], `t` [N, M, R] against the yardstick, every entry: identical
    classes, no NaN; returns the largest errors (d, gradient, t)"""
    d64, g64 = y.sdf(obst, pos)
    t64 = y.ray(obst, pos, dirs)
    for name, x64 in (("d", d64), ("grad", g64), ("t", t64)):
        assert not np.isnan(got[name]).any(), name
        _same(classes(got[name]), classes(x64), f"class of {name}")
    return tuple(float(y.rel_err(got[k], w).max()) for k, w in (("d", d64), ("grad", g64), ("t", t64)))


def compare_all(got, obst, pos, dirs=None, radius=y.COLLISION_RADIUS, max_range=y.MAX_RANGE):
    """`got`: any of `clear4` [N, 4], `nearest`, `hit` [N], `ranges`, `ray_hit` [N, R] of a float32 implementation; `obst` [M, 8] or one
    list per point [N, M, 8]; `dirs` [N, R, 3] world directions.  EVERY point and ray: `nearest`, `hit` and `ray_hit` equal to the
    yardstick's, the class of every d and range identical, no NaN; returns the largest errors (d, normal, ranges)."""
    want = y.clearance(obst, pos, radius)
    err_d = err_n = err_r = 0.0
    if got.get("nearest") is not None:
        _same(got["nearest"], want["nearest"], "nearest")
    if got.get("hit") is not None:
        _same(np.asarray(got["hit"]).astype(bool), want["hit"], "hit")
    if got.get("clear4") is not None:
        c = np.asarray(got["clear4"], dtype=np.float64)
        assert not np.isnan(c).any(), "NaN in clear4"
        _same(classes(c[:, 3]), classes(want["d"]), "class of d")
        _same(classes(c[:, :3]), classes(want["normal"]), "class of the normal")
        err_d, err_n = float(y.rel_err(c[:, 3], want["d"]).max()), float(y.rel_err(c[:, :3], want["normal"]).max())
    if got.get("ranges") is not None:
        s = y.scan(obst, pos, dirs, float(max_range))
        r = np.asarray(got["ranges"], dtype=np.float64)
        assert not np.isnan(r).any(), "NaN in ranges"
        _same(classes(r, float(max_range)), classes(s["ranges"], float(max_range)), "class of ranges")
        if got.get("ray_hit") is not None:
            _same(got["ray_hit"], s["ray_hit"], "ray_hit")
        err_r = float(y.rel_err(r, s["ranges"]).max())
    return err_d, err_n, err_r


# ---- the frames --------------------------------------------------------------------------------------------------------------------------
#: identity and the half turns about x, y, z (x, y, z, w), and the signs their rotation matrices give the three axes
HALF_TURNS = (((0, 0, 0, 1), (1, 1, 1)), ((1, 0, 0, 0), (1, -1, -1)), ((0, 1, 0, 0), (-1, 1, -1)), ((0, 0, 1, 0), (-1, -1, 1)))
SCALES = (1.0, 2.0, 0.5)


# ---- non-axis rays -----------------------------------------------------------------------------------------------------------------------
def shifted_lattice():
    """`(pos [1650, 3], quat [1650, 4])`: the lattice moved by SHIFT, point i turned about z by yaw (i mod 37) * 2 pi / 37"""
    pos = _f32(lattice().pos.astype(np.float64) + np.array(SHIFT))
    yaw = (np.arange(len(pos)) % N_YAWS) * (2.0 * np.pi / N_YAWS)
    quat = np.stack([np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2), np.cos(yaw / 2)], axis=1)
    return pos, _f32(quat)


# ---- the fused kernel's split walk ---------------------------------------------------------------------------------------------------------
def task_lists():
    """{M: [M, 8]} lists of 5, 8, 9 and 65 records for groups of 1 .. 64 lanes: the corridor; the lattice's twins behind one skipped
    record; the corridor with a skipped record between any two; and the walls, 20 skipped records, a pillar, 10 skipped, its mirror
    image, the solid twins, 24 skipped and the floor as record 64 -- with 64 lanes that one shares lane 0 with the first wall"""
    co, tw = corridor().obst, twins(lattice().obst)
    none = [_f32(y.record(y.NONE, (0, 0, 1), (9, 9, 9)))]
    nine = [co[0]] + [r for rec in co[1:] for r in (none[0], rec)]
    long = [co[0], co[1]] + none * 20 + [co[2]] + none * 10 + [co[3]] + list(tw[:6]) + none * 24 + [co[4]]
    out = {5: co, 8: padded(tw, 8, front=1), 9: _f32(nine), 65: _f32(long)}
    assert all(len(v) == k for k, v in out.items())
    return out


def task_points(n):
    """[n, 3]: the corridor's 68 points, then lattice points (every seventh, so that surfaces, ties and both zeros are among them)"""
    pts = np.concatenate([corridor().pos, lattice().pos[3::7]])
    assert n <= len(pts)
    return _f32(pts[:n])

"""The yardstick of the obstacle queries (include/gpd.h gpd_obstacles): a float64 numpy restatement of the geometry -- signed
distance with unit gradient, first entry of a ray -- and of the two reductions, the test scene both suites use, and the rules for
what a comparison with a float32 answer may leave out.  Written from the definitions, not from csrc/obstacle_math.inc; pinned by
analytic known answers in tests/test_host_obstacles.py.  Test infrastructure."""
import numpy as np

NONE, SPHERE, BOX, CYLINDER, FLOOR = -1, 0, 1, 2, 3
MAX_RANGE, COLLISION_RADIUS = 5.0, 0.06
#: the project's ceiling for |x32 - x64| / max(1, |x64|)
CEILING = 1e-4
#: what a comparison may leave out (conditions on the float64 answers alone) and how much of it
GRAZE_MOVE, GRAZE_GROW, NEAR_TIE, ON_THRESHOLD = 1e-3, 1e-4, 1e-4, 1e-4
CAP_RAYS, CAP_DRONES = 0.02, 0.01


def record(kind, centre=(0, 0, 0), size=(0, 0, 0)):
    return [centre[0], centre[1], centre[2], kind, size[0], size[1], size[2], 0.0]


def _side(v):
    return np.where(v < 0, -1.0, 1.0)


def _norm(v):
    return np.sqrt((v * v).sum(axis=-1))


def _lists(obst):
    """obst [M, 8] (one list) or [N, M, 8] (one per point) -> [1 or N, M, 8]"""
    obst = np.asarray(obst, dtype=np.float64)
    return obst[None] if obst.ndim == 2 else obst


def sdf(obst, p):
    """`(d [N, M], grad [N, M, 3])` of the points p [N, 3]: d negative inside, +inf (gradient 0) for NONE"""
    obst, p = _lists(obst), np.asarray(p, dtype=np.float64)
    N, M = len(p), obst.shape[1]
    v = p[:, None, :] - obst[..., 0:3]
    kind = np.broadcast_to(obst[..., 3], (N, M))
    a = np.broadcast_to(obst[..., 4:7], (N, M, 3))
    d, g = np.full((N, M), np.inf), np.zeros((N, M, 3))
    with np.errstate(all="ignore"):
        # sphere: |v| - r; at the centre the gradient is (0, 0, 1)
        ln = _norm(v)
        gs = np.where((ln > 0)[..., None], v / np.where(ln > 0, ln, 1.0)[..., None], np.array([0.0, 0.0, 1.0]))
        # box: |max(q, 0)| + min(max(q), 0), q = |v| - a; inside the axis of least penetration (argmax: the first of equals)
        q = np.abs(v) - a
        o = np.maximum(q, 0.0)
        out = _norm(o)
        onehot = np.eye(3)[np.argmax(q, axis=-1)]
        gb = _side(v) * np.where((out > 0)[..., None], o / np.where(out > 0, out, 1.0)[..., None], onehot)
        db = out + np.minimum(q.max(axis=-1), 0.0)
        # vertical cylinder: the same on (rho - r, |vz| - h); on the axis the radial direction is (1, 0, 0); inside the side wins a tie
        rho = np.hypot(v[..., 0], v[..., 1])
        u = np.where((rho > 0)[..., None], v[..., :2] / np.where(rho > 0, rho, 1.0)[..., None], np.array([1.0, 0.0]))
        qr, qz = rho - a[..., 0], np.abs(v[..., 2]) - a[..., 2]
        orr, oz = np.maximum(qr, 0.0), np.maximum(qz, 0.0)
        outc = np.hypot(orr, oz)
        safe = np.where(outc > 0, outc, 1.0)
        wr = np.where(outc > 0, orr / safe, np.where(qr >= qz, 1.0, 0.0))
        wz = np.where(outc > 0, oz / safe, np.where(qr >= qz, 0.0, 1.0))
        gc = np.concatenate([u * wr[..., None], (_side(v[..., 2]) * wz)[..., None]], axis=-1)
        dc = outc + np.minimum(np.maximum(qr, qz), 0.0)
    for k, dk, gk in ((SPHERE, ln - a[..., 0], gs), (BOX, db, gb), (CYLINDER, dc, gc),
                      (FLOOR, v[..., 2], np.broadcast_to(np.array([0.0, 0.0, 1.0]), (N, M, 3)))):
        d = np.where(kind == k, dk, d)
        g = np.where((kind == k)[..., None], gk, g)
    return d, g


def _slab(v, d, a, t0, t1):
    """[t0, t1] intersected with the t for which |v + t d| <= a; a parallel direction decides by the origin alone"""
    par = d == 0
    with np.errstate(all="ignore"):
        inv = 1.0 / np.where(par, 1.0, d)
        ta, tb = (-a - v) * inv, (a - v) * inv
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    return np.where(par, t0, np.maximum(t0, lo)), np.where(par, np.where(np.abs(v) > a, -np.inf, t1), np.minimum(t1, hi))


def ray(obst, p, dirs):
    """t [N, M, R]: the first t >= 0 at which p + t d is inside or on the obstacle (0 for an origin inside), +inf for a miss.
    dirs [N, R, 3] unit vectors."""
    obst, p, dirs = _lists(obst), np.asarray(p, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
    N, M, R = len(p), obst.shape[1], dirs.shape[1]
    v = (p[:, None, :] - obst[..., 0:3])[:, :, None, :]            # [N, M, 1, 3]
    d = dirs[:, None, :, :]                                         # [N, 1, R, 3]
    kind = np.broadcast_to(obst[..., 3], (N, M))[:, :, None]
    a = np.broadcast_to(obst[..., 4:7], (N, M, 3))[:, :, None, :]
    shape = (N, M, R)
    vx, vy, vz = (np.broadcast_to(v[..., i], shape) for i in range(3))
    dx, dy, dz = (np.broadcast_to(d[..., i], shape) for i in range(3))
    zero, inf = np.zeros(shape), np.full(shape, np.inf)
    with np.errstate(all="ignore"):
        # sphere: the smaller root of t^2 + 2 b t + c = 0
        r = a[..., 0]
        b, c = vx * dx + vy * dy + vz * dz, vx * vx + vy * vy + vz * vz - r * r
        disc = b * b - c
        ts = np.where(c <= 0, 0.0, np.where((b < 0) & (disc >= 0), c / (np.sqrt(np.maximum(disc, 0.0)) - b), np.inf))
        # box: three slabs
        t0, t1 = _slab(vx, dx, a[..., 0], zero, inf)
        t0, t1 = _slab(vy, dy, a[..., 1], t0, t1)
        t0, t1 = _slab(vz, dz, a[..., 2], t0, t1)
        tb = np.where(t0 <= t1, t0, np.inf)
        # vertical cylinder: the infinite cylinder's interval and the slab of the caps
        aa, bb, cc = dx * dx + dy * dy, vx * dx + vy * dy, vx * vx + vy * vy - r * r
        vert = aa == 0
        sa = np.where(vert, 1.0, aa)
        dc = bb * bb - sa * cc
        rt = np.sqrt(np.maximum(dc, 0.0))
        lo = np.where(vert, np.where(cc > 0, np.inf, 0.0), np.where(dc >= 0, np.maximum((-bb - rt) / sa, 0.0), np.inf))
        hi = np.where(vert, np.where(cc > 0, -np.inf, np.inf), np.where(dc >= 0, (-bb + rt) / sa, -np.inf))
        t0, t1 = _slab(vz, dz, a[..., 2], lo, hi)
        tc = np.where(t0 <= t1, t0, np.inf)
        # floor: the half-space z <= cz
        tf = np.where(vz <= 0, 0.0, np.where(dz < 0, vz / np.where(dz < 0, -dz, 1.0), np.inf))
    t = inf
    for k, tk in ((SPHERE, ts), (BOX, tb), (CYLINDER, tc), (FLOOR, tf)):
        t = np.where(kind == k, tk, t)
    return t


def _two_smallest(x, axis):
    """(smallest, its first index, second smallest) along `axis`"""
    x = np.moveaxis(x, axis, -1)
    first = np.argmin(x, axis=-1)
    best = np.take_along_axis(x, first[..., None], axis=-1)[..., 0]
    if x.shape[-1] == 1:
        return best, first, np.full(best.shape, np.inf)
    rest = x.copy()
    np.put_along_axis(rest, first[..., None], np.inf, axis=-1)
    return best, first, rest.min(axis=-1)


def clearance(obst, p, collision_radius=COLLISION_RADIUS):
    """dict: `d` [N], `normal` [N, 3], `nearest` [N] (ties to the lower record), `hit` [N], `second` [N] (the next distance).  Every
    record NONE, or a position that is not finite: (0, 0, 0, +inf), -1, no hit."""
    p = np.asarray(p, dtype=np.float64)
    fin = np.isfinite(p).all(axis=-1)
    d, g = sdf(obst, np.where(fin[:, None], p, 0.0))
    d = np.where(fin[:, None], d, np.inf)
    best, who, second = _two_smallest(d, 1)
    normal = np.take_along_axis(g, who[:, None, None], axis=1)[:, 0]
    some = np.isfinite(best)
    return dict(d=best, normal=np.where(some[:, None], normal, 0.0), nearest=np.where(some, who, -1), hit=best < collision_radius,
                second=second)


def scan(obst, p, dirs, max_range=MAX_RANGE):
    """dict: `ranges` [N, R] capped at max_range, `ray_hit` [N, R] (-1: nothing closer than max_range), `second` [N, R] (the next
    entry distance).  A pose that is not finite: max_range and -1."""
    p, dirs = np.asarray(p, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
    fin = np.isfinite(p).all(axis=-1) & np.isfinite(dirs).all(axis=(1, 2))
    t = ray(obst, np.where(fin[:, None], p, 0.0), np.where(fin[:, None, None], dirs, np.array([1.0, 0.0, 0.0])))
    t = np.where(fin[:, None, None], t, np.inf)
    best, who, second = _two_smallest(t, 1)
    seen = best < max_range
    return dict(ranges=np.where(seen, best, max_range), ray_hit=np.where(seen, who, -1), second=second, entry=best)


def quat_to_mat(q):
    """btMatrix3x3::setRotation: the rotation of q = (x, y, z, w), whatever |q|"""
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = (q[..., i] for i in range(4))
    s = 2.0 / (q * q).sum(axis=-1)
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - s * (y * y + z * z); R[..., 0, 1] = s * (x * y - w * z); R[..., 0, 2] = s * (x * z + w * y)
    R[..., 1, 0] = s * (x * y + w * z); R[..., 1, 1] = 1 - s * (x * x + z * z); R[..., 1, 2] = s * (y * z - w * x)
    R[..., 2, 0] = s * (x * z - w * y); R[..., 2, 1] = s * (y * z + w * x); R[..., 2, 2] = 1 - s * (x * x + y * y)
    return R


def yaw_of(q):
    """yaw of pybullet's getEulerFromQuaternion (its gimbal branches included) of the NORMALISED quaternion"""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(axis=-1, keepdims=True))
    x, y, z, w = (q[..., i] for i in range(4))
    sarg = -2.0 * (x * z - w * y)
    regular = np.arctan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z)
    return np.where(sarg <= -0.99999, 2.0 * np.arctan2(x, -y), np.where(sarg >= 0.99999, 2.0 * np.arctan2(-x, y), regular))


def rotate(dirs, quat, frame):
    """dirs [R, 3] in the frame of every drone -> world directions [N, R, 3]: 0 world, 1 levelled (about z by the yaw), 2 body"""
    dirs, quat = np.asarray(dirs, dtype=np.float64), np.asarray(quat, dtype=np.float64)
    if frame == 0:
        return np.broadcast_to(dirs, (len(quat),) + dirs.shape).copy()
    with np.errstate(all="ignore"):
        if frame == 2:
            return np.einsum("nij,rj->nri", quat_to_mat(quat), dirs)
        yaw = yaw_of(quat)
        c, s = np.cos(yaw)[:, None], np.sin(yaw)[:, None]
        return np.stack([c * dirs[None, :, 0] - s * dirs[None, :, 1], s * dirs[None, :, 0] + c * dirs[None, :, 1],
                         np.broadcast_to(dirs[None, :, 2], c.shape[:1] + dirs.shape[:1])], axis=-1)


def grown(obst, delta):
    """every obstacle grown by `delta` (shrunk for a negative one): radii, half extents, half heights, the floor's level"""
    o = np.array(obst, dtype=np.float64)
    kind = o[..., 3]
    o[..., 4:7] = np.where(np.isin(kind, (SPHERE, BOX, CYLINDER))[..., None], np.maximum(o[..., 4:7] + delta, 0.0), o[..., 4:7])
    o[..., 2] = np.where(kind == FLOOR, o[..., 2] + delta, o[..., 2])
    return o


def grazing(obst, p, dirs, max_range=MAX_RANGE):
    """[N, R] bool: rays whose answer moves by more than 1e-3 m when every obstacle is grown or shrunk by 1e-4 m"""
    base = scan(obst, p, dirs, max_range)["ranges"]
    return np.maximum(np.abs(scan(grown(obst, GRAZE_GROW), p, dirs, max_range)["ranges"] - base),
                      np.abs(scan(grown(obst, -GRAZE_GROW), p, dirs, max_range)["ranges"] - base)) > GRAZE_MOVE


def rel_err(x32, x64):
    x32, x64 = np.asarray(x32, dtype=np.float64), np.asarray(x64, dtype=np.float64)
    same_inf = np.isinf(x64) & (x32 == x64)
    with np.errstate(invalid="ignore"):
        e = np.abs(x32 - x64) / np.maximum(1.0, np.abs(x64))
    return np.where(same_inf, 0.0, e)


def compare_clearance(got, obst, p, collision_radius=COLLISION_RADIUS):
    """`got`: dict with any of `clear4` [N, 4], `nearest` [N], `hit` [N] from a float32 implementation.  Asserts the identities that
    have no tolerance under the exclusion rules (and the caps on what they leave out); returns the largest error of d and of the
    normal's components."""
    want = clearance(obst, p, collision_radius)
    n = len(want["d"])
    some = np.isfinite(want["d"])
    with np.errstate(invalid="ignore"):                     # (inf - inf of a drone without any obstacle: no tie)
        near_tie = some & (want["second"] - want["d"] < NEAR_TIE)
    on_edge = some & (np.abs(want["d"] - collision_radius) < ON_THRESHOLD)
    assert near_tie.sum() <= CAP_DRONES * n and on_edge.sum() <= CAP_DRONES * n, (int(near_tie.sum()), int(on_edge.sum()), n)
    err_d = err_n = 0.0
    if got.get("nearest") is not None:
        np.testing.assert_array_equal(np.asarray(got["nearest"])[~near_tie], want["nearest"][~near_tie])
    if got.get("hit") is not None:
        np.testing.assert_array_equal(np.asarray(got["hit"]).astype(bool)[~on_edge], want["hit"][~on_edge])
    if got.get("clear4") is not None:
        c = np.asarray(got["clear4"], dtype=np.float64)
        err_d = float(rel_err(c[:, 3], want["d"]).max())
        # (at a near tie the two candidates' gradients differ, whichever is right)
        keep = ~near_tie
        err_n = float(rel_err(c[keep, :3], want["normal"][keep]).max()) if keep.any() else 0.0
    return err_d, err_n


def compare_scan(got, obst, p, dirs, max_range=MAX_RANGE):
    """`got`: dict with `ranges` [N, R] and optionally `ray_hit`.  Grazing rays are left out (at most 2 % of them), near ties of the
    record too; returns the largest error of the ranges."""
    want = scan(obst, p, dirs, max_range)
    graze = grazing(obst, p, dirs, max_range)
    assert graze.mean() <= CAP_RAYS, float(graze.mean())
    keep = ~graze
    err = float(rel_err(np.asarray(got["ranges"])[keep], want["ranges"][keep]).max()) if keep.any() else 0.0
    if got.get("ray_hit") is not None:
        with np.errstate(invalid="ignore"):                 # (inf - inf of a ray that enters nothing: no tie)
            tie = want["second"] - want["entry"] < NEAR_TIE
        tie_drones = (tie & keep).any(axis=1)
        assert tie_drones.sum() <= CAP_DRONES * len(tie_drones), int(tie_drones.sum())
        ok = keep & ~tie
        np.testing.assert_array_equal(np.asarray(got["ray_hit"])[ok], want["ray_hit"][ok])
    return err


def scene(seed=0, n_drones=210, n_rays=16):
    """The test scene: 8 spheres, 8 boxes, 8 cylinders (drawn kind by kind, centres first, then sizes) and a floor at z = 0;
    `(obst [25, 8], pos [n, 3], dirs [n, R, 3])`"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-4.0, -4.0, 0.3]), np.array([4.0, 4.0, 2.7])
    rows = []
    c = rng.uniform(lo, hi, size=(8, 3))
    r = rng.uniform(0.2, 0.6, size=8)
    rows += [record(SPHERE, c[i], (r[i], 0, 0)) for i in range(8)]
    c = rng.uniform(lo, hi, size=(8, 3))
    h = rng.uniform(0.15, 0.6, size=(8, 3))
    rows += [record(BOX, c[i], h[i]) for i in range(8)]
    c = rng.uniform(lo, hi, size=(8, 3))
    r = rng.uniform(0.15, 0.4, size=8)
    hh = rng.uniform(0.5, 1.5, size=8)
    rows += [record(CYLINDER, c[i], (r[i], 0, hh[i])) for i in range(8)]
    rows.append(record(FLOOR))
    pos = rng.uniform([-4.0, -4.0, 0.05], [4.0, 4.0, 3.0], size=(n_drones, 3))
    dirs = rng.normal(size=(n_drones, n_rays, 3))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    return np.array(rows), pos, dirs

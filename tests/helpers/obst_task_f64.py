"""The obstacle task (include/gpd.h gpd_rollout_obst), what its tests share: the float64 restatement of csrc/obst_task_math.inc, the
table of device cases with the scene each one flies, and the bound of the host comparison.  No GPU needed: the scenes are numpy."""
import collections
import math

import numpy as np

NONE, SPHERE, BOX, CYLINDER, FLOOR = -1, 0, 1, 2, 3
GND, DRAG, DW, GROUND, DAMP = 1, 2, 4, 8, 16
EVERY = GND | DRAG | GROUND | DAMP
COLLISION_RADIUS = 0.06
ULP32 = 2.0 ** -23


# ---- csrc/obst_task_math.inc in float64 ---------------------------------------------------------------------------------------------------
def hit(d, r):
    return np.asarray(d, dtype=np.float64) < r


def reward(task_reward, d, r, hit_reward, prox_margin, prox_weight):
    """task_reward + hit_reward * hit - prox_weight * max(0, prox_margin - (d - r)); the hinge is 0 for d = +inf"""
    d = np.asarray(d, dtype=np.float64)
    hinge = np.maximum(0.0, prox_margin - (d - r))
    return np.asarray(task_reward, dtype=np.float64) + hit_reward * hit(d, r) - prox_weight * hinge


def bound(task_reward, d, r, hit_reward, prox_margin, prox_weight):
    """4 ulp (fp32) of |task_reward| + |hit_reward| + prox_weight (prox_margin + |d - r|): the formula is a handful of roundings of
    terms of that size and nothing else (five at most, half an ulp each)"""
    gap = np.where(np.isfinite(d), np.abs(np.asarray(d, dtype=np.float64) - r), 0.0)
    return 4.0 * ULP32 * (np.abs(task_reward) + abs(hit_reward) + prox_weight * (prox_margin + gap))


def math_inputs(seed=0, count=4096):
    """[count, 6] float32 rows task_reward, d, r, hit_reward, prox_margin, prox_weight: inside and outside the margin, in contact,
    exactly at contact, and d = +inf"""
    rng = np.random.default_rng(seed)
    x = np.empty((count, 6), dtype=np.float32)
    x[:, 0] = np.where(rng.random(count) < 0.3, -1.0, rng.uniform(0.0, 2.0, count))
    x[:, 2] = rng.uniform(0.02, 0.2, count)
    x[:, 1] = x[:, 2] + rng.uniform(-0.3, 1.0, count).astype(np.float32)
    x[:, 3] = rng.uniform(-20.0, 5.0, count)
    x[:, 4] = rng.uniform(0.0, 0.8, count)
    x[:, 5] = rng.uniform(0.0, 10.0, count)
    x[::17, 1] = np.inf
    x[5::29, 1] = x[5::29, 2]                 # d == r: no contact (strict)
    x[3::31, 5] = 0.0
    x[7::37, 4] = 0.0
    return x


# ---- the device cases ---------------------------------------------------------------------------------------------------------------------
#: obst: ("shared", M) one list of M records with NONE records between the live ones, or ("lists", M) field planes per aviary with a
#: pitch above E and NaN beyond E
Case = collections.namedtuple("Case", "name N K S act flags rays frame obst task auto_reset")
CASES = (
    Case("vel_shared7_r16_body", 257, 5, 5, "vel", 0, 16, "body", ("shared", 7), "hover", 1),
    Case("rpm_shared1_r0", 257, 5, 1, "rpm", 0, 0, "world", ("shared", 1), "none", 0),
    Case("pid_lists_r5_level", 70, 5, 5, "pid", EVERY, 5, "level", ("lists", 5), "hover", 1),
    Case("vel_shared65_r64_world", 70, 1, 1, "vel", EVERY, 64, "world", ("shared", 65), "hover", 1),
    Case("rpm_lists_r1_body", 1, 5, 5, "rpm", EVERY, 1, "body", ("lists", 5), "none", 0),
    Case("vel_lists_r16_level", 257, 1, 5, "vel", 0, 16, "level", ("lists", 5), "none", 0),
    Case("pid_shared7_r5_body", 257, 5, 1, "pid", 0, 5, "body", ("shared", 7), "hover", 1),
    Case("rpm_shared65_r16_world", 257, 5, 5, "rpm", EVERY, 16, "world", ("shared", 65), "hover", 1),
    Case("vel_lists_r64_body", 70, 5, 5, "vel", EVERY, 64, "body", ("lists", 5), "none", 0),
)
ACT_CODE = {"rpm": 0, "pid": 1, "vel": 2}
ACT_DIM = {"rpm": 4, "pid": 3, "vel": 4}
FRAMES = {"world": 0, "level": 1, "body": 2}
#: the task every case flies: contact ends the episode and costs 5, the hinge reaches 0.5 m beyond contact
HIT_REWARD, PROX_MARGIN, PROX_WEIGHT, MAX_RANGE = -5.0, 0.5, 2.0, 2.5
PYB_FREQ = 240
HITTERS = 0.35          # the share of drones that start on a collision course


def group_lanes(n_rays):
    g = 1
    while g < max(1, n_rays):
        g *= 2
    return g


def record(kind, centre=(0.0, 0.0, 0.0), size=(0.0, 0.0, 0.0)):
    return [centre[0], centre[1], centre[2], float(kind), size[0], size[1], size[2], 0.0]


def _records(rng, M, jitter):
    """[M, 8]: live records at every other slot (all of them for M = 1), NONE between; the live ones on a 0.5 m grid at z = 1, kinds
    cycling sphere / box / cylinder, and from five records on a floor 0.4 m below them (what the rays that look down see)"""
    rec = np.array([record(NONE)] * M, dtype=np.float64)
    live = list(range(0, M, 2))
    side = max(1, math.ceil(math.sqrt(len(live))))
    cells = [(i, j) for i in range(side) for j in range(side)]
    for n, m in enumerate(live):
        i, j = cells[n]
        c = ((i - 0.5 * (side - 1)) * 0.5 + jitter[0], (j - 0.5 * (side - 1)) * 0.5 + jitter[1], 1.0)
        kind = (SPHERE, BOX, CYLINDER)[(n + int(jitter[2])) % 3]
        s = rng.uniform(0.04, 0.06, 3)
        size = (s[0], 0.0, 0.0) if kind == SPHERE else (s[0], s[1], 0.12) if kind == BOX else (s[0], 0.0, 0.12)
        rec[m] = record(kind, c, size)
    if M >= 5:
        rec[live[-1]] = record(FLOOR, (0.0, 0.0, 0.6))
        live = live[:-1]
    return rec, live


def _approach(rng, r):
    """a horizontal unit direction n pointing away from record r's surface, and the point of the surface it leaves from"""
    kind, c, a = int(r[3]), r[0:3], r[4:7]
    if kind == BOX:
        axis, sign = int(rng.integers(0, 2)), float(rng.choice((-1.0, 1.0)))
        n = np.zeros(3)
        n[axis] = sign
        on = c + n * a[axis]
        on[1 - axis] += rng.uniform(-0.5, 0.5) * a[1 - axis]
        on[2] += rng.uniform(-0.5, 0.5) * a[2]
        return n, on
    th = rng.uniform(0.0, 2.0 * math.pi)
    n = np.array([math.cos(th), math.sin(th), 0.0])
    on = c + n * a[0]
    if kind == CYLINDER:
        on[2] += rng.uniform(-0.5, 0.5) * a[2]
    return n, on


Scene = collections.namedtuple("Scene", "records table obst_ld n_obst kin pid last_rpm init_xyz init_rpy actions rays hitter gap travel")


def rpy_to_quat(rpy):
    r, p, y = rpy[..., 0] / 2, rpy[..., 1] / 2, rpy[..., 2] / 2
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


def scene(case, seed=0, far=False):
    """The inputs of a case.  About HITTERS of the drones start with a gap to contact of 10-60 % of what their start speed covers in
    K - 1 steps (one step for K = 1), flying straight at their nearest surface; the others start 0.05-0.12 m beyond that reach (inside
    the proximity margin) and fly along the surface or away.  Tilted, turning, with controller members that are not zero.  The reset
    pose of aviary 0 lies inside its nearest obstacle.  `far`: every record moved 50 m away (nothing is ever near)."""
    rng = np.random.default_rng(seed + 1000 * CASES.index(case))
    N, K, S = case.N, case.K, case.S
    mode, M = case.obst
    dt = S / PYB_FREQ
    shared, live = _records(rng, M, (0.0, 0.0, 0))
    recs = np.empty((N, M, 8))
    for e in range(N):
        recs[e] = shared if mode == "shared" else _records(rng, M, (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), e))[0]
    hitter = rng.random(N) < HITTERS
    hitter[0] = True
    pos, vel, gap, travel = np.empty((N, 3)), np.empty((N, 3)), np.empty(N), np.empty(N)
    init_xyz = np.empty((N, 3))
    for e in range(N):
        r = recs[e, live[int(rng.integers(0, len(live)))]]
        n, on = _approach(rng, r)
        speed = rng.uniform(0.6, 1.4)
        travel[e] = speed * dt * max(1, K - 1)
        if hitter[e]:
            gap[e] = rng.uniform(0.1, 0.6) * travel[e]
            vel[e] = -speed * n
        else:
            gap[e] = travel[e] + rng.uniform(0.05, 0.12)
            t = np.array([-n[1], n[0], 0.0])
            vel[e] = speed * (t * rng.choice((-1.0, 1.0)) + 0.3 * n) / math.sqrt(1.09)
        pos[e] = on + n * (COLLISION_RADIUS + gap[e])
        init_xyz[e] = on + np.array([0.0, 0.0, 0.5 + rng.uniform(0.0, 0.1)])      # a free pose above the course, at rest
    init_xyz[0] = recs[0, live[0], 0:3] + np.array([0.01, 0.0, 0.0])    # ... and one inside an obstacle
    if far:
        recs[..., 0] += 50.0
        recs[..., 2] = np.where(recs[..., 3] == FLOOR, -50.0, recs[..., 2])
    rpy = rng.uniform(-0.15, 0.15, (N, 3))
    kin = np.concatenate([pos, rpy_to_quat(rpy), vel, rng.uniform(-0.5, 0.5, (N, 3))], axis=1).T.astype(np.float32)      # [13, N]
    pid = np.concatenate([rng.uniform(-0.05, 0.05, (N, 3)), rpy + rng.uniform(-0.01, 0.01, (N, 3)), rng.uniform(-0.05, 0.05, (N, 3))], axis=1).T
    last_rpm = rng.uniform(14000.0, 15000.0, (4, N)).astype(np.float32)
    init_rpy = np.zeros((N, 3))
    init_rpy[:, 2] = rng.uniform(-1.0, 1.0, N)
    vdir = vel / np.linalg.norm(vel, axis=1, keepdims=True)
    if case.act == "rpm":
        actions = rng.uniform(-0.2, 0.2, (K, N, 4))
    elif case.act == "vel":
        actions = np.concatenate([vdir[None] + rng.uniform(-0.1, 0.1, (K, N, 3)), rng.uniform(0.5, 1.0, (K, N, 1))], axis=2)
    else:
        actions = (pos + 0.5 * vdir)[None] + rng.uniform(-0.02, 0.02, (K, N, 3))
    rays = None
    if case.rays:
        az = np.arange(case.rays) * (2.0 * math.pi / case.rays) + 0.1
        el = 0.6 * np.sin(3.0 * az)
        rays = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
        rays = (rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32)
    if mode == "shared":
        table, ld = recs[0].astype(np.float32), 1
    else:
        ld = N + 3                                                       # a pitch above E, NaN beyond E
        table = np.full((M * 8, ld), np.nan, dtype=np.float32)
        table[:, :N] = recs.transpose(1, 2, 0).reshape(M * 8, N)
    return Scene(recs, table, ld, M, kin, pid.astype(np.float32), last_rpm, init_xyz, init_rpy, actions.astype(np.float32), rays, hitter, gap, travel)

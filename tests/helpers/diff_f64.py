"""The yardstick of the differentiable rollout (tests/test_host_diff.py, tests/test_gpu_diff.py): a torch restatement of one env step
for the subset `gpd_rollout_tape` / `gpd_rollout_vjp` support -- single-drone aviaries, the four RPM action types, no add-on physics or
drag, no task or the hover task, per-drone constants (the plant path).  It is dtype-generic; run in float64 under autograd it is the
reference the device gradients are held against, and its forward is held against `oracle.batched_oracle` (1e-12).

Selects are written so that the branch NOT taken cannot produce NaN gradients (`torch.where` multiplies the untaken branch's gradient
by zero, and 0 * inf = NaN): every operand of an untaken branch is replaced by a harmless one first.  A plain sin(t) / |w| is NaN at rest.

`stats` (a dict) records the extremes a run met at each select -- the gimbal test, the no-turn test, the tumbling test, the reward clamp --
and, under "lanes", the same per drone (`_lanes`): which lanes sat on which side, at every step and sub-step.

The same file holds the input generators of the GPU tests: `make_inputs` (near hover, far from every threshold) and `make_edge_inputs`
(part of the lanes on the far side of a select, with margin).  Test infrastructure."""
import math
from types import SimpleNamespace

import numpy as np
import torch

ACT_DIM = {"rpm": 4, "one_d_rpm": 1, "raw_rpm": 4, "direct_rpm": 4}
ACT_CODE = {"rpm": 0, "one_d_rpm": 3, "raw_rpm": 5, "direct_rpm": 6}
GIMBAL = 0.99999
TURN_N2 = 1e-16
#: the airframes of `config`, by their member of utils.enums.DroneModel
MODELS = {"cf2x": "CF2X", "cf2p": "CF2P", "racer": "RACE"}
#: order of the plant scale factors (include/gpd.h GPD_SCALE_*)
SCALES = ("mass", "ixx", "iyy", "izz", "kf", "km", "drag_xy", "drag_z", "gnd_eff")


def config(model="cf2x", act="rpm", S=1, drag=False, task="hover", pyb_freq=240):
    """what one env step depends on besides the constants: airframe ("cf2x" | "cf2p" | "racer"), action type, sub-steps per step,
    the drag term, the task ("none" | "hover")"""
    return SimpleNamespace(model=model, act=act, S=int(S), drag=bool(drag), task=task, h=1.0 / pyb_freq)


def consts(C, n, dtype=torch.float64, device="cpu", scales=None):
    """Per-drone constants [n] from an object with the reference's attribute names (M, L, KF, KM, J, DRAG_COEFF, GRAVITY, HOVER_RPM,
    MAX_RPM: `DroneParams` or the oracle's `UrdfConstants`); `scales` [9, n]: the plant path's scale factors (the action mapping's
    HOVER_RPM and the MAX_RPM clip stay nominal, include/gpd.h), numpy or torch -- a tensor may be an autograd leaf: the products are
    formed in torch float64, inside the graph, and each is cast to `dtype`."""
    s = torch.ones((9, n), dtype=torch.float64) if scales is None else torch.as_tensor(scales, dtype=torch.float64)
    J = np.diag(np.asarray(C.J, dtype=np.float64))
    drag = np.asarray(C.DRAG_COEFF, dtype=np.float64)
    t = lambda v: (v if isinstance(v, torch.Tensor) else torch.full((n,), float(v), dtype=torch.float64)).to(dtype=dtype, device=device)   # noqa: E731
    return SimpleNamespace(
        M=t(float(C.M) * s[0]), GRAVITY=t(float(C.G * C.M) * s[0]), L=t(C.L), KF=t(float(C.KF) * s[4]), KM=t(float(C.KM) * s[5]),
        J=torch.stack([t(float(J[0]) * s[1]), t(float(J[1]) * s[2]), t(float(J[2]) * s[3])], dim=1),
        DRAG=torch.stack([t(float(drag[0]) * s[6]), t(float(drag[1]) * s[6]), t(float(drag[2]) * s[7])], dim=1),
        HOVER_RPM=t(C.HOVER_RPM), MAX_RPM=t(C.MAX_RPM))


def rpm_from_action(c, cfg, a):
    """[n, A] -> [n, 4] (envs/BaseRLAviary.py:187-239, envs/CtrlAviary.py:140); the clip has zero gradient outside its bounds"""
    if cfg.act == "rpm":
        return c.HOVER_RPM[:, None] * (1 + 0.05 * a)
    if cfg.act == "one_d_rpm":
        return (c.HOVER_RPM[:, None] * (1 + 0.05 * a)).expand(-1, 4)
    if cfg.act == "raw_rpm":
        return torch.minimum(torch.maximum(a, torch.zeros_like(a)), c.MAX_RPM[:, None].expand_as(a))
    return a


def _lanes(stats, key, value):
    """per-lane record of a run: stats["lanes"][key] = (min, max) over every evaluation, each a float64 array [n] -- what the scalar
    minima and maxima of `stats` cannot tell: how many lanes sat on which side of a select, and for how long"""
    v = value.detach().to(torch.float64).numpy()
    lanes = stats.setdefault("lanes", {})
    lo, hi = lanes.get(key, (v, v))
    lanes[key] = (np.minimum(lo, v), np.maximum(hi, v))


def rotation(q):
    """btMatrix3x3::setRotation: columns-of-rows list R[i][j], each [n]"""
    x, y, z, w = q.unbind(-1)
    s = 2.0 / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    return [[1.0 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1.0 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1.0 - (xx + yy)]]


def euler(q, stats=None):
    """pybullet_getEulerFromQuaternion with its gimbal branches, NaN-safe selects"""
    x, y, z, w = q.unbind(-1)
    sarg = -2.0 * (x * z - w * y)
    lo, hi = sarg <= -GIMBAL, sarg >= GIMBAL
    gim = lo | hi
    if stats is not None:
        stats["sarg_max"] = max(stats.get("sarg_max", 0.0), float(sarg.detach().abs().max()))
        _lanes(stats, "sarg_abs", sarg.abs())
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    # regular branch on safe operands where the gimbal branch is taken ...
    rb = torch.where(gim, one, w * w - x * x - y * y + z * z)
    yb = torch.where(gim, one, w * w + x * x - y * y - z * z)
    roll = torch.where(gim, zero, torch.atan2(2.0 * (y * z + w * x), rb))
    pitch = torch.asin(torch.where(gim, zero, sarg))
    yaw = torch.atan2(2.0 * (x * y + w * z), yb)
    # ... and the gimbal branch on safe operands where it is not
    gy = torch.where(gim, y, one)
    yaw_g = torch.where(lo, 2.0 * torch.atan2(x, -gy), 2.0 * torch.atan2(-x, gy))
    pitch = torch.where(lo, torch.full_like(x, -0.5 * math.pi), torch.where(hi, torch.full_like(x, 0.5 * math.pi), pitch))
    return torch.stack([roll, pitch, torch.where(gim, yaw_g, yaw)], dim=-1)


def substep(c, cfg, kin, rpm, drag_sum, stats=None):
    """envs/BaseAviary.py:831-892 for the supported terms; returns the new (pos, quat, vel, rates) and the observed world ang_v"""
    pos, quat, vel, w = kin
    h = cfg.h
    R = rotation(quat)
    f = c.KF[:, None] * rpm ** 2
    fz = f.sum(-1)
    F = torch.stack([R[0][2] * fz, R[1][2] * fz, R[2][2] * fz - c.GRAVITY], dim=-1)
    if cfg.drag:
        F = F - c.DRAG * vel * (drag_sum * (2 * math.pi / 60))[:, None]
    yaw_t = c.KM[:, None] * rpm ** 2 * (-1.0 if cfg.model == "racer" else 1.0)
    tz = -yaw_t[:, 0] + yaw_t[:, 1] - yaw_t[:, 2] + yaw_t[:, 3]
    if cfg.model == "cf2p":
        tx, ty = (f[:, 1] - f[:, 3]) * c.L, (-f[:, 0] + f[:, 2]) * c.L
    else:
        arm = c.L / math.sqrt(2)
        tx = (f[:, 0] + f[:, 1] - f[:, 2] - f[:, 3]) * arm
        ty = (-f[:, 0] + f[:, 1] + f[:, 2] - f[:, 3]) * arm
        if cfg.model == "cf2x":
            tx = -tx
    Jw = c.J * w
    tau = torch.stack([tx, ty, tz], dim=-1) - torch.cross(w, Jw, dim=-1)
    w = w + h * (tau / c.J)
    vel = vel + h * (F / c.M[:, None])
    pos = pos + h * vel
    n2 = (w * w).sum(-1)
    turn = n2 > TURN_N2                                            # !np.isclose(|w|, 0)
    if stats is not None:
        stats["n2_min"] = min(stats.get("n2_min", math.inf), float(n2.detach().min()))
        stats["u_max"] = max(stats.get("u_max", 0.0), float(n2.detach().max()) * (0.25 * h * h))
        _lanes(stats, "n2", n2)
        _lanes(stats, "u", n2 * (0.25 * h * h))                       # (the half-angle squared: the kernels' tumbling test is u > 1)
    n = torch.sqrt(torch.where(turn, n2, torch.ones_like(n2)))     # (safe: sqrt and the division never see 0)
    th = n * h / 2
    qx, qy, qz, qw = quat.unbind(-1)
    p, q_, r = w.unbind(-1)
    lam = torch.stack([r * qy - q_ * qz + p * qw, -r * qx + p * qz + q_ * qw, q_ * qx - p * qy + r * qw, -p * qx - q_ * qy - r * qz], dim=-1)
    qn = torch.cos(th)[:, None] * quat + (torch.sin(th) / n)[:, None] * lam
    quat_new = torch.where(turn[:, None], qn, quat)
    ang_v = torch.stack([R[i][0] * p + R[i][1] * q_ + R[i][2] * r for i in range(3)], dim=-1)    # PRE-update rotation, post-update rates
    return (pos, quat_new, vel, w), ang_v


def step(c, cfg, kin, act, prev_sum, target=None, stats=None):
    """one env step: -> kin', obs12 [n, 12], reward [n], this step's rpm sum (the next step's first drag term sees it)"""
    rpm = rpm_from_action(c, cfg, act)
    cur_sum = rpm.sum(-1)
    ang_v = None
    for s in range(cfg.S):
        kin, ang_v = substep(c, cfg, kin, rpm, prev_sum if s == 0 else cur_sum, stats)
    pos, quat, vel, _ = kin
    obs = torch.cat([pos, euler(quat, stats), vel, ang_v], dim=-1)
    if cfg.task == "hover":
        d2 = ((target - pos) ** 2).sum(-1)
        arg = 2.0 - d2 * d2
        if stats is not None:
            stats["reward_arg_min"] = min(stats.get("reward_arg_min", math.inf), float(arg.detach().min()))
            _lanes(stats, "reward_arg", arg)
        reward = torch.where(arg > 0, arg, torch.zeros_like(arg))
    else:
        reward = -torch.ones_like(pos[:, 0])
    return kin, obs, reward, cur_sum


def rollout(c, cfg, kin0, actions, first_sum, target=None, stats=None):
    """K steps: actions [K, n, A] -> obs12 [K, n, 12], reward [K, n], kin_K.  `first_sum` [n]: the rpm sum carried in from before the
    call (a constant)."""
    kin, prev, obs, rew = kin0, first_sum, [], []
    for t in range(actions.shape[0]):
        kin, o, r, prev = step(c, cfg, kin, actions[t], prev, target, stats)
        obs.append(o)
        rew.append(r)
    return torch.stack(obs), torch.stack(rew), kin


def quat_from_rpy(rpy):
    """btQuaternion::setEulerZYX + normalize, numpy float64 [n, 3] -> [n, 4] xyzw"""
    h = 0.5 * np.asarray(rpy, dtype=np.float64)
    cr, sr, cp, sp, cy, sy = np.cos(h[:, 0]), np.sin(h[:, 0]), np.cos(h[:, 1]), np.sin(h[:, 1]), np.cos(h[:, 2]), np.sin(h[:, 2])
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def make_inputs(C, cfg, n, K, seed=0, at_rest=False, outside_clip=True):
    """The GPU tests' inputs, every value representable in float32 (both precisions start from the same numbers): positions within
    +-0.15 m of (0, 0, 1), small random attitudes (+-0.2 rad), velocities +-0.25 m/s, body rates +-1 rad/s (`at_rest`: exactly zero,
    level), actions U(-1, 1) (the raw action types: RPMs around hover, and -- RAW_RPM with `outside_clip` -- a third of them outside
    [0, MAX_RPM]), the rpm sum carried in, and random cotangents for every output.  numpy float64 arrays."""
    rng = np.random.default_rng(seed)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)     # noqa: E731
    A = ACT_DIM[cfg.act]
    pos = f32(np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.15, 0.15, (n, 3)))
    quat = f32(quat_from_rpy(rng.uniform(-0.2, 0.2, (n, 3))))
    vel = f32(rng.uniform(-0.25, 0.25, (n, 3)))
    rates = f32(rng.uniform(-1.0, 1.0, (n, 3)))
    if at_rest:
        quat = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))
        rates = np.zeros((n, 3))
    u = rng.uniform(-1.0, 1.0, (K, n, A))
    if cfg.act in ("raw_rpm", "direct_rpm"):
        u = C.HOVER_RPM * (1 + 0.05 * u)
        if cfg.act == "raw_rpm" and outside_clip:
            pick = rng.uniform(size=u.shape)
            u = np.where(pick < 1 / 6, -0.1 * u, np.where(pick < 1 / 3, C.MAX_RPM + 0.1 * u, u))
    last_rpm = f32(C.HOVER_RPM * (1 + 0.05 * rng.uniform(-1, 1, (n, 4))))
    return SimpleNamespace(n=n, K=K, A=A, pos=pos, quat=quat, vel=vel, rates=rates, actions=f32(u), last_rpm=last_rpm,
                           first_sum=f32(((last_rpm[:, 0] + last_rpm[:, 1]) + last_rpm[:, 2]) + last_rpm[:, 3]),
                           target=np.tile(np.array([0.0, 0.0, 1.0]), (n, 1)),
                           g_obs=f32(rng.standard_normal((K, n, 12))), g_rew=f32(rng.standard_normal((K, n))),
                           g_pos=f32(rng.standard_normal((n, 3))), g_quat=f32(rng.standard_normal((n, 4))),
                           g_vel=f32(rng.standard_normal((n, 3))), g_rates=f32(rng.standard_normal((n, 3))))


GROUPS = ("actions", "pos", "quat", "vel", "rates")


def reference_grads(C, cfg, inp, dtype=torch.float64, scales=None, shared_action=False, stats=None, g_obs=True, wrt_scales=False):
    """Gradients of sum(cotangent * output) over every output with respect to the actions and the four groups of the initial state,
    by torch autograd over the restatement: dict of numpy float64 arrays (GROUPS).  `shared_action`: actions[0] at every step.
    `wrt_scales`: the scales are a leaf too, and "scales" [9, n] (rows in SCALES order) their gradient; a scale the configuration
    does not read gets zeros."""
    T = lambda v: torch.as_tensor(v, dtype=dtype)     # noqa: E731
    leaf = lambda v: T(v).clone().requires_grad_(True)     # noqa: E731
    kin0 = tuple(leaf(v) for v in (inp.pos, inp.quat, inp.vel, inp.rates))
    a = leaf(inp.actions[0:1] if shared_action else inp.actions)
    leaves, names = (a,) + kin0, GROUPS
    if wrt_scales:
        scales = torch.as_tensor(scales, dtype=torch.float64).clone().requires_grad_(True)
        leaves, names = leaves + (scales,), GROUPS + ("scales",)
    c = consts(C, inp.n, dtype, scales=scales)
    acts = a.expand(inp.K, -1, -1) if shared_action else a
    obs, rew, kin_k = rollout(c, cfg, kin0, acts, T(inp.first_sum), T(inp.target), stats)
    loss = (T(inp.g_rew) * rew).sum() + sum((T(g) * k).sum() for g, k in zip((inp.g_pos, inp.g_quat, inp.g_vel, inp.g_rates), kin_k))
    if g_obs:
        loss = loss + (T(inp.g_obs) * obs).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    out = {k: (torch.zeros_like(x) if g is None else g).detach().to(torch.float64).numpy() for k, g, x in zip(names, grads, leaves)}
    out["forward"] = (obs.detach(), rew.detach(), tuple(k.detach() for k in kin_k))
    return out


def group_errors(got, want):
    """max |g - g64| / max |g64| per group (the metric of the tests)"""
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max() / max(float(np.abs(want[k]).max()), 1e-300)) for k in GROUPS}


def forward_error(obs, obs64):
    """the forward obs12 [K, n, 12] against the float64 run, relative to each column's scale: the largest over the columns of
    max |obs - obs64| / max(1, max |obs64|) (absolute for columns of order one; the angular velocity of a tumbling drone is not)"""
    obs, obs64 = np.asarray(obs, dtype=np.float64), np.asarray(obs64, dtype=np.float64)
    return float((np.abs(obs - obs64).max(axis=(0, 1)) / np.maximum(1.0, np.abs(obs64).max(axis=(0, 1)))).max())


#: the gradient cases of tests/test_gpu_diff.py (and of the host tests that vouch for the reference on the same inputs): 70 drones
#: (ld = 128: two waves, one ragged), task hover.  `scales`: plant scale factors drawn within +-20 %.
GPU_CASES = {
    "rpm_k32_s1": dict(model="cf2x", act="rpm", S=1, drag=False, K=32),
    "rpm_k8_s8": dict(model="cf2x", act="rpm", S=8, drag=False, K=8),
    "drag_k16_s8": dict(model="cf2x", act="rpm", S=8, drag=True, K=16),
    "one_d_k5_s2": dict(model="cf2x", act="one_d_rpm", S=2, drag=False, K=5),
    "raw_k3_clipped": dict(model="cf2x", act="raw_rpm", S=1, drag=False, K=3),
    "cf2p_drag_k8_s2": dict(model="cf2p", act="rpm", S=2, drag=True, K=8),
    "racer_k8_s1": dict(model="racer", act="rpm", S=1, drag=False, K=8),
    "plant_drag_k8_s2": dict(model="cf2x", act="rpm", S=2, drag=True, K=8, scales=True),
}


def case(name, n=70, seed=1):
    """(cfg, K, scales [9, n] or None) of a GPU case"""
    d = dict(GPU_CASES[name])
    K, with_scales = d.pop("K"), d.pop("scales", False)
    scales = np.asarray(np.random.default_rng(seed + 100).uniform(0.8, 1.2, (9, n)), dtype=np.float32).astype(np.float64) if with_scales else None
    return config(**d), K, scales


# ---- the far side of the selects ---------------------------------------------------------------------------------------------------
#: the edge cases of tests/test_gpu_diff.py (and of the host tests that establish their conditions): 200 drones (ld = 256: four waves),
#: task hover, one airframe per kind and all three over the table (the sub-step's adjoint branches on the airframe).  `tumble` keeps
#: K S at 4 sub-steps: explicit Euler amplifies the off-axis rates by about 1.7x per sub-step at those speeds.
EDGE_CASES = {
    "tumble": dict(model="cf2x", act="rpm", S=2, drag=False, K=2),
    "gimbal": dict(model="racer", act="one_d_rpm", S=2, drag=False, K=3),
    "near_gimbal": dict(model="racer", act="one_d_rpm", S=2, drag=False, K=3),
    "reward_far": dict(model="cf2x", act="rpm", S=2, drag=True, K=4),
    "wide_attitude": dict(model="cf2p", act="rpm", S=2, drag=True, K=4),
}
EDGE_N = 200
#: pitch of the `near_gimbal` lanes: sin(85 deg) = 0.99619, 3.8e-3 below the gimbal test, 1 / cos(pitch) = 11.5.  Nearer is not a
#: float32 question any more: the asin adjoint divides by sqrt((1 - s)(1 + s)) of an s that float32 products round at 3e-8, and the
#: float32 restatement itself leaves the 1e-5 rule of tests/test_host_diff.py (86.5 deg: 8e-6 .. 1.0e-5 over three draws, 88 deg --
#: which also sits inside the 1e-3 every lane keeps from every threshold -- 1.5e-5 .. 2.5e-5; 85 deg: below 3e-6)
NEAR_GIMBAL_PITCH = math.radians(85.0)


def edge_case(kind):
    """(cfg, K) of an edge case"""
    d = dict(EDGE_CASES[kind])
    K = d.pop("K")
    return config(**d), K


TUMBLE_PLANT_K = 1


def edge_scales(n=EDGE_N, seed=1):
    """plant scale factors [9, n] within +-20 %, every value a float32: `tumble` through the plant sweep, which flies the first step
    alone (TUMBLE_PLANT_K) -- with unequal inertias the second step's float32 restatement comes within 3 % of the 1e-5 rule"""
    return np.asarray(np.random.default_rng(seed + 100).uniform(0.8, 1.2, (9, n)), dtype=np.float32).astype(np.float64)


def rare_lanes(n=EDGE_N):
    """bool [n]: every third drone among drones 0 .. 127"""
    i = np.arange(n)
    return (i % 3 == 0) & (i < 128)


def make_edge_inputs(C, cfg, n, K, kind, seed=1):
    """`make_inputs` with the RARE lanes moved to the far side of a select, every value representable in float32.  The rare lanes are
    every third drone among drones 0 .. 127 (`rare_lanes`): with n = 200 the lanes of waves 0 and 1 diverge and waves 2 and 3 hold
    ordinary lanes only; every other lane is `make_inputs`' own.  By `kind`:
      tumble         body rates of 520 .. 700 rad/s, about z for every other rare lane and about a random body axis for the rest: more
                     than 1 rad per sub-step (u = (|w| h / 2)^2 > 1 beyond 480 rad/s), the exact sincos path of the quaternion update
      gimbal         pitch exactly +-pi/2 (alternating), roll 0, a random yaw, body rates zero.  Meant for ONE_D_RPM: four equal thrusts
                     give no torque, the rates stay zero and the lane stays in the gimbal branch at every step
      near_gimbal    the same lanes at pitch +-85 deg (NEAR_GIMBAL_PITCH): the regular branch where 1 / cos(pitch) is 11.5
      reward_far     1.25 .. 1.6 m from the target in a random direction: 2 - d^4 <= -0.44, the clamped side of the reward
      wide_attitude  roll and yaw anywhere in +-3.1 rad, pitch in +-1.3 rad, the quaternion's sign random (w < 0 for half of them) and
                     its length 0.95 .. 1.05, capped so that |q|^2 |sin pitch| <= 0.97: the gimbal test reads the unnormalised
                     2 (w y - x z), and the cap keeps these lanes on its regular side with room for the flight's drift
    numpy float64 arrays, plus `rare` (bool [n])."""
    inp = make_inputs(C, cfg, n, K, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)     # noqa: E731
    rare = rare_lanes(n)
    m = int(rare.sum())
    if kind == "tumble":
        axis = rng.standard_normal((m, 3))
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        axis[::2] = np.array([0.0, 0.0, 1.0])
        inp.rates[rare] = f32(axis * (rng.uniform(520.0, 700.0, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1))))
    elif kind in ("gimbal", "near_gimbal"):
        pitch = (0.5 * math.pi if kind == "gimbal" else NEAR_GIMBAL_PITCH) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
        rpy = np.stack([np.zeros(m), pitch, rng.uniform(-3.1, 3.1, m)], axis=-1)
        inp.quat[rare] = f32(quat_from_rpy(rpy))
        inp.rates[rare] = 0.0
    elif kind == "reward_far":
        direction = rng.standard_normal((m, 3))
        direction /= np.linalg.norm(direction, axis=-1, keepdims=True)
        inp.pos[rare] = f32(inp.target[rare] + direction * rng.uniform(1.25, 1.6, (m, 1)))
    elif kind == "wide_attitude":
        rpy = np.stack([rng.uniform(-3.1, 3.1, m), rng.uniform(-1.3, 1.3, m), rng.uniform(-3.1, 3.1, m)], axis=-1)
        length = np.minimum(rng.uniform(0.95, 1.05, m), np.sqrt(0.97 / np.maximum(np.abs(np.sin(rpy[:, 1])), 1e-3)))
        inp.quat[rare] = f32(quat_from_rpy(rpy) * (length * rng.choice([-1.0, 1.0], m))[:, None])
    else:
        raise ValueError(f"unknown edge kind {kind!r}")
    inp.rare = rare
    return inp


def with_cotangents(inp, g_obs=None, g_rew=None):
    """a copy of the inputs whose cotangents are zero but for the given ones (`g_obs` [K, n, 12], `g_rew` [K, n])"""
    out = SimpleNamespace(**vars(inp))
    out.g_obs = np.zeros_like(inp.g_obs) if g_obs is None else g_obs
    out.g_rew = np.zeros_like(inp.g_rew) if g_rew is None else g_rew
    for k in ("g_pos", "g_quat", "g_vel", "g_rates"):
        setattr(out, k, np.zeros_like(getattr(inp, k)))
    return out


def first_steps(inp, k):
    """the inputs cut to their first k steps"""
    out = SimpleNamespace(**vars(inp))
    out.K, out.actions, out.g_obs, out.g_rew = k, inp.actions[:k], inp.g_obs[:k], inp.g_rew[:k]
    return out


def lanes_of(inp, idx):
    """the inputs of the drones `idx` alone (every per-drone array sliced)"""
    out, idx = SimpleNamespace(**vars(inp)), np.asarray(idx)
    for k, v in vars(inp).items():
        if isinstance(v, np.ndarray):
            setattr(out, k, v[:, idx] if k in ("actions", "g_obs", "g_rew") else v[idx])
    out.n = len(idx)
    return out

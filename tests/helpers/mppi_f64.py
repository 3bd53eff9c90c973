"""The yardstick of `gpd_mppi` (include/gpd.h): a float64 numpy restatement written from the definitions -- Philox4x32-10, the uniforms
as the same float32 values, Box-Muller in float64, the clamp, the rollout through oracle.batched_oracle.BatchedAviary with N * M
aviaries (the physics and the DSLPID behind the oracle everything else is held against), the running cost, the softmax update -- and
the cases tests/test_gpu_mppi.py runs on the device, which tests/test_host_mppi.py examines without one.  Test infrastructure."""
import collections

import numpy as np

import obstacles_f64 as obst_y
from conftest import urdf

#: the project's ceiling for |x32 - x64| / max(1, |x64|)
CEILING = 1e-4
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


# ---- the noise -------------------------------------------------------------------------------------------------------------------
def philox(ctr, key):
    """Philox4x32-10: ctr [..., 4], key [..., 2] (unsigned 32-bit values) -> [..., 4] uint32"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & np.uint64(MASK), (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & np.uint64(MASK)]
        k = [(k[0] + np.uint64(W0)) & np.uint64(MASK), (k[1] + np.uint64(W1)) & np.uint64(MASK)]
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(words):
    """the float32 VALUE of ((x >> 8) + 0.5) 2^-24 -- exact below 2^23, rounded to even above, in (0, 1] -- as float64"""
    x = (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return ((x + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)


def box_muller(words):
    """[..., 4] words -> [..., 4] standard normals in float64: z0, z1 from words 0, 1 and z2, z3 from words 2, 3"""
    u = uniforms(words)
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    t0, t1 = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1)


def normals(N, M, H, iteration, seed):
    """z [N, M, H, 4]: the normals of the counters (n, m, h, iteration) under the key `seed`"""
    n, m, h = np.meshgrid(np.arange(N), np.arange(M), np.arange(H), indexing="ij")
    ctr = np.stack([n, m, h, np.full_like(n, iteration)], axis=-1)
    return box_muller(philox(ctr, np.broadcast_to(np.asarray(seed, dtype=np.uint64), ctr.shape[:-1] + (2,))))


def perturbed(u_in, sigma, lo, hi, M, iteration, seed):
    """a [N, M, H, 4] = clamp(u_in[h][n] + sigma z, lo, hi)"""
    H, N, _ = u_in.shape
    z = normals(N, M, H, iteration, seed)
    return np.clip(np.asarray(u_in, dtype=np.float64).transpose(1, 0, 2)[:, None] + np.asarray(sigma, dtype=np.float64) * z, lo, hi)


# ---- the update ------------------------------------------------------------------------------------------------------------------
def update(u_in, a, S, lam, lo, hi):
    """(u_out [H, N, 4], stats [N, 4]) from the samples' actions a [N, M, H, 4] and costs S [N, M]"""
    u = np.asarray(u_in, dtype=np.float64).transpose(1, 0, 2)                     # [N, H, 4]
    S = np.asarray(S, dtype=np.float64)
    fin = np.isfinite(S)
    N = len(S)
    u_out, stats = np.empty_like(u), np.zeros((N, 4))
    for n in range(N):
        if not fin[n].any():
            u_out[n] = np.clip(u[n], lo, hi)
            stats[n] = [np.inf, np.inf, 0.0, 0.0]
            continue
        smin = S[n][fin[n]].min()
        w = np.where(fin[n], np.exp(-(np.where(fin[n], S[n], smin) - smin) / lam), 0.0)
        u_out[n] = u[n] + np.einsum("m,mhk->hk", w, a[n] - u[n][None]) / w.sum()
        stats[n] = [smin, (w * np.where(fin[n], S[n], 0.0)).sum() / w.sum(), w.sum() ** 2 / (w * w).sum(), fin[n].sum()]
    return u_out.transpose(1, 0, 2), stats


# ---- the rollout and its cost ----------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name N M H S act obst goal_per_step iteration")
#: the device cases: a lone wave / a partial block / two blocks, one sample per lane / the sample loop, one step / five, one sub-step /
#: five, both action types, no list / a shared list of 3 / per-aviary lists of 7, a constant goal / one per step, iteration 0 / 7
CASES = [Case("rpm-1-64-h1-s1-none", 1, 64, 1, 1, "rpm", "none", False, 0),
         Case("rpm-3-192-h5-s5-shared", 3, 192, 5, 5, "rpm", "shared", True, 7),
         Case("rpm-6-64-h5-s1-lists", 6, 64, 5, 1, "rpm", "lists", False, 0),
         Case("rpm-6-192-h1-s5-none", 6, 192, 1, 5, "rpm", "none", True, 7),
         Case("vel-1-192-h5-s5-lists", 1, 192, 5, 5, "vel", "lists", True, 7),
         Case("vel-3-64-h1-s1-none", 3, 64, 1, 1, "vel", "none", False, 0),
         Case("vel-6-192-h5-s5-shared", 6, 192, 5, 5, "vel", "shared", False, 7),
         Case("vel-6-64-h5-s1-lists", 6, 64, 5, 1, "vel", "lists", True, 0)]
Weights = collections.namedtuple("Weights", "w_pos w_vel w_tilt w_rate w_term w_obs obst_margin collision_radius")
Inputs = collections.namedtuple("Inputs", "pos quat vel rates pid u_in goal obst sigma lo hi lam weights seed")
ACT_CODE = {"rpm": 0, "vel": 2}


def make_lists(rng, n_lists, n_obst, centre):
    """[n_lists, n_obst, 8] float32 records around the drones' `centre`: spheres, boxes and cylinders close enough for the hinge to
    act; with seven records one is skipped (NONE, with garbage sizes) and the last is a floor"""
    kinds = rng.choice([obst_y.SPHERE, obst_y.BOX, obst_y.CYLINDER], size=(n_lists, n_obst))
    out = np.zeros((n_lists, n_obst, 8))
    out[..., 0:3] = centre + rng.uniform(-0.9, 0.9, size=(n_lists, n_obst, 3))
    out[..., 4:7] = rng.uniform(0.1, 0.35, size=(n_lists, n_obst, 3))
    if n_obst >= 7:
        kinds[:, 2] = obst_y.NONE
        kinds[:, -1] = obst_y.FLOOR
        out[:, -1, 0:3] = 0.0
    out[..., 3] = kinds
    return out.astype(np.float32)


def make_inputs(case):
    """the case's float32 inputs (the yardstick sees the rounded values): a tilted, moving start state, non-zero controller members,
    a nominal inside the bounds with one row outside them, goals half a metre away, the lists"""
    rng = np.random.default_rng(sum(map(ord, case.name)))
    N, H = case.N, case.H
    from oracle import bullet_math as bm
    pos = rng.uniform([-0.3, -0.3, 0.35], [0.3, 0.3, 0.8], size=(N, 3))
    quat = bm.quaternion_from_euler_b(rng.uniform(-0.3, 0.3, size=(N, 3)))
    vel, rates = rng.uniform(-0.5, 0.5, size=(N, 3)), rng.uniform(-1.0, 1.0, size=(N, 3))
    pid = np.concatenate([rng.uniform(-0.1, 0.1, size=(N, 3)), bm.euler_from_quaternion_b(quat.astype(np.float32).astype(np.float64))
                          + rng.uniform(-0.002, 0.002, size=(N, 3)), rng.uniform(-0.2, 0.2, size=(N, 3))], axis=1)
    if case.act == "rpm":
        u_in = rng.uniform(-0.6, 0.6, size=(H, N, 4))
        sigma, lo, hi = [0.5, 0.4, 0.5, 0.3], [-1.0] * 4, [1.0] * 4
        weights = Weights(1.0, 0.5, 2.0, 0.5, 3.0, 5.0, 0.5, 0.06)
    else:
        u_in = np.concatenate([rng.uniform(-0.6, 0.6, size=(H, N, 3)), rng.uniform(0.2, 0.8, size=(H, N, 1))], axis=-1)
        sigma, lo, hi = [0.4, 0.4, 0.3, 0.25], [-1.0, -1.0, -1.0, 0.0], [1.0, 1.0, 1.0, 1.0]
        weights = Weights(1.0, 0.5, 2.0, 0.5, 3.0, 5.0, 0.5, 0.06)
    # the temperature follows the horizon's length in time (the costs' spread among the samples does): the weights are neither all equal
    # nor one sample's alone, and an error of 1e-6 of the costs moves them by ~1e-5 (tests/test_host_mppi.py checks both)
    lam = 0.04 * H * case.S
    if N * H > 1:
        u_in[0, 0] = [1.5, -1.25, 0.25, 1.5]                        # a row outside the bounds (by amounts float32 holds exactly)
    goal = pos[None] + rng.uniform(-0.5, 0.5, size=(H if case.goal_per_step else 1, N, 3))
    obst = None if case.obst == "none" else make_lists(rng, 1 if case.obst == "shared" else N, 3 if case.obst == "shared" else 7,
                                                       np.array([0.0, 0.0, 0.6]))
    f = lambda v: np.asarray(v, dtype=np.float32)       # noqa: E731
    return Inputs(f(pos), f(quat), f(vel), f(rates), f(pid), f(u_in), f(goal), obst, f(sigma), f(lo), f(hi), float(np.float32(lam)),
                  Weights(*[float(np.float32(w)) for w in weights]), (0x1234ABCD + case.N, 0x9E3779B1))


def rollout_costs(case, inp, a, model="cf2x", store32=False):
    """S [N, M]: every sample's H env steps through the batched oracle, scored after each step.  `store32`: everything that is carried
    from one env step to the next -- the kinematic state, the controller members, the running sum -- and every term of the cost is
    rounded to float32 (the oracle's arithmetic inside a step stays float64: it has no float32 form)"""
    r32 = (lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)) if store32 else (lambda v: v)
    from oracle import bullet_math as bm
    from oracle.batched_oracle import BatchedAviary
    N, M, H = case.N, case.M, case.H
    E = N * M
    orc = BatchedAviary(urdf(model), model, E, 1, physics_flags=0, pyb_freq=240, ctrl_freq=240 // case.S, act=case.act, task="none")
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64), M, axis=0)[:, None]       # noqa: E731  [N, k] -> [N * M, 1, k]
    orc.pos, orc.quat, orc.vel, orc.rpy_rates = rep(inp.pos), rep(inp.quat), rep(inp.vel), rep(inp.rates)
    orc.rpy = bm.euler_from_quaternion_b(orc.quat)
    if case.act == "vel":
        orc.pid.integral_pos_e, orc.pid.last_rpy, orc.pid.integral_rpy_e = rep(inp.pid[:, 0:3]), rep(inp.pid[:, 3:6]), rep(inp.pid[:, 6:9])
    w = inp.weights
    lists = None if inp.obst is None else np.repeat(inp.obst.astype(np.float64), M if len(inp.obst) > 1 else 1, axis=0)
    S = np.zeros(E)
    for h in range(H):
        orc.step(r32(a[:, :, h].reshape(E, 1, 4)))
        orc.pos, orc.quat, orc.vel, orc.rpy_rates, orc.rpy = r32(orc.pos), r32(orc.quat), r32(orc.vel), r32(orc.rpy_rates), r32(orc.rpy)
        if case.act == "vel":
            orc.pid.integral_pos_e, orc.pid.last_rpy, orc.pid.integral_rpy_e = r32(orc.pid.integral_pos_e), r32(orc.pid.last_rpy), r32(orc.pid.integral_rpy_e)
        g = rep(inp.goal[h if case.goal_per_step else 0])[:, 0]
        p, v, om = orc.pos[:, 0], orc.vel[:, 0], orc.rpy_rates[:, 0]
        r22 = bm.matrix_from_quaternion_b(orc.quat)[:, 0, 2, 2]
        c = r32(w.w_pos * (w.w_term if h == H - 1 else 1.0) * ((p - g) ** 2).sum(-1)) + r32(w.w_vel * (v * v).sum(-1)) + r32(w.w_tilt * (1.0 - r22)) \
            + r32(w.w_rate * (om * om).sum(-1))
        if lists is not None:
            d = r32(obst_y.sdf(lists, p)[0].min(axis=1))
            c = c + r32(w.w_obs * np.maximum(0.0, w.obst_margin - (d - w.collision_radius)) ** 2)
        S = r32(S + c)
    return S.reshape(N, M)


def plan(case, inp=None, store32=False):
    """the whole call in float64: dict(a [N, M, H, 4], costs [N, M], u_out [H, N, 4], stats [N, 4]); `store32`: see rollout_costs (the
    actions rounded to float32 too)"""
    inp = make_inputs(case) if inp is None else inp
    a = perturbed(inp.u_in, inp.sigma, inp.lo.astype(np.float64), inp.hi.astype(np.float64), case.M, case.iteration, inp.seed)
    S = rollout_costs(case, inp, a, store32=store32)
    u_out, stats = update(inp.u_in, a, S, inp.lam, inp.lo.astype(np.float64), inp.hi.astype(np.float64))
    return dict(a=a, costs=S, u_out=u_out, stats=stats)


def rel_err(x32, x64):
    x64 = np.asarray(x64, dtype=np.float64)
    return np.abs(np.asarray(x32, dtype=np.float64) - x64) / np.maximum(1.0, np.abs(x64))

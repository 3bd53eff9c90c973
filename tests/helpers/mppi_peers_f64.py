"""The yardstick of `gpd_mppi_peers` (include/gpd.h): the float64 plan of mppi_f64 (RPM, VEL: the batched oracle with its DSLPID) and of
mppi_ctbr_f64 (CTBR: ctbr_f64.CtbrF64) with the peers' hinge in the running cost and the path of the new nominal -- the noise, the
clamp, the softmax update, the obstacle lists and the metric are those helpers'; the rollout is restated here because neither exposes
the samples' positions step by step -- and the cases tests/test_gpu_mppi_peers.py runs on the device, which
tests/test_host_mppi_peers.py examines without one.  Test infrastructure."""
import collections

import numpy as np

import mppi_ctbr_f64 as yc
import mppi_f64 as y
import obstacles_f64 as obst_y
from conftest import urdf

CEILING = y.CEILING
rel_err = y.rel_err

Case = collections.namedtuple("Case", "name act model N M H S k extra obst stride0 goal_per_step iteration")
#: the device cases -- a lone wave with 3 intruder rows (n_rows > N), a full block and a block of one wave (N = 5), three blocks (9);
#: one sample per lane / the sample loop; one step / five; one sub-step / five; k = 1, 3, 32 (idx_ld = k + 2 everywhere); one row set
#: for every step (`stride0`) / a table with a step stride of 4 (n_rows + 3); the three models, no list / a shared list, the three
#: airframes (VEL needs DSLPID: cf2x)
CASES = [Case("rpm-cf2x-1-64-h1-s1-k1", "rpm", "cf2x", 1, 64, 1, 1, 1, 3, "none", True, False, 0),
         Case("vel-cf2x-5-128-h5-s5-k3", "vel", "cf2x", 5, 128, 5, 5, 3, 0, "shared", False, True, 7),
         Case("ctbr-racer-9-64-h5-s1-k32", "ctbr", "racer", 9, 64, 5, 1, 32, 2, "none", False, False, 0),
         Case("rpm-cf2p-9-128-h5-s5-k3", "rpm", "cf2p", 9, 128, 5, 5, 3, 0, "shared", True, True, 7),
         Case("vel-cf2x-9-64-h1-s1-k32", "vel", "cf2x", 9, 64, 1, 1, 32, 1, "none", True, False, 0),
         Case("ctbr-cf2p-5-128-h1-s5-k1", "ctbr", "cf2p", 5, 128, 1, 5, 1, 0, "shared", False, True, 7),
         Case("ctbr-cf2x-1-128-h5-s5-k3", "ctbr", "cf2x", 1, 128, 5, 5, 3, 3, "none", True, False, 7),
         Case("rpm-racer-5-64-h5-s1-k32", "rpm", "racer", 5, 64, 5, 1, 32, 0, "none", False, True, 0),
         Case("vel-cf2x-1-64-h5-s5-k3", "vel", "cf2x", 1, 64, 5, 5, 3, 3, "shared", False, False, 7),
         Case("rpm-cf2x-5-64-h1-s5-k1", "rpm", "cf2x", 5, 64, 1, 5, 1, 0, "shared", True, False, 0)]
Inputs = collections.namedtuple("Inputs", "pos quat vel rates pid u_in goal obst sigma lo hi lam weights seed idx table w_peer peer_dist")
PEER_DIST, W_PEER = 0.5, 4.0


def base_case(case):
    """the case of the model's own yardstick whose start states, nominal, goals, list and sampler this one takes"""
    if case.act == "ctbr":
        return yc.Case(case.name, case.model, case.N, case.M, case.H, case.S, case.obst, case.goal_per_step, case.iteration, False)
    return y.Case(case.name, case.N, case.M, case.H, case.S, case.act, case.obst, case.goal_per_step, case.iteration)


def make_inputs(case):
    """the float32 inputs of the model's own yardstick, and the peers: a table [H or 1, n_rows, 4] (float32; w is garbage the kernel must
    ignore) in which a drone's row is its start carried on at its start velocity plus a wobble, an intruder's row a point 0.15 .. 0.3 m
    from some drone that drifts; one row NaN where there are rows enough; and idx [N, k + 2] (int32) of the other rows in a random order
    (the drones' start points lie within 0.6 m x 0.6 m x 0.45 m: with peer_dist 0.5 m the hinge acts), with -1 in the middle of a row,
    a drone's own row, an entry >= n_rows, a drone whose entries are all -1 -- and, in the two columns beyond k, close rows the kernel
    must not read"""
    b = base_case(case)
    base = yc.make_inputs(b) if case.act == "ctbr" else y.make_inputs(b)
    rng = np.random.default_rng(sum(map(ord, case.name)) + 2)
    N, H, k = case.N, case.H, case.k
    n_rows = N + case.extra
    dt = case.S / 240.0
    steps = 1 if case.stride0 else H
    table = np.zeros((steps, n_rows, 4))
    for h in range(steps):
        table[h, :N, :3] = base.pos + base.vel * dt * (h + 1) + rng.uniform(-0.02, 0.02, size=(N, 3))
    for r in range(N, n_rows):
        start = base.pos[rng.integers(N)] + rng.uniform(0.15, 0.3) * (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
        table[:, r, :3] = start + np.arange(1, steps + 1)[:, None] * dt * rng.uniform(-0.5, 0.5, size=3)
    table[..., 3] = rng.uniform(-9.0, 9.0, size=table.shape[:-1])
    idx = np.full((N, k + 2), -1, dtype=np.int32)
    for n in range(N):
        others = rng.permutation([r for r in range(n_rows) if r != n])
        fill = others[:k]
        idx[n, :len(fill)] = fill
        idx[n, k:] = others[:2] if len(others) >= 2 else np.resize(others, 2)          # beyond k: never read
    if n_rows >= 5:
        table[:, idx[0, 0]] = np.nan                                  # a row that is not finite (drone 0's first entry names it)
    if N >= 5 and k >= 3:
        idx[1, 1] = -1                                                # -1 in the middle: the entries behind it still count
        idx[2, 0] = 2                                                 # the drone's own row
        idx[3, 1] = n_rows + 4                                        # beyond the table
        idx[4, :k] = -1                                               # a drone without peers
    f = lambda v: np.asarray(v, dtype=np.float32)       # noqa: E731
    pid = getattr(base, "pid", None)
    return Inputs(base.pos, base.quat, base.vel, base.rates, pid, base.u_in, base.goal, base.obst, base.sigma, base.lo, base.hi, base.lam,
                  base.weights, base.seed, idx, f(table), float(np.float32(W_PEER)), float(np.float32(PEER_DIST)))


def counted(case, inp):
    """per drone the entries of its idx row that count, in order: in 0 .. n_rows - 1 and not the drone's own row"""
    n_rows = inp.table.shape[1]
    return [[int(r) for r in inp.idx[n, :case.k] if 0 <= r < n_rows and r != n] for n in range(case.N)]


def hinge(peer_dist, d):
    """max(0, peer_dist - d)^2, and 0 for a distance that is not finite"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(d), np.maximum(0.0, peer_dist - d), 0.0) ** 2


def peer_terms(case, inp, h, p):
    """(sum of the hinges [N, B], nearest distance [N, B]) of the points p [N, B, 3] against the table's rows after step h"""
    rows = inp.table[0 if case.stride0 else h, :, :3].astype(np.float64)
    total, nearest = np.zeros(p.shape[:2]), np.full(p.shape[:2], np.inf)
    for n, cnt in enumerate(counted(case, inp)):
        for r in cnt:
            d = np.sqrt(((p[n] - rows[r]) ** 2).sum(-1))
            with np.errstate(invalid="ignore"):
                total[n] += hinge(inp.peer_dist, d)
                nearest[n] = np.where(d < nearest[n], d, nearest[n])
    return total, nearest


class Model:
    """B copies of each of the case's N drones under the case's model, in float64"""

    def __init__(self, case, inp, B):
        self.case, self.E = case, case.N * B
        rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64), B, axis=0)       # noqa: E731  [N, k] -> [N * B, k]
        if case.act == "ctbr":
            import ctbr_f64
            self.sim = ctbr_f64.CtbrF64(case.model, self.E, pos=rep(inp.pos), quat=rep(inp.quat), vel=rep(inp.vel), w=rep(inp.rates), pyb_freq=240,
                                        ctrl_freq=240 // case.S)
            self.av = self.sim.av
        else:
            from oracle import bullet_math as bm
            from oracle.batched_oracle import BatchedAviary
            av = BatchedAviary(urdf(case.model), case.model, self.E, 1, physics_flags=0, pyb_freq=240, ctrl_freq=240 // case.S, act=case.act, task="none")
            av.pos, av.quat, av.vel, av.rpy_rates = rep(inp.pos)[:, None], rep(inp.quat)[:, None], rep(inp.vel)[:, None], rep(inp.rates)[:, None]
            av.rpy = bm.euler_from_quaternion_b(av.quat)
            if case.act == "vel":
                av.pid.integral_pos_e, av.pid.last_rpy, av.pid.integral_rpy_e = rep(inp.pid[:, 0:3])[:, None], rep(inp.pid[:, 3:6])[:, None], rep(inp.pid[:, 6:9])[:, None]
            self.sim, self.av = None, av

    def step(self, a):
        """one step on the actions a [E, 4]"""
        if self.case.act == "ctbr":
            self.sim.step(a)
        else:
            self.av.step(a.reshape(self.E, 1, 4))


def rollout_costs(case, inp, a, peers=True):
    """(S [N, M], peer [N, M]): every sample's H steps, scored after each one as `mppi_f64.rollout_costs` scores it, plus w_peer times the
    hinges' sum; `peer` is that part of S alone"""
    from oracle import bullet_math as bm
    N, M, H = case.N, case.M, case.H
    sim = Model(case, inp, M)
    av, w = sim.av, inp.weights
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64), M, axis=0)       # noqa: E731
    S, part = np.zeros(N * M), np.zeros(N * M)
    for h in range(H):
        sim.step(a[:, :, h].reshape(N * M, 4))
        g = rep(inp.goal[h if case.goal_per_step else 0])
        p, v, om = av.pos[:, 0], av.vel[:, 0], av.rpy_rates[:, 0]
        r22 = bm.matrix_from_quaternion_b(av.quat)[:, 0, 2, 2]
        c = w.w_pos * (w.w_term if h == H - 1 else 1.0) * ((p - g) ** 2).sum(-1) + w.w_vel * (v * v).sum(-1) + w.w_tilt * (1.0 - r22) \
            + w.w_rate * (om * om).sum(-1)
        if inp.obst is not None:
            d = obst_y.sdf(inp.obst.astype(np.float64), p)[0].min(axis=1)
            c = c + w.w_obs * np.maximum(0.0, w.obst_margin - (d - w.collision_radius)) ** 2
        if peers:
            pen = inp.w_peer * peer_terms(case, inp, h, p.reshape(N, M, 3))[0].reshape(-1)
            c, part = c + pen, part + pen
        S = S + c
    return S.reshape(N, M), part.reshape(N, M)


def nominal_path(case, inp, u):
    """path [H, N, 4]: the nominal u [H, N, 4] flown without noise from the start state; x, y, z after each step and the distance to the
    nearest counted peer there (+inf: none)"""
    sim = Model(case, inp, 1)
    out = np.zeros((case.H, case.N, 4))
    for h in range(case.H):
        sim.step(np.asarray(u[h], dtype=np.float64))
        p = sim.av.pos[:, 0]
        out[h, :, :3] = p
        out[h, :, 3] = peer_terms(case, inp, h, p[:, None])[1][:, 0]
    return out


def plan(case, inp=None, peers=True):
    """the whole call in float64: dict(a [N, M, H, 4], costs [N, M], peer [N, M], u_out [H, N, 4], stats [N, 4], path [H, N, 4])"""
    inp = make_inputs(case) if inp is None else inp
    lo, hi = inp.lo.astype(np.float64), inp.hi.astype(np.float64)
    a = y.perturbed(inp.u_in, inp.sigma, lo, hi, case.M, case.iteration, inp.seed)
    S, part = rollout_costs(case, inp, a, peers=peers)
    u_out, stats = y.update(inp.u_in, a, S, inp.lam, lo, hi)
    return dict(a=a, costs=S, peer=part, u_out=u_out, stats=stats, path=nominal_path(case, inp, np.clip(u_out, lo, hi)))


def path_err(got, want):
    """the metric on path_out: rel_err, an infinite distance matching an infinite one exactly"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want)
    assert (got[inf] == want[inf]).all()
    return rel_err(np.where(inf, 0.0, got), np.where(inf, 0.0, want))

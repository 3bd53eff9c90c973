"""The yardstick of `gpd_mppi_ctbr` (include/gpd.h): composed from the float64 helpers that exist -- the noise, the clamp, the softmax
update, the obstacle lists and the metric of mppi_f64.py, and the closed loop of ctbr_f64.CtbrF64 (the rate loop of DESIGN.md section
3.17 in every sub-step of the oracle's explicit integrator) over N * M aviaries -- with the running cost written as in
`mppi_f64.rollout_costs`; and the cases tests/test_gpu_mppi_ctbr.py runs on the device, which tests/test_host_mppi_ctbr.py examines
without one.  Test infrastructure."""
import collections

import numpy as np

import ctbr_f64 as ctbr_y
import mppi_f64 as y
import obstacles_f64 as obst_y

CEILING = y.CEILING
rel_err = y.rel_err

Case = collections.namedtuple("Case", "name model N M H S obst goal_per_step iteration wide")
#: the device cases: a lone wave / a partial block / two blocks, one sample per lane / the sample loop, one step / five, one sub-step /
#: five, no list / a shared list of 3 / per-aviary lists of 7, a constant goal / one per step, iteration 0 / 7, bounds inside the
#: controller's clips / wider than thrust_max and rate_max (`wide`: the rate loop's own clips act), the three airframes (the other
#: allocation on cf2p, the other sign of the yaw torque on racer)
CASES = [Case("cf2x-1-64-h1-s1-none", "cf2x", 1, 64, 1, 1, "none", False, 0, False),
         Case("cf2x-3-192-h5-s5-lists", "cf2x", 3, 192, 5, 5, "lists", True, 7, True),
         Case("cf2x-6-64-h5-s1-lists", "cf2x", 6, 64, 5, 1, "lists", False, 0, False),
         Case("cf2x-6-192-h1-s5-none", "cf2x", 6, 192, 1, 5, "none", True, 7, True),
         Case("racer-3-64-h5-s5-shared", "racer", 3, 64, 5, 5, "shared", False, 0, False),
         Case("cf2p-6-192-h5-s1-shared", "cf2p", 6, 192, 5, 1, "shared", True, 7, True),
         Case("cf2p-1-192-h5-s5-lists", "cf2p", 1, 192, 5, 5, "lists", False, 7, True),
         Case("racer-6-64-h1-s1-lists", "racer", 6, 64, 1, 1, "lists", True, 0, False)]
Inputs = collections.namedtuple("Inputs", "pos quat vel rates u_in goal obst sigma lo hi lam weights seed")

#: bounds inside the controller's clips (thrust_max 40.9 m/s^2, rate_max 2 pi rad/s), and bounds beyond them on the upper thrust and on
#: the rates; the nominal row put outside either (by amounts float32 holds exactly)
INSIDE = ([2.0, -4.0, -4.0, -3.0], [18.0, 4.0, 4.0, 3.0], [20.0, -5.0, 4.5, 1.0])
WIDE = ([4.0, -7.0, -7.0, -7.0], [45.0, 7.0, 7.0, 7.0], [48.0, -9.0, 7.5, 1.0])


def make_inputs(case):
    """the case's float32 inputs: the tilted, moving start states, goals and lists of `mppi_f64.make_inputs`; a nominal of 7 .. 13 m/s^2
    and +-2 rad/s with one row outside the bounds; the noise (3, 2.5, 2.5, 1.5)"""
    base = y.make_inputs(y.Case(case.name, case.N, case.M, case.H, case.S, "rpm", case.obst, case.goal_per_step, case.iteration))
    rng = np.random.default_rng(sum(map(ord, case.name)) + 1)
    N, H = case.N, case.H
    u_in = np.concatenate([rng.uniform(7.0, 13.0, size=(H, N, 1)), rng.uniform(-2.0, 2.0, size=(H, N, 3))], axis=-1)
    lo, hi, outside = WIDE if case.wide else INSIDE
    if N > 1:                       # (a lone drone keeps its nominal inside: its samples are the case's only ones)
        u_in[0, 0] = outside
    # the temperature: the costs' spread among the samples follows the horizon's length in time, and thrust and rate commands spread the
    # end states further than RPM fractions do -- four times the factor of mppi_f64's cases, so that the conditions
    # tests/test_host_mppi_ctbr.py states hold on every case (with 0.04 four of them miss the conditioning bound, up to 3.5e-5, and two
    # have a drone whose effective sample size is below 1.5)
    lam = 0.16 * H * case.S
    f = lambda v: np.asarray(v, dtype=np.float32)       # noqa: E731
    return Inputs(base.pos, base.quat, base.vel, base.rates, f(u_in), base.goal, base.obst, f([3.0, 2.5, 2.5, 1.5]), f(lo), f(hi),
                  float(np.float32(lam)), base.weights, base.seed)


def rollout_costs(case, inp, a, store32=False):
    """(S [N, M], at_zero [N, M], at_max [N, M]): every sample's H control steps through CtbrF64, scored after each step; the flags
    say that some rotor of the sample was held at 0 / at f_max in some sub-step.  `store32`: what is carried from one control step to
    the next -- the kinematic state, the running sum -- and every term of the cost is rounded to float32 (the arithmetic inside a
    step stays float64, as in `mppi_f64.rollout_costs`)"""
    r32 = (lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)) if store32 else (lambda v: v)
    from oracle import bullet_math as bm
    N, M, H = case.N, case.M, case.H
    E = N * M
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64), M, axis=0)       # noqa: E731  [N, k] -> [N * M, k]
    sim = ctbr_y.CtbrF64(case.model, E, pos=rep(inp.pos), quat=rep(inp.quat), vel=rep(inp.vel), w=rep(inp.rates), pyb_freq=240, ctrl_freq=240 // case.S)
    av, w = sim.av, inp.weights
    lists = None if inp.obst is None else np.repeat(inp.obst.astype(np.float64), M if len(inp.obst) > 1 else 1, axis=0)
    S = np.zeros(E)
    for h in range(H):
        sim.step(r32(a[:, :, h].reshape(E, 4)))
        av.pos, av.quat, av.vel, av.rpy_rates = r32(av.pos), r32(av.quat), r32(av.vel), r32(av.rpy_rates)
        g = rep(inp.goal[h if case.goal_per_step else 0])
        p, v, om = av.pos[:, 0], av.vel[:, 0], av.rpy_rates[:, 0]
        r22 = bm.matrix_from_quaternion_b(av.quat)[:, 0, 2, 2]
        c = r32(w.w_pos * (w.w_term if h == H - 1 else 1.0) * ((p - g) ** 2).sum(-1)) + r32(w.w_vel * (v * v).sum(-1)) + r32(w.w_tilt * (1.0 - r22)) \
            + r32(w.w_rate * (om * om).sum(-1))
        if lists is not None:
            d = r32(obst_y.sdf(lists, p)[0].min(axis=1))
            c = c + r32(w.w_obs * np.maximum(0.0, w.obst_margin - (d - w.collision_radius)) ** 2)
        S = r32(S + c)
    return S.reshape(N, M), sim.at_zero.reshape(N, M), sim.at_max.reshape(N, M)


def plan(case, inp=None, store32=False):
    """the whole call in float64: dict(a [N, M, H, 4], costs [N, M], u_out [H, N, 4], stats [N, 4], at_zero, at_max [N, M])"""
    inp = make_inputs(case) if inp is None else inp
    lo, hi = inp.lo.astype(np.float64), inp.hi.astype(np.float64)
    a = y.perturbed(inp.u_in, inp.sigma, lo, hi, case.M, case.iteration, inp.seed)
    S, at_zero, at_max = rollout_costs(case, inp, a, store32=store32)
    u_out, stats = y.update(inp.u_in, a, S, inp.lam, lo, hi)
    return dict(a=a, costs=S, u_out=u_out, stats=stats, at_zero=at_zero, at_max=at_max)


def nominal_costs(case, inp, obs):
    """[N]: the cost in float64 of observations obs [H, N, 12] (pos | rpy | vel | ang_v in the world frame, as gpd_rollout_ctbr
    stores them) without a list: |omega_body| = |omega_world|, R22 = cos(roll) cos(pitch)"""
    w = inp.weights
    S = np.zeros(case.N)
    for h in range(case.H):
        o = np.asarray(obs[h], dtype=np.float64)
        g = inp.goal[h if case.goal_per_step else 0].astype(np.float64)
        S += w.w_pos * (w.w_term if h == case.H - 1 else 1.0) * ((o[:, 0:3] - g) ** 2).sum(-1) + w.w_vel * (o[:, 6:9] ** 2).sum(-1) \
            + w.w_tilt * (1.0 - np.cos(o[:, 3]) * np.cos(o[:, 4])) + w.w_rate * (o[:, 9:12] ** 2).sum(-1)
    return S

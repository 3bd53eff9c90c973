"""The yardstick of `gpd_mppi_plant` (include/gpd.h): composed from the float64 helpers that exist -- the noise, the clamp, the softmax
update, the lists and the metric of mppi_f64.py, the inputs of mppi_f64 / mppi_ctbr_f64 -- with the rollout through ONE oracle PER
DRONE (oracle.batched_oracle.BatchedAviary for RPM and VEL, ctbr_f64.CtbrF64 for CTBR, E = M samples each) whose `physics_flags` are
the case's and whose plant constants are scaled by the drone's row of the table, as tests/test_gpu_plant.py scales its oracle
(restated here: HOVER_RPM, MAX_RPM and the controllers stay nominal); and the cases tests/test_gpu_mppi_plant.py runs on the device,
which tests/test_host_mppi_plant.py examines without one.  Test infrastructure."""
import collections

import numpy as np

import ctbr_f64 as ctbr_y
import mppi_ctbr_f64 as yc
import mppi_f64 as y
import obstacles_f64 as obst_y
from conftest import urdf

CEILING = y.CEILING
rel_err = y.rel_err
GND, DRAG, DW, GROUND, DAMP = 1, 2, 4, 8, 16
SCALE_FIELDS = ("mass", "ixx", "iyy", "izz", "kf", "km", "drag_xy", "drag_z", "gnd_eff")
#: how far the start heights (and the goals) of mppi_f64.make_inputs are lowered: 0.10 .. 0.55 m, where the ground effect is read
LOWER = 0.25

Case = collections.namedtuple("Case", "name act N M H S obst goal_per_step iteration flags table temp salt", defaults=(1.0, ""))
#: the device cases: a lone wave / a partial block / two blocks, one sample per lane / the sample loop, one step / five, one sub-step /
#: five, RPM / VEL / CTBR, no list / a shared list of 3 / per-aviary lists of 7, no flag / GND|DRAG / GND|DRAG|GROUND|DAMP, no table / a
#: table of nine scales from U(0.8, 1.25) per drone (pitch N + 5, NaN beyond N); every flag set and every table state with every action
#: type.  A flag needs time to move a cost: the flagged cases are the long ones.  `temp`: the temperature relative to the rule of
#: mppi_f64 / mppi_ctbr_f64.make_inputs, `salt`: appended to the name that seeds the inputs -- chosen so that EVERY drone's effective
#: sample size lies strictly between 2 and M / 2 (tests/test_host_mppi_plant.py)
CASES = [Case("rpm-1-64-h1-s1-none-f0-table", "rpm", 1, 64, 1, 1, "none", False, 0, 0, True, 0.5),
         Case("rpm-3-192-h5-s5-shared-f27-table", "rpm", 3, 192, 5, 5, "shared", True, 7, GND | DRAG | GROUND | DAMP, True, 0.5),
         Case("rpm-6-64-h5-s5-lists-f3", "rpm", 6, 64, 5, 5, "lists", False, 0, GND | DRAG, False, 0.5),
         Case("rpm-6-192-h1-s5-none-f0-table", "rpm", 6, 192, 1, 5, "none", True, 7, 0, True, 0.25),
         Case("vel-1-64-h1-s1-none-f0-table", "vel", 1, 64, 1, 1, "none", False, 0, 0, True, 2.0),
         Case("vel-3-192-h5-s5-lists-f3-table", "vel", 3, 192, 5, 5, "lists", True, 7, GND | DRAG, True, 1.0),
         Case("vel-6-192-h5-s5-shared-f27", "vel", 6, 192, 5, 5, "shared", False, 7, GND | DRAG | GROUND | DAMP, False, 0.7, "-i"),
         Case("ctbr-1-192-h5-s5-none-f3", "ctbr", 1, 192, 5, 5, "none", False, 7, GND | DRAG, False, 0.5),
         Case("ctbr-3-64-h1-s1-lists-f0-table", "ctbr", 3, 64, 1, 1, "lists", True, 0, 0, True, 0.5),
         Case("ctbr-6-192-h5-s5-shared-f27-table", "ctbr", 6, 192, 5, 5, "shared", True, 7, GND | DRAG | GROUND | DAMP, True, 0.5),
         Case("ctbr-6-64-h5-s1-lists-f0-table", "ctbr", 6, 64, 5, 1, "lists", False, 0, 0, True, 0.5)]
Inputs = collections.namedtuple("Inputs", "pos quat vel rates pid u_in goal obst sigma lo hi lam weights seed last_rpm scales")


def make_inputs(case):
    """the case's float32 inputs: those of `mppi_f64.make_inputs` (RPM, VEL) or `mppi_ctbr_f64.make_inputs` (CTBR, cf2x, bounds inside
    the clips) with the start heights and the goals lowered by LOWER; the last RPMs within +-15 % of hover; the scales [9, N] (None
    without a table); the temperature times `case.temp`"""
    name = case.name + case.salt
    if case.act == "ctbr":
        base = yc.make_inputs(yc.Case(name, "cf2x", case.N, case.M, case.H, case.S, case.obst, case.goal_per_step, case.iteration, False))
        pid = None
    else:
        base = y.make_inputs(y.Case(name, case.N, case.M, case.H, case.S, case.act, case.obst, case.goal_per_step, case.iteration))
        pid = base.pid
    rng = np.random.default_rng(sum(map(ord, name)) + 2)
    down = np.float32([0.0, 0.0, LOWER])
    last_rpm = rng.uniform(0.85, 1.15, size=(case.N, 4)) * 14468.0
    scales = rng.uniform(0.8, 1.25, size=(len(SCALE_FIELDS), case.N)) if case.table else None
    f = lambda v: None if v is None else np.asarray(v, dtype=np.float32)       # noqa: E731
    return Inputs(base.pos - down, base.quat, base.vel, base.rates, pid, base.u_in, base.goal - down, base.obst, base.sigma, base.lo, base.hi,
                  float(np.float32(base.lam * case.temp)), base.weights, base.seed, f(last_rpm), f(scales))


def scale_oracle(b, s):
    """the plant constants of the oracle `b` scaled by the dict `s` of the nine factors (tests/test_gpu_plant.py `_scale_oracle`,
    restated): M, GRAVITY = G M, J and J_INV, KF, KM, DRAG_COEFF, GND_EFF_COEFF; HOVER_RPM, MAX_RPM and the controller stay nominal"""
    C = b.C
    C.M = C.M * s["mass"]
    C.GRAVITY = C.G * C.M
    J = np.diag(np.diag(C.J) * np.array([s["ixx"], s["iyy"], s["izz"]]))
    C.J, C.J_INV = J, np.linalg.inv(J)
    C.KF, C.KM = C.KF * s["kf"], C.KM * s["km"]
    C.DRAG_COEFF = C.DRAG_COEFF * np.array([s["drag_xy"], s["drag_xy"], s["drag_z"]])
    C.GND_EFF_COEFF = C.GND_EFF_COEFF * s["gnd_eff"]


def ground_z(model="cf2x"):
    """the height the ground plane holds a drone at (oracle/batched_oracle.py `_substep`)"""
    from oracle.aviary_oracle import UrdfConstants
    C = UrdfConstants(urdf(model), model)
    return C.COLLISION_H / 2 - C.COLLISION_Z_OFFSET


def rollout_costs(case, inp, a, flags=None, scales="case", model="cf2x"):
    """(S [N, M], lowest [N, M]): every sample's H steps through its drone's own oracle, scored after each step as
    `mppi_f64.rollout_costs` scores them, and the lowest height the sample had after a step.  `flags`, `scales` ([9, N] or None):
    in place of the case's"""
    from oracle import bullet_math as bm
    from oracle.batched_oracle import BatchedAviary
    flags = case.flags if flags is None else flags
    scales = inp.scales if isinstance(scales, str) else scales
    N, M, H = case.N, case.M, case.H
    w = inp.weights
    rep = lambda v: np.repeat(np.asarray(v, dtype=np.float64)[None], M, axis=0)       # noqa: E731  [k] -> [M, k]
    S, lowest = np.zeros((N, M)), np.full((N, M), np.inf)
    for n in range(N):
        if case.act == "ctbr":
            sim = ctbr_y.CtbrF64(model, M, pos=rep(inp.pos[n]), quat=rep(inp.quat[n]), vel=rep(inp.vel[n]), w=rep(inp.rates[n]),
                                 last_rpm=rep(inp.last_rpm[n]), physics_flags=flags, pyb_freq=240, ctrl_freq=240 // case.S)
            orc = sim.av
            step = lambda act: sim.step(act)       # noqa: E731
        else:
            orc = BatchedAviary(urdf(model), model, M, 1, physics_flags=flags, pyb_freq=240, ctrl_freq=240 // case.S, act=case.act, task="none")
            orc.pos, orc.quat, orc.vel, orc.rpy_rates = (rep(v)[:, None] for v in (inp.pos[n], inp.quat[n], inp.vel[n], inp.rates[n]))
            orc.rpy = bm.euler_from_quaternion_b(orc.quat)
            orc.last_rpm = rep(inp.last_rpm[n])[:, None]
            if case.act == "vel":
                orc.pid.integral_pos_e, orc.pid.last_rpy, orc.pid.integral_rpy_e = (rep(inp.pid[n, i:i + 3])[:, None] for i in (0, 3, 6))
            step = lambda act: orc.step(act[:, None])       # noqa: E731
        if scales is not None:
            scale_oracle(orc, {k: float(scales[i, n]) for i, k in enumerate(SCALE_FIELDS)})
        lists = None if inp.obst is None else np.repeat(inp.obst[n if len(inp.obst) > 1 else 0].astype(np.float64)[None], M, axis=0)
        for h in range(H):
            step(a[n, :, h])
            g = inp.goal[h if case.goal_per_step else 0][n].astype(np.float64)
            p, v, om = orc.pos[:, 0], orc.vel[:, 0], orc.rpy_rates[:, 0]
            r22 = bm.matrix_from_quaternion_b(orc.quat)[:, 0, 2, 2]
            c = w.w_pos * (w.w_term if h == H - 1 else 1.0) * ((p - g) ** 2).sum(-1) + w.w_vel * (v * v).sum(-1) + w.w_tilt * (1.0 - r22) \
                + w.w_rate * (om * om).sum(-1)
            if lists is not None:
                d = obst_y.sdf(lists, p)[0].min(axis=1)
                c = c + w.w_obs * np.maximum(0.0, w.obst_margin - (d - w.collision_radius)) ** 2
            S[n] += c
            lowest[n] = np.minimum(lowest[n], p[:, 2])
    return S, lowest


def plan(case, inp=None, flags=None, scales="case"):
    """the whole call in float64: dict(a [N, M, H, 4], costs [N, M], u_out [H, N, 4], stats [N, 4], lowest [N, M])"""
    inp = make_inputs(case) if inp is None else inp
    lo, hi = inp.lo.astype(np.float64), inp.hi.astype(np.float64)
    a = y.perturbed(inp.u_in, inp.sigma, lo, hi, case.M, case.iteration, inp.seed)
    S, lowest = rollout_costs(case, inp, a, flags, scales)
    u_out, stats = y.update(inp.u_in, a, S, inp.lam, lo, hi)
    return dict(a=a, costs=S, u_out=u_out, stats=stats, lowest=lowest)

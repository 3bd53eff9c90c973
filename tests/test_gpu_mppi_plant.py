"""MPPI on the aviary's own model on the MI355X: `gpd_mppi_plant` against the float64 yardstick (tests/helpers/mppi_plant_f64.py, examined
without a GPU in tests/test_host_mppi_plant.py) over the smallest shapes at which the kernel takes another path -- a lone wave, a
partial block, two blocks; one sample per lane and the sample loop; one step and five; one sub-step and five; RPM, VEL and CTBR; no
list, a shared one, per-aviary ones; no flag, GND|DRAG, GND|DRAG|GROUND|DAMP; no table and a table of pitch N + 5 with NaN beyond N --
then: without flags, without a table or with an all-ones one, the model's own entry bit for bit; at sigma 0 with every flag, a table and
drones that meet the ground plane, the costs of the project's own rollouts; the table indexed by drone; the `MPPI` / `CTBRMPPI` classes
with `model=` and `plant=`; and the example.

MEASURED on an MI355X (|x32 - x64| / max(1, |x64|), the largest over the eleven cases below; bound 1e-4):
    costs 9.1e-06 (vel-6-192-h5-s5-shared-f27)   u_out 2.4e-06   stats 1.1e-05 (vel-3-192-h5-s5-lists-f3-table)
Without flags, without a table or with an all-ones one: the bits of gpd_mppi / gpd_mppi_ctbr.  On the ground at sigma 0 against the
project's own rollouts (bound 1e-5): 6.0e-08 (RPM, 2 of 6 drones on the plane) 5.2e-08 (VEL, 1) 4.4e-08 (CTBR, 3).  Permuted columns:
permuted costs, the same bits.
The example at 32 drones, mean distance to the goal over the last second: model nominal 0.0955 m, model aviary 0.0231 m, a wrong belief
0.1352 m."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import mppi_plant_f64 as yq  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
PAD = 3
ACT_CODE = {"rpm": 0, "vel": 2, "ctbr": 6}
EVERY = yq.GND | yq.DRAG | yq.GROUND | yq.DAMP


def make_core(case, dev, flags=None):
    """(core, ctrl): single cf2x drones of the case's action type at 240 / S Hz under `flags` (None: the case's); ctrl: their
    VectorCTBR (CTBR) or None"""
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.control import VectorCTBR
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    core = engine.SimCore(drone_model=DroneModel.CF2X, num_envs=case.N, drones_per_env=1, physics=case.flags if flags is None else flags,
                          pyb_freq=240, ctrl_freq=240 // case.S, act_code=ACT_CODE[case.act], task=engine.TASK_NONE, auto_reset=False,
                          track_rpm=True, device=dev)
    return core, (VectorCTBR(case.N, DroneModel.CF2X, device=dev) if case.act == "ctbr" else None)


def set_state(core, inp):
    kin = np.concatenate([inp.pos, inp.quat, inp.vel, inp.rates], axis=1).T
    pid = torch.as_tensor(inp.pid.T.copy(), dtype=torch.float32) if core.pid is not None and inp.pid is not None else None
    core.set_state(kin=torch.as_tensor(kin, dtype=torch.float32), pid=pid, last_rpm=torch.as_tensor(inp.last_rpm.T.copy(), dtype=torch.float32))


class HandState:
    """a GpdState of pitch `ld` built by hand from the inputs (the planes of include/gpd.h), NaN beyond N in every block; `rows`: the
    plant table [19, ld] derived from the scales by gpd_plant_derive, NaN beyond N, or None"""

    def __init__(self, core, inp, N, ld, dev):
        from gym_pybullet_drones_amd import _native
        f32 = dict(dtype=torch.float32, device=dev)
        nan = float("nan")
        planes = torch.full((3, ld, 4), nan, **f32)
        planes[0, :N, :3], planes[0, :N, 3] = torch.as_tensor(inp.pos, device=dev), torch.as_tensor(inp.rates[:, 0], device=dev)
        planes[1, :N] = torch.as_tensor(inp.quat, device=dev)
        planes[2, :N, :3], planes[2, :N, 3] = torch.as_tensor(inp.vel, device=dev), torch.as_tensor(inp.rates[:, 1], device=dev)
        wz = torch.full((ld,), nan, **f32)
        wz[:N] = torch.as_tensor(inp.rates[:, 2], device=dev)
        self.kin = torch.cat([planes.reshape(-1), wz])
        self.pid = torch.full((9, ld), nan, **f32)
        if inp.pid is not None:
            self.pid[:, :N] = torch.as_tensor(inp.pid.T.copy(), device=dev)
        self.last_rpm = torch.full((4, ld), nan, **f32)
        self.last_rpm[:, :N] = torch.as_tensor(inp.last_rpm.T.copy(), device=dev)
        self.counter = torch.zeros((ld,), dtype=torch.int32, device=dev)
        self.ld = ld
        self.struct = _native.GpdState(kin=self.kin.data_ptr(), last_rpm=self.last_rpm.data_ptr(), pid=self.pid.data_ptr(),
                                       step_counter=self.counter.data_ptr(), ld=ld)
        self.rows = None
        if inp.scales is not None:
            scales = torch.ones((9, ld), **f32)
            scales[:, :N] = torch.as_tensor(inp.scales, device=dev)
            self.rows = torch.full((_native.PLANT_ROWS, ld), nan, **f32)
            _native.call("gpd_plant_derive", dev, None, core._params, scales, None, N, 1, ld, self.rows)
            self.rows[:, N:] = nan
        self.parts = [self.kin, self.pid, self.last_rpm, self.counter] + ([] if self.rows is None else [self.rows])

    def snapshot(self):
        return [t.clone() for t in self.parts]

    def unchanged(self, before):
        return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, self.parts))


def mppi_struct(case, inp, **change):
    from gym_pybullet_drones_amd import _native
    F4 = ctypes.c_float * 4
    d = dict(horizon=case.H, samples=case.M, sigma=F4(*inp.sigma), act_lo=F4(*inp.lo), act_hi=F4(*inp.hi), lam=inp.lam, **inp.weights._asdict(),
             seed=(ctypes.c_uint32 * 2)(*inp.seed), iteration=case.iteration)
    d.update(change)
    return _native.GpdMppi(**d)


def entry(core, ctrl, case, inp, state=None, rows=None, own=False, **change):
    """one call -> dict of numpy outputs (the rows beyond N of every output checked against the sentinel).  `state`: a GpdState (None:
    the core's); `rows`: the plant table or None; `own`: the model's OWN entry (gpd_mppi / gpd_mppi_ctbr) on the same tensors"""
    from gym_pybullet_drones_amd import _native
    dev, N, H, M = core.device, case.N, case.H, case.M
    u_in = torch.zeros((H, N + PAD, 4), device=dev)
    u_in[:, :N] = torch.as_tensor(change.pop("u_in", inp.u_in), device=dev)
    g = change.pop("goal", inp.goal)
    goal = torch.zeros((len(g), N + PAD, 4), device=dev)
    goal[:, :N, :3] = torch.as_tensor(g, device=dev)
    u_out = torch.full((H, N + PAD, 4), SENTINEL, device=dev)
    costs, stats = torch.full((N + PAD, M), SENTINEL, device=dev), torch.full((N + PAD, 4), SENTINEL, device=dev)
    if inp.obst is None:
        obst, n_obst, obst_ld = None, 0, 0
    elif len(inp.obst) == 1:
        obst, n_obst, obst_ld = torch.as_tensor(inp.obst[0], device=dev).contiguous(), inp.obst.shape[1], 0
    else:           # per-aviary lists: float f of record r of aviary e at [(r * 8 + f) * ld + e], ld = N + 2
        n_obst, obst_ld = inp.obst.shape[1], N + 2
        obst = torch.full((n_obst * 8, obst_ld), float("nan"), device=dev)
        obst[:, :N] = torch.as_tensor(inp.obst.transpose(1, 2, 0).reshape(n_obst * 8, N), device=dev)
    q = mppi_struct(case, inp, **change)
    state = core._state if state is None else state
    rest = (u_in, (N + PAD) * 4, goal, (N + PAD) * 4 if len(g) > 1 else 0, obst, n_obst, obst_ld, u_out, costs, stats)
    if own:
        lead = (core._params,) if ctrl is None else (core._params, ctrl.struct())
        _native.call("gpd_mppi" if ctrl is None else "gpd_mppi_ctbr", dev, None, *lead, state, core._cfg, q, *rest)
    else:
        _native.call("gpd_mppi_plant", dev, None, core._params, None if ctrl is None else ctrl.struct(), state, core._cfg, q, rows, *rest)
    torch.cuda.synchronize()
    out = dict(u_out=u_out.cpu().numpy(), costs=costs.cpu().numpy(), stats=stats.cpu().numpy())
    assert (out["u_out"][:, N:] == SENTINEL).all() and (out["costs"][N:] == SENTINEL).all() and (out["stats"][N:] == SENTINEL).all()
    return dict(u_out=out["u_out"][:, :N], costs=out["costs"][:N], stats=out["stats"][:N])


@pytest.mark.parametrize("case", yq.CASES, ids=[c.name for c in yq.CASES])
def test_entry_agrees_with_the_yardstick(gpu_device, case):
    """costs, u_out and stats4 within the project's 1e-4 on a state and a table of pitch N + 5 with NaN beyond N; every sample counted;
    the rows beyond N of every output intact; every byte of the state and of the table as it was"""
    inp = yq.make_inputs(case)
    want = yq.plan(case, inp)
    core, ctrl = make_core(case, gpu_device)
    hand = HandState(core, inp, case.N, case.N + 5, gpu_device)
    assert (hand.rows is not None) == case.table
    before = hand.snapshot()
    got = entry(core, ctrl, case, inp, state=hand.struct, rows=hand.rows)
    assert hand.unchanged(before), "the state or the table was written"
    err = {k: float(yq.rel_err(got[k], want[k]).max()) for k in ("costs", "u_out", "stats")}
    print(f"MEASURED {case.name}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"  ess {want['stats'][:, 2].round(1)}")
    assert (got["stats"][:, 3] == case.M).all()
    assert max(err.values()) <= yq.CEILING, err
    assert ((got["u_out"] >= inp.lo[None, None]) & (got["u_out"] <= inp.hi[None, None])).all()


@pytest.mark.parametrize("case", [yq.CASES[3], yq.CASES[5], yq.CASES[9]], ids=lambda c: c.name)
def test_without_flags_the_models_own_entry_bit_for_bit(gpu_device, case):
    """flags 0 and no table, and separately flags 0 and a table of all-ones scales: costs, u_out and stats4 are gpd_mppi's (RPM, VEL)
    or gpd_mppi_ctbr's -- a nominal row holds the nominal struct's bits and the residual it subtracts is +0 (x - (+0) is x) -- and with
    the case's own table the costs are not"""
    inp = yq.make_inputs(case)
    core, ctrl = make_core(case, gpu_device, flags=0)
    set_state(core, inp)
    own = entry(core, ctrl, case, inp, own=True)
    bare = entry(core, ctrl, case, inp)
    core.set_plant(torch.ones((9, case.N), device=gpu_device))
    ones = entry(core, ctrl, case, inp, rows=core.plant_rows)
    for k in ("u_out", "costs", "stats"):
        np.testing.assert_array_equal(bare[k], own[k], err_msg=k)
        np.testing.assert_array_equal(ones[k], own[k], err_msg=k)
    core.set_plant(torch.as_tensor(inp.scales, device=gpu_device))
    assert (entry(core, ctrl, case, inp, rows=core.plant_rows)["costs"] != own["costs"]).mean() > 0.99


def nominal_cost(case, inp, obs):
    """[N]: the cost in float64 of observations obs [H, N, 12] (pos | rpy | vel | ang_v in the world frame) without a list:
    |omega_body| = |omega_world|, R22 = cos(roll) cos(pitch)"""
    w = inp.weights
    S = np.zeros(case.N)
    for h in range(case.H):
        o = obs[h]
        g = inp.goal[h if case.goal_per_step else 0].astype(np.float64)
        S += w.w_pos * (w.w_term if h == case.H - 1 else 1.0) * ((o[:, 0:3] - g) ** 2).sum(-1) + w.w_vel * (o[:, 6:9] ** 2).sum(-1) \
            + w.w_tilt * (1.0 - np.cos(o[:, 3]) * np.cos(o[:, 4])) + w.w_rate * (o[:, 9:12] ** 2).sum(-1)
    return S


@pytest.mark.parametrize("act", ["rpm", "vel", "ctbr"])
def test_costs_are_those_of_the_projects_own_rollout_on_the_ground(gpu_device, act):
    """sigma = 0, H = 4, a perturbed table, GND|DRAG|GROUND|DAMP, six drones that start between 5 mm and 25 cm above the plane, level
    and sinking at 1.5 .. 0.8 m/s (the ground effect alone stops a slower one): some meet the plane within the horizon's 83 ms, some
    do not.  Every sample's cost equals the cost computed in float64 from
    `SimCore.rollout` / `rollout_ctbr` with `set_plant` flying the same clamped nominal -- the same physics code, only the cost's
    summation differs -- within 1e-5 relative.  This is the test that covers the ground plane"""
    case = yq.Case(f"{act}-6-64-h4-s5-none-f27-table", act, 6, 64, 4, 5, "none", False, 0, EVERY, True)
    inp = yq.make_inputs(case)
    z0 = yq.ground_z()
    rng = np.random.default_rng(11)
    pos = inp.pos.copy()
    pos[:, 2] = z0 + np.array([0.005, 0.01, 0.02, 0.06, 0.15, 0.25])
    vel = np.stack([rng.uniform(-0.2, 0.2, case.N), rng.uniform(-0.2, 0.2, case.N), np.linspace(-1.5, -0.8, case.N)], axis=1)
    inp = inp._replace(pos=pos.astype(np.float32), vel=vel.astype(np.float32), quat=np.tile(np.float32([0, 0, 0, 1]), (case.N, 1)),
                       rates=np.zeros((case.N, 3), np.float32), goal=(inp.goal + np.float32([0, 0, 0.25])))
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    core.set_plant(torch.as_tensor(inp.scales, device=gpu_device))
    got = entry(core, ctrl, case, inp, rows=core.plant_rows, sigma=(ctypes.c_float * 4)(0, 0, 0, 0))
    acts = torch.as_tensor(np.clip(inp.u_in, inp.lo, inp.hi), device=gpu_device).contiguous()
    obs = core.rollout(acts)[0] if ctrl is None else core.rollout_ctbr(ctrl, acts, case.H, mode="cmd")
    obs = obs.double().cpu().numpy()
    landed = (np.abs(obs[:, :, 2] - z0) < 1e-6).any(axis=0)
    S = nominal_cost(case, inp, obs)
    err = float((np.abs(got["costs"] - S[:, None]) / np.abs(S[:, None])).max())
    print(f"MEASURED consistency with the project's own rollout on the ground ({act}): {err:.2e}  drones on the plane {landed.astype(int)}")
    assert landed.any() and not landed.all()
    assert (got["costs"] == got["costs"][:, :1]).all(), "sigma 0: every sample flies the nominal"
    assert err < 1e-5


def test_rows_index_by_drone(gpu_device):
    """six drones share one start state and one nominal, sigma 0, six different rows: permuting the table's columns permutes
    costs[:, 0] the same way, bit for bit"""
    case = yq.CASES[2]._replace(table=True)              # (RPM, 6 drones, GND|DRAG)
    inp = yq.make_inputs(case)
    same = lambda v: np.repeat(v[:1], case.N, axis=0)       # noqa: E731
    inp = inp._replace(pos=same(inp.pos), quat=same(inp.quat), vel=same(inp.vel), rates=same(inp.rates), pid=same(inp.pid), last_rpm=same(inp.last_rpm),
                       u_in=np.repeat(inp.u_in[:, 1:2], case.N, axis=1), goal=np.repeat(inp.goal[:, :1], case.N, axis=1), obst=None)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    zero = (ctypes.c_float * 4)(0, 0, 0, 0)
    core.set_plant(torch.as_tensor(inp.scales, device=gpu_device))
    a = entry(core, ctrl, case, inp, rows=core.plant_rows, sigma=zero)["costs"][:, 0]
    perm = np.array([4, 2, 5, 0, 3, 1])
    core.set_plant(torch.as_tensor(inp.scales[:, perm], device=gpu_device))
    b = entry(core, ctrl, case, inp, rows=core.plant_rows, sigma=zero)["costs"][:, 0]
    assert len(set(a.tolist())) == case.N, "six rows, six costs"
    np.testing.assert_array_equal(b, a[perm])


@pytest.mark.parametrize("act", ["vel", "ctbr"])
def test_planner_class_flies_the_cores_model_and_its_own_belief(gpu_device, act):
    """`model="aviary"` is the entry called by hand with the core's flags and table; after `core.set_plant(other)` the next `plan()`
    differs, with `model="nominal"` it does not; `plant=` equal to the core's scales gives the bits of the default aviary model;
    `planner.set_plant` leaves `core.plant_scales` alone"""
    from gym_pybullet_drones_amd import mppi
    case = next(c for c in yq.CASES if c.act == act and c.N == 6 and c.flags)._replace(obst="none", iteration=0, goal_per_step=False)
    inp = yq.make_inputs(case._replace(table=True))
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    scales = torch.as_tensor(inp.scales, device=gpu_device)
    other = scales.flip(1).contiguous()
    core.set_plant(scales)
    kw = dict(cost=mppi.MPPICost(**inp.weights._asdict()), seed=inp.seed[0] | (inp.seed[1] << 32), act_lo=tuple(inp.lo), act_hi=tuple(inp.hi))
    make = (lambda **m: mppi.MPPI(core, case.H, case.M, tuple(inp.sigma), inp.lam, **kw, **m)) if ctrl is None else \
        (lambda **m: mppi.CTBRMPPI(core, ctrl, case.H, case.M, tuple(inp.sigma), inp.lam, **kw, **m))

    def planned(pl):
        pl.nominal[:] = torch.as_tensor(inp.u_in, device=gpu_device)
        pl.iteration = 0
        first = pl.plan(inp.goal[0]).cpu().numpy()
        return first, pl.costs.cpu().numpy().copy(), pl.nominal.cpu().numpy().copy()

    aviary, nominal = make(model="aviary"), make()
    by_hand = entry(core, ctrl, case, inp, rows=core.plant_rows)
    first, costs, u = planned(aviary)
    np.testing.assert_array_equal(costs, by_hand["costs"])
    np.testing.assert_array_equal(u, by_hand["u_out"])
    np.testing.assert_array_equal(first, by_hand["u_out"][0])
    flagless, _ = make_core(case, gpu_device, flags=0)
    set_state(flagless, inp)
    own = entry(flagless, ctrl, case, inp, own=True)
    n_costs = planned(nominal)[1]
    np.testing.assert_array_equal(n_costs, own["costs"])
    belief = make(model="aviary", plant=scales)
    np.testing.assert_array_equal(planned(belief)[1], costs)
    # the core's airframes change: the aviary model follows at the next launch, the nominal model and the belief do not
    core.set_plant(other)
    moved = planned(aviary)[1]
    assert (moved != costs).mean() > 0.99
    np.testing.assert_array_equal(moved, entry(core, ctrl, case, inp, rows=core.plant_rows)["costs"])
    np.testing.assert_array_equal(planned(nominal)[1], n_costs)
    np.testing.assert_array_equal(planned(belief)[1], costs)
    # the belief changes: the core's table does not
    kept = core.plant_scales.clone()
    belief.set_plant(other)
    assert torch.equal(core.plant_scales, kept) and belief.plant_rows.data_ptr() != core.plant_rows.data_ptr()
    np.testing.assert_array_equal(planned(belief)[1], moved)
    belief.set_plant({"mass": 1.1}, mask=torch.tensor([True, False, False, False, False, False]))
    assert float(belief.plant_scales[0, 0]) == np.float32(1.1) and torch.equal(belief.plant_scales[:, 1:case.N], other[:, 1:])
    assert torch.equal(core.plant_scales, kept)


def test_randomized_example_flies_closer_on_the_aviarys_own_model(gpu_device):
    spec = importlib.util.spec_from_file_location("example_mppi_randomized", os.path.join(REPO, "examples", "mppi_randomized.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    nominal, aviary, wrong = mod.run(drones=32, device=gpu_device)
    print(f"MEASURED 32 randomised drones, mean distance to the goal over the last second: model nominal {nominal:.4f} m, "
          f"model aviary {aviary:.4f} m, a wrong belief {wrong:.4f} m")
    assert aviary < nominal and aviary < wrong

"""MPPI over thrust and body-rate commands on the MI355X: `gpd_mppi_ctbr` against the float64 yardstick
(tests/helpers/mppi_ctbr_f64.py, examined without a GPU in tests/test_host_mppi_ctbr.py) over the smallest shapes at which the kernel
takes another path -- a lone wave, a partial block, two blocks; one sample per lane and the sample loop; one step and five; one
sub-step and five; no list, a shared list, per-aviary lists with a skipped record and a floor at a pitch above N; a constant goal and
one per step; two iteration words; bounds inside the controller's clips and beyond them; the three airframes -- then the purity of the
call, its agreement with `gpd_rollout_ctbr`, the `CTBRMPPI` class and `VectorAviary.mppi_ctbr`, and the example.

MEASURED on an MI355X (|x32 - x64| / max(1, |x64|), the largest over the eight cases below; bound 1e-4):
    costs 8.6e-07   u_out 6.8e-07   stats 4.1e-07
Consistency with gpd_rollout_ctbr (relative; bound 1e-5): 7.2e-08, with bounds inside the controller's clips and beyond them.
The example at 128 drones: the blind flight collides for 71.9 %, MPPI for 0.0 % (89.1 % pass x >= +2 m)."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import mppi_ctbr_f64 as yc  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
PAD = 3
MODELS = {"cf2x": "CF2X", "cf2p": "CF2P", "racer": "RACE"}


def make_core(case, dev):
    """(core, ctrl): single drones with DIRECT_RPM actions at 240 / S Hz, and their VectorCTBR"""
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.control import VectorCTBR
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    model = getattr(DroneModel, MODELS[case.model])
    core = engine.SimCore(drone_model=model, num_envs=case.N, drones_per_env=1, physics=0, pyb_freq=240, ctrl_freq=240 // case.S, act_code=6,
                          task=engine.TASK_NONE, auto_reset=False, track_rpm=True, device=dev)
    return core, VectorCTBR(case.N, model, device=dev)


def set_state(core, inp):
    kin = np.concatenate([inp.pos, inp.quat, inp.vel, inp.rates], axis=1).T
    core.set_state(kin=torch.as_tensor(kin, dtype=torch.float32))


def device_table(inp, case, dev):
    """(tensor, n_obst, obst_ld): the shared list [M, 8] at pitch 0, or field planes [M * 8, ld] with ld = N + 5 > N (NaN beyond N)"""
    if inp.obst is None:
        return None, 0, 0
    if case.obst == "shared":
        return torch.as_tensor(inp.obst[0], device=dev).contiguous(), inp.obst.shape[1], 0
    E, M, _ = inp.obst.shape
    ld = E + 5
    t = np.full((M * 8, ld), np.nan, dtype=np.float32)
    t[:, :E] = inp.obst.transpose(1, 2, 0).reshape(M * 8, E)
    return torch.as_tensor(t, device=dev).contiguous(), M, ld


def mppi_struct(case, inp, **change):
    from gym_pybullet_drones_amd import _native
    F4 = ctypes.c_float * 4
    d = dict(horizon=case.H, samples=case.M, sigma=F4(*inp.sigma), act_lo=F4(*inp.lo), act_hi=F4(*inp.hi), lam=inp.lam, **inp.weights._asdict(),
             seed=(ctypes.c_uint32 * 2)(*inp.seed), iteration=case.iteration)
    d.update(change)
    return _native.GpdMppi(**d)


def entry(core, ctrl, case, inp, **change):
    """one call on the core's state -> dict of numpy outputs (the rows beyond N of every output checked against the sentinel)"""
    from gym_pybullet_drones_amd import _native
    dev, N, H, M = core.device, case.N, case.H, case.M
    u_in = torch.zeros((H, N + PAD, 4), device=dev)
    u_in[:, :N] = torch.as_tensor(change.pop("u_in", inp.u_in), device=dev)
    g = inp.goal
    goal = torch.zeros((len(g), N + PAD, 4), device=dev)
    goal[:, :N, :3] = torch.as_tensor(g, device=dev)
    u_out = torch.full((H, N + PAD, 4), SENTINEL, device=dev)
    costs, stats = torch.full((N + PAD, M), SENTINEL, device=dev), torch.full((N + PAD, 4), SENTINEL, device=dev)
    table, n_obst, ld = device_table(inp, case, dev)
    q = mppi_struct(case, inp, **change)
    _native.call("gpd_mppi_ctbr", dev, None, core._params, ctrl.struct(), core._state, core._cfg, q, u_in, (N + PAD) * 4, goal,
                 (N + PAD) * 4 if case.goal_per_step else 0, table, n_obst, ld, u_out, costs, stats)
    torch.cuda.synchronize()
    out = dict(u_out=u_out.cpu().numpy(), costs=costs.cpu().numpy(), stats=stats.cpu().numpy())
    assert (out["u_out"][:, N:] == SENTINEL).all() and (out["costs"][N:] == SENTINEL).all() and (out["stats"][N:] == SENTINEL).all()
    return dict(u_out=out["u_out"][:, :N], costs=out["costs"][:N], stats=out["stats"][:N])


def state_bytes(core):
    parts = [core.kin_store, core.step_counter] + [t for t in (core.pid, core.last_rpm) if t is not None]
    return [t.clone() for t in parts], parts


@pytest.mark.parametrize("case", yc.CASES, ids=[c.name for c in yc.CASES])
def test_entry_agrees_with_the_yardstick(gpu_device, case):
    """costs, u_out and stats4 within the project's 1e-4, nothing left out; the call leaves every byte of GpdState as it was"""
    inp = yc.make_inputs(case)
    want = yc.plan(case, inp)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    before, parts = state_bytes(core)
    got = entry(core, ctrl, case, inp)
    assert all(torch.equal(a, b) for a, b in zip(before, parts)), "the state was written"
    err = {k: float(yc.rel_err(got[k], want[k]).max()) for k in ("costs", "u_out", "stats")}
    print(f"MEASURED {case.name}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"  ess {want['stats'][:, 2].round(1)}")
    assert (got["stats"][:, 3] == case.M).all()
    assert max(err.values()) <= yc.CEILING, err
    lo, hi = inp.lo[None, None], inp.hi[None, None]
    assert ((got["u_out"] >= lo) & (got["u_out"] <= hi)).all()


def test_same_call_same_bits_and_other_noise_other_costs(gpu_device):
    case = yc.CASES[1]
    inp = yc.make_inputs(case)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    a, b = entry(core, ctrl, case, inp), entry(core, ctrl, case, inp)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    other_it = entry(core, ctrl, case, inp, iteration=case.iteration + 1)
    other_seed = entry(core, ctrl, case, inp, seed=(ctypes.c_uint32 * 2)(inp.seed[0] + 1, inp.seed[1]))
    for o in (other_it, other_seed):
        assert (o["costs"] != a["costs"]).mean() > 0.99 and not np.array_equal(o["u_out"], a["u_out"])


@pytest.mark.parametrize("case", [yc.CASES[2], yc.CASES[5]], ids=lambda c: c.name)
def test_without_noise_every_sample_is_the_nominal(gpu_device, case):
    """sigma = 0: u_out is clamp(u_in) bit for bit (the nominal has a row outside the bounds), the M costs of a drone are one value,
    and the effective sample size is M"""
    inp = yc.make_inputs(case)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    got = entry(core, ctrl, case, inp, sigma=(ctypes.c_float * 4)(0, 0, 0, 0))
    np.testing.assert_array_equal(got["u_out"], np.clip(inp.u_in, inp.lo, inp.hi))
    assert (got["costs"] == got["costs"][:, :1]).all()
    np.testing.assert_array_equal(got["stats"][:, 2:], np.full((case.N, 2), case.M, dtype=np.float32))
    np.testing.assert_array_equal(got["stats"][:, 0], got["costs"][:, 0])


@pytest.mark.parametrize("wide", [False, True], ids=["inside", "wide"])
def test_costs_are_those_of_the_projects_own_ctbr_rollout(gpu_device, wide):
    """sigma = 0, H = 4, no obstacles: the samples' cost equals the cost computed in float64 from `gpd_rollout_ctbr`'s observations of
    the same (clamped) nominal flown in "cmd" mode -- the rate loop and the physics are the same code, only the cost's summation
    differs -- within 1e-5 relative.  `wide`: the nominal row beyond thrust_max and rate_max, which the rate loop clips in both."""
    case = yc.Case("cf2x-6-64-h4-s5-none", "cf2x", 6, 64, 4, 5, "none", False, 0, wide)
    inp = yc.make_inputs(case)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    got = entry(core, ctrl, case, inp, sigma=(ctypes.c_float * 4)(0, 0, 0, 0))
    cmds = torch.as_tensor(np.clip(inp.u_in, inp.lo, inp.hi), device=gpu_device).contiguous()
    obs = core.rollout_ctbr(ctrl, cmds, case.H, mode="cmd").double().cpu().numpy()        # [H, N, 12]: pos | rpy | vel | ang_v (world)
    S = yc.nominal_costs(case, inp, obs)
    err = float((np.abs(got["costs"][:, 0] - S) / np.abs(S)).max())
    print(f"MEASURED consistency with gpd_rollout_ctbr ({'wide' if wide else 'inside'}): {err:.2e}")
    assert err < 1e-5


def test_planner_class_runs_the_entry_and_shifts_its_nominal(gpu_device):
    """`CTBRMPPI.plan(goal, iterations=2)` is two calls of the entry by hand (the nominal swapped, the iteration word bumped);
    `advance()` shifts the nominal and repeats its last row; `reset()` writes rows; the defaults are the controller's clips and hover"""
    from gym_pybullet_drones_amd import mppi
    from gym_pybullet_drones_amd.obstacles import ObstacleField
    case = yc.CASES[4]._replace(iteration=0)
    inp = yc.make_inputs(case)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    cost = mppi.MPPICost(**inp.weights._asdict())
    field = ObstacleField()
    for rec in inp.obst[0].astype(np.float64):               # (the sizes a kind does not read are left out: the same distances)
        {yc.obst_y.SPHERE: lambda r: field.sphere(r[0:3], r[4]), yc.obst_y.BOX: lambda r: field.box(r[0:3], r[4:7]),
         yc.obst_y.CYLINDER: lambda r: field.cylinder(r[0:3], r[4], r[6])}[int(rec[3])](rec)
    pl = mppi.CTBRMPPI(core, ctrl, case.H, case.M, tuple(inp.sigma), inp.lam, cost=cost, seed=inp.seed[0] | (inp.seed[1] << 32), field=field,
                       act_lo=tuple(inp.lo), act_hi=tuple(inp.hi))
    assert (pl.nominal.cpu().numpy() == np.float32([ctrl.struct().g, 0, 0, 0])).all()
    pl.nominal[:] = torch.as_tensor(inp.u_in, device=gpu_device)
    first = pl.plan(inp.goal[0], iterations=2)
    one = entry(core, ctrl, case, inp, iteration=0)
    two = entry(core, ctrl, case, inp, iteration=1, u_in=one["u_out"])
    np.testing.assert_array_equal(pl.nominal.cpu().numpy(), two["u_out"])
    np.testing.assert_array_equal(first.cpu().numpy(), two["u_out"][0])
    np.testing.assert_array_equal(pl.costs.cpu().numpy(), two["costs"])
    assert pl.iteration == 2
    before = pl.nominal.clone()
    pl.advance()
    assert torch.equal(pl.nominal[:-1], before[1:]) and torch.equal(pl.nominal[-1], before[-1])
    pl.reset(rows=torch.tensor([1], device=gpu_device), value=(9.0, 0.5, 0.0, -0.25))
    assert (pl.nominal[:, 1].cpu().numpy() == np.float32([9.0, 0.5, 0.0, -0.25])).all() and torch.equal(pl.nominal[:, 0], before[[*range(1, case.H), case.H - 1], 0])
    default = mppi.CTBRMPPI(core, ctrl, case.H, case.M, 1.0, 1.0)
    r = np.float32(ctrl.rate_max)
    assert list(default._q.act_lo) == [0.0, -r, -r, -r] and list(default._q.act_hi) == [np.float32(ctrl.thrust_max), r, r, r]


def test_a_hovering_drone_flown_by_the_planner_approaches_its_goal(gpu_device):
    """40 plan / rollout_ctbr / advance cycles of `VectorAviary.mppi_ctbr` at 48 Hz: the drone ends closer to a goal 0.5 m away than it
    started (a relation, not a number)"""
    from gym_pybullet_drones_amd.control import VectorCTBR
    from gym_pybullet_drones_amd.envs import VectorCtrlAviary
    from gym_pybullet_drones_amd.mppi import MPPICost
    start = np.array([[[0.0, 0.0, 1.0]], [[0.3, -0.2, 0.8]]])
    env = VectorCtrlAviary(2, 1, initial_xyzs=start, pyb_freq=240, ctrl_freq=48, device=gpu_device)
    env.reset()
    ctrl = VectorCTBR(2, device=env.device)
    goal = torch.as_tensor(start[:, 0] + np.array([0.5, 0.0, 0.0]), dtype=torch.float32, device=env.device)
    pl = env.mppi_ctbr(ctrl, 12, 128, sigma=(2.0, 3.0, 3.0, 0.5), lam=0.01, cost=MPPICost(w_pos=1.0, w_vel=0.02, w_tilt=0.1, w_rate=0.001, w_term=5.0), seed=3)
    d0 = (env.core.positions() - goal).norm(dim=1)
    for _ in range(40):
        env.rollout_ctbr(ctrl, pl.plan(goal), 1, mode="cmd", last_only=True)
        pl.advance()
    d1 = (env.core.positions() - goal).norm(dim=1)
    print("distance to the goal:", d0.cpu().numpy(), "->", d1.cpu().numpy(), "ess", pl.stats[:, 2].cpu().numpy())
    assert (d1 < d0).all()
    env.close()


def test_mppi_ctbr_example_collides_less_than_the_blind_flight(gpu_device):
    spec = importlib.util.spec_from_file_location("example_mppi_ctbr", os.path.join(REPO, "examples", "mppi_ctbr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    blind, hit, passed = mod.run(drones=128, device=gpu_device)
    print(f"128 drones: blind {100 * blind:.1f} % collided, MPPI over CTBR commands {100 * hit:.1f} % collided and {100 * passed:.1f} % passed")
    assert 0.0 <= hit < blind <= 1.0

"""MPPI with the peers' paths in the cost on the MI355X: `gpd_mppi_peers` against the float64 yardstick (tests/helpers/mppi_peers_f64.py,
examined without a GPU in tests/test_host_mppi_peers.py) over the smallest shapes at which the kernel takes another path -- a lone wave
with intruder rows, a full block and a block of one wave, three blocks; one sample per lane and the sample loop; one step and five; one
sub-step and five; k = 1, 3, 32 at idx_ld = k + 2; one row set and a padded step stride; RPM, VEL and CTBR; no list and a shared one;
lists with -1 in the middle, the drone's own row, an entry beyond the table, no entry at all, a NaN row -- then: without peers the
model's own entry bit for bit, path_out against the project's own rollouts, repeatability, mirrored peers, the `SwarmMPPI` class and
`VectorAviary.mppi_swarm`, and the example.

MEASURED on an MI355X (|x32 - x64| / max(1, |x64|), the largest over the ten cases below; bound 1e-4):
    costs 9.8e-06   u_out 3.2e-06   stats 1.1e-05   path_out 1.3e-07 (all four on vel-cf2x-5-128-h5-s5-k3)
Without peers, and with w_peer = 0: the bits of gpd_mppi / gpd_mppi_ctbr.  path_out against the project's own rollouts (bound 1e-5): 0,
the same bits, for RPM, VEL and CTBR.  Mirrored peer and goal (bound 1e-4): costs 8.5e-07 (VEL) 2.0e-07 (CTBR), u_out 3.0e-08, path
5.8e-11; the peer term is at least 0.29 / 0.18 of every sample's cost.
The example at 64 drones, 20 s: blind to each other 100.0 % collided (100.0 % at the goal); with the peers' paths in the cost 0.0 %
collided (79.7 % at the goal)."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import mppi_peers_f64 as yp  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
PAD = 3
MODELS = {"cf2x": "CF2X", "cf2p": "CF2P", "racer": "RACE"}
ACT_CODE = {"rpm": 0, "vel": 2, "ctbr": 6}
OUT = ("u_out", "costs", "stats", "path")


def make_core(case, dev):
    """(core, ctrl): single drones of the case's airframe and action type at 240 / S Hz; ctrl: their VectorCTBR (CTBR) or None"""
    from gym_pybullet_drones_amd import engine
    from gym_pybullet_drones_amd.control import VectorCTBR
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    model = getattr(DroneModel, MODELS[case.model])
    core = engine.SimCore(drone_model=model, num_envs=case.N, drones_per_env=1, physics=0, pyb_freq=240, ctrl_freq=240 // case.S,
                          act_code=ACT_CODE[case.act], task=engine.TASK_NONE, auto_reset=False, track_rpm=True, device=dev)
    return core, (VectorCTBR(case.N, model, device=dev) if case.act == "ctbr" else None)


def set_state(core, inp):
    kin = np.concatenate([inp.pos, inp.quat, inp.vel, inp.rates], axis=1).T
    pid = torch.as_tensor(inp.pid.T.copy(), dtype=torch.float32) if core.pid is not None and inp.pid is not None else None
    core.set_state(kin=torch.as_tensor(kin, dtype=torch.float32), pid=pid)


def mppi_struct(case, inp, **change):
    from gym_pybullet_drones_amd import _native
    F4 = ctypes.c_float * 4
    d = dict(horizon=case.H, samples=case.M, sigma=F4(*inp.sigma), act_lo=F4(*inp.lo), act_hi=F4(*inp.hi), lam=inp.lam, **inp.weights._asdict(),
             seed=(ctypes.c_uint32 * 2)(*inp.seed), iteration=case.iteration)
    d.update(change)
    return _native.GpdMppi(**d)


def entry(core, ctrl, case, inp, peers=True, path=True, **change):
    """one call on the core's state -> dict of numpy outputs (the rows beyond N of every output checked against the sentinel).
    `peers` False: the model's OWN entry (gpd_mppi / gpd_mppi_ctbr) on the same tensors.  The table goes to the device as one row set
    (`stride0`) or with a step stride of n_rows + 3 rows (the rows beyond n_rows: a point amid the drones that must not be read)"""
    from gym_pybullet_drones_amd import _native
    dev, N, H, M = core.device, case.N, case.H, case.M
    u_in = torch.zeros((H, N + PAD, 4), device=dev)
    u_in[:, :N] = torch.as_tensor(change.pop("u_in", inp.u_in), device=dev)
    g = change.pop("goal", inp.goal)
    goal = torch.zeros((len(g), N + PAD, 4), device=dev)
    goal[:, :N, :3] = torch.as_tensor(g, device=dev)
    u_out = torch.full((H, N + PAD, 4), SENTINEL, device=dev)
    costs, stats = torch.full((N + PAD, M), SENTINEL, device=dev), torch.full((N + PAD, 4), SENTINEL, device=dev)
    path_out = torch.full((H, N + PAD, 4), SENTINEL, device=dev)
    obst = None if inp.obst is None else torch.as_tensor(inp.obst[0], device=dev).contiguous()
    n_obst = 0 if inp.obst is None else inp.obst.shape[1]
    idx = torch.as_tensor(change.pop("idx", inp.idx), dtype=torch.int32, device=dev).contiguous()
    tab = np.asarray(change.pop("table", inp.table), dtype=np.float32)
    k, w_peer, peer_dist = change.pop("k", case.k), change.pop("w_peer", inp.w_peer), change.pop("peer_dist", inp.peer_dist)
    n_rows = tab.shape[1]
    if len(tab) == 1:
        table, stride = torch.as_tensor(tab[0], device=dev).contiguous(), 0
    else:
        table = torch.zeros((len(tab), n_rows + 3, 4), device=dev)
        table[..., 2] = 0.6
        table[:, :n_rows] = torch.as_tensor(tab, device=dev)
        stride = (n_rows + 3) * 4
    q = mppi_struct(case, inp, **change)
    lead = (core._params,) if ctrl is None else (core._params, ctrl.struct())
    rest = (u_in, (N + PAD) * 4, goal, (N + PAD) * 4 if len(g) > 1 else 0, obst, n_obst, 0, u_out, costs, stats)
    if peers:
        r = _native.GpdMppiPeers(idx=idx.data_ptr(), pos=table.data_ptr(), path_out=path_out.data_ptr() if path else None, pos_step_stride=stride, k=k,
                                 idx_ld=idx.shape[1], n_rows=n_rows, w_peer=w_peer, peer_dist=peer_dist)
        _native.call("gpd_mppi_peers", dev, None, core._params, None if ctrl is None else ctrl.struct(), core._state, core._cfg, q, r, *rest)
    else:
        _native.call("gpd_mppi" if ctrl is None else "gpd_mppi_ctbr", dev, None, *lead, core._state, core._cfg, q, *rest)
    torch.cuda.synchronize()
    out = dict(u_out=u_out.cpu().numpy(), costs=costs.cpu().numpy(), stats=stats.cpu().numpy(), path=path_out.cpu().numpy())
    assert (out["u_out"][:, N:] == SENTINEL).all() and (out["costs"][N:] == SENTINEL).all() and (out["stats"][N:] == SENTINEL).all()
    assert (out["path"][:, N:] == SENTINEL).all() and (peers and path or (out["path"] == SENTINEL).all())
    return dict(u_out=out["u_out"][:, :N], costs=out["costs"][:N], stats=out["stats"][:N], path=out["path"][:, :N])


def state_bytes(core):
    parts = [core.kin_store, core.step_counter] + [t for t in (core.pid, core.last_rpm) if t is not None]
    return [t.clone() for t in parts], parts


@pytest.mark.parametrize("case", yp.CASES, ids=[c.name for c in yp.CASES])
def test_entry_agrees_with_the_yardstick(gpu_device, case):
    """costs, u_out, stats4 and path_out within the project's 1e-4, the rows beyond N intact, every byte of GpdState as it was"""
    inp = yp.make_inputs(case)
    want = yp.plan(case, inp)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    before, parts = state_bytes(core)
    got = entry(core, ctrl, case, inp)
    assert all(torch.equal(a, b) for a, b in zip(before, parts)), "the state was written"
    err = {k: float(yp.rel_err(got[k], want[k]).max()) for k in ("costs", "u_out", "stats")}
    err["path"] = float(yp.path_err(got["path"], want["path"]).max())
    print(f"MEASURED {case.name}: " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"  ess {want['stats'][:, 2].round(1)}")
    assert (got["stats"][:, 3] == case.M).all()
    assert max(err.values()) <= yp.CEILING, err
    assert ((got["u_out"] >= inp.lo[None, None]) & (got["u_out"] <= inp.hi[None, None])).all()


@pytest.mark.parametrize("case", [yp.CASES[3], yp.CASES[1], yp.CASES[2]], ids=lambda c: c.name)
def test_without_peers_the_models_own_entry_bit_for_bit(gpu_device, case):
    """every idx entry -1, and again w_peer = 0 with the real peers (a NaN row among them): u_out, costs and stats4 are gpd_mppi's
    (RPM, VEL) or gpd_mppi_ctbr's -- the same IEEE sequence under -ffp-contract=off, plus `+ 0.0f` -- and with the peers the costs are
    not"""
    inp = yp.make_inputs(case)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    own = entry(core, ctrl, case, inp, peers=False)
    nobody = entry(core, ctrl, case, inp, idx=np.full_like(inp.idx, -1))
    weightless = entry(core, ctrl, case, inp, w_peer=0.0)
    for k in ("u_out", "costs", "stats"):
        np.testing.assert_array_equal(nobody[k], own[k], err_msg=k)
        np.testing.assert_array_equal(weightless[k], own[k], err_msg=k)
    assert np.isinf(nobody["path"][..., 3]).all()
    np.testing.assert_array_equal(nobody["path"][..., :3], weightless["path"][..., :3])
    assert (entry(core, ctrl, case, inp)["costs"] > own["costs"]).mean() > 0.25


@pytest.mark.parametrize("case", [yp.CASES[3], yp.CASES[1], yp.CASES[2]], ids=lambda c: c.name)
def test_path_is_the_projects_own_rollout_of_the_new_nominal(gpu_device, case):
    """x, y, z of path_out against `SimCore.rollout` / `rollout_ctbr(mode="cmd")` flying u_out from the same state: the same device
    code, 1e-5 relative; and without path_out the other outputs are the same bits"""
    inp = yp.make_inputs(case)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    got = entry(core, ctrl, case, inp)
    bare = entry(core, ctrl, case, inp, path=False)
    assert all(np.array_equal(got[k], bare[k]) for k in ("u_out", "costs", "stats"))
    acts = torch.as_tensor(got["u_out"], device=gpu_device).contiguous()
    obs = core.rollout(acts)[0] if ctrl is None else core.rollout_ctbr(ctrl, acts, case.H, mode="cmd")
    pos = obs.double().cpu().numpy()[..., 0:3]
    err = float((np.abs(got["path"][..., :3] - pos) / np.maximum(1.0, np.abs(pos))).max())
    print(f"MEASURED consistency of path_out with the rollout ({case.name}): {err:.2e}")
    assert err < 1e-5


def test_same_call_same_bits(gpu_device):
    case = yp.CASES[2]
    inp = yp.make_inputs(case)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    a, b = entry(core, ctrl, case, inp), entry(core, ctrl, case, inp)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in OUT)
    other = entry(core, ctrl, case, inp, iteration=case.iteration + 1)
    assert (other["costs"] != a["costs"]).mean() > 0.99


@pytest.mark.parametrize("act", ["vel", "ctbr"])
def test_mirrored_peer_and_goal_give_mirrored_costs(gpu_device, act):
    """A level drone at rest; a drifting peer beside it and a goal; then peer and goal mirrored through the drone's start in the
    horizontal plane (x, y -> -x, -y about the start: half a turn about the vertical, under which an X airframe at yaw 0 maps onto
    itself with its rotors swapped in pairs), the nominal's horizontal components negated.  The noise acts on the components the
    mirror leaves alone (sigma 0 on the others), so sample m of one call is the mirror image of sample m of the other: equal costs,
    mirrored u_out and path, within the yardstick's bound.  The peer term is more than 100 times that bound of EVERY sample's cost: an
    error of the term's own size would show"""
    case = yp.Case(f"{act}-mirror", act, "cf2x", 1, 128, 5, 5, 1, 1, "none", False, False, 0)
    inp = yp.make_inputs(case)
    start = np.float32([[0.0, 0.0, 1.0]])
    flip = np.float32([-1.0, -1.0, 1.0])
    sigma = np.float32([0.0, 0.0, 0.3, 0.3] if act == "vel" else [3.0, 0.0, 0.0, 1.5])
    u = np.tile(np.float32([0.5, 0.25, 0.125, 0.5] if act == "vel" else [10.0, 0.5, -0.25, 0.5]), (case.H, 1, 1))
    uflip = np.float32([-1.0, -1.0, 1.0, 1.0] if act == "vel" else [1.0, -1.0, -1.0, 1.0])
    steps = np.arange(1, case.H + 1, dtype=np.float32)[:, None]
    off = np.float32([0.1875, -0.125, 0.0625]) + steps * np.float32([-0.015625, 0.0078125, 0.0])          # the peer relative to the start
    goal_off = np.float32([0.375, 0.25, 0.125])
    inp = inp._replace(pos=start, quat=np.float32([[0, 0, 0, 1]]), vel=np.zeros((1, 3), np.float32), rates=np.zeros((1, 3), np.float32),
                       pid=None if inp.pid is None else np.zeros((1, 9), np.float32), sigma=sigma, idx=np.int32([[1, -1, -1]]))

    def table(sign):
        t = np.zeros((case.H, 2, 4), np.float32)
        t[:, 0, :3] = start
        t[:, 1, :3] = start + off * sign
        return t
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    a = entry(core, ctrl, case, inp, u_in=u, goal=(start + goal_off)[None], table=table(1.0))
    b = entry(core, ctrl, case, inp, u_in=u * uflip, goal=(start + goal_off * flip)[None], table=table(flip))
    alone = entry(core, ctrl, case, inp, u_in=u, goal=(start + goal_off)[None], table=table(1.0), w_peer=0.0)
    share = float(((a["costs"] - alone["costs"]) / a["costs"]).min())
    pa, pb = a["path"], b["path"].copy()
    pb[..., :3] = start + (pb[..., :3] - start) * flip
    err = dict(costs=float(yp.rel_err(b["costs"], a["costs"]).max()), u_out=float(yp.rel_err(b["u_out"] * uflip, a["u_out"]).max()),
               path=float(yp.rel_err(pb, pa).max()))
    print(f"MEASURED mirror ({act}): " + "  ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"  the peer term's least share of a cost {share:.2f}")
    assert share > 100.0 * yp.CEILING
    assert max(err.values()) <= yp.CEILING, err


def test_planner_class_runs_the_entry_and_swaps_its_tables(gpu_device):
    """`SwarmMPPI.plan(goal, iterations=2)` is two calls of the entry by hand: the lists of one neighbour search, the first table by
    constant velocity from the state, the second the first call's path_out; `advance()` shifts nominal and paths; `reset()` forgets the
    paths; the defaults"""
    from gym_pybullet_drones_amd import mppi
    from gym_pybullet_drones_amd.obstacles import ObstacleField
    case = yp.CASES[1]._replace(iteration=0)
    inp = yp.make_inputs(case)
    core, ctrl = make_core(case, gpu_device)
    set_state(core, inp)
    cost = mppi.MPPICost(**inp.weights._asdict())
    field = ObstacleField()
    for rec in inp.obst[0].astype(np.float64):               # (the sizes a kind does not read are left out: the same distances)
        {yp.obst_y.SPHERE: lambda r: field.sphere(r[0:3], r[4]), yp.obst_y.BOX: lambda r: field.box(r[0:3], r[4:7]),
         yp.obst_y.CYLINDER: lambda r: field.cylinder(r[0:3], r[4], r[6])}[int(rec[3])](rec)
    pl = mppi.SwarmMPPI(core, case.H, case.M, tuple(inp.sigma), inp.lam, cost=cost, seed=inp.seed[0] | (inp.seed[1] << 32), field=field, k=case.k,
                        radius=0.45, w_peer=inp.w_peer, peer_dist=inp.peer_dist, act_lo=tuple(inp.lo), act_hi=tuple(inp.hi))
    assert (pl.nominal.cpu().numpy() == np.float32([1, 0, 0, 0])).all() and torch.isnan(pl._paths[0]).all()
    pl.nominal[:] = torch.as_tensor(inp.u_in, device=gpu_device)
    goal = inp.goal[0]
    first = pl.plan(goal, iterations=2)
    idx = pl.search.out.idx.cpu().numpy()
    d = np.linalg.norm(inp.pos[:, None] - inp.pos[None], axis=-1)
    assert ((idx >= 0).sum(axis=1) == np.minimum(case.k, (d < 0.45).sum(axis=1) - 1)).all() and (idx >= 0).any() and (idx < 0).any()
    steps = torch.arange(1, case.H + 1, dtype=torch.float32, device=gpu_device)[:, None, None] * core._cfg.ctrl_dt
    table = torch.zeros((case.H, case.N, 4), device=gpu_device)
    table[..., :3] = core.kin_P[None, :case.N, :3] + steps * core.kin_V[None, :case.N, :3]
    one = entry(core, ctrl, case, inp, iteration=0, goal=goal[None], idx=idx, table=table.cpu().numpy())
    two = entry(core, ctrl, case, inp, iteration=1, goal=goal[None], idx=idx, table=one["path"], u_in=one["u_out"])
    np.testing.assert_array_equal(pl.nominal.cpu().numpy(), two["u_out"])
    np.testing.assert_array_equal(first.cpu().numpy(), two["u_out"][0])
    np.testing.assert_array_equal(pl.costs.cpu().numpy(), two["costs"])
    np.testing.assert_array_equal(pl.paths.cpu().numpy(), two["path"])
    np.testing.assert_array_equal(pl.min_separation.cpu().numpy(), two["path"][..., 3].min(axis=0))
    assert pl.iteration == 2 and (one["path"] != two["path"]).any()
    nominal, paths = pl.nominal.clone(), pl.paths.clone()
    pl.advance()
    shifted = [*range(1, case.H), case.H - 1]
    assert torch.equal(pl.nominal, nominal[shifted]) and torch.equal(pl.paths, paths[shifted])
    pl.reset()
    assert (pl.nominal.cpu().numpy() == np.float32([1, 0, 0, 0])).all() and not pl._published
    pl.nominal[:] = torch.as_tensor(inp.u_in, device=gpu_device)
    pl.iteration = 0
    pl.plan(goal)
    np.testing.assert_array_equal(pl.paths.cpu().numpy(), one["path"])
    default = mppi.SwarmMPPI(core, 24, 64, 1.0, 1.0)
    assert default.peer_dist == 2.0 * core.P.COLLISION_R + 0.3 and default.k == 8 and default.w_peer == 100.0
    assert default.radius == pytest.approx(default.peer_dist + 2.0 * core.P.SPEED_LIMIT * 24 * core._cfg.ctrl_dt)
    assert list(default._q.act_lo) == [-1.0, -1.0, -1.0, 0.0]


def test_intruders_are_counted_by_every_drone_and_vector_aviary_binds_the_planner(gpu_device):
    """`VectorAviary.mppi_swarm` on two distant drones with one intruder row: before its path is given the row is NaN and nobody has a
    peer; given a path beside drone 1, that drone's separation is the distance to it and its plan costs more"""
    from gym_pybullet_drones_amd import mppi
    from gym_pybullet_drones_amd.envs import VectorVelocityAviary
    start = np.array([[[0.0, 0.0, 1.0]], [[5.0, 0.0, 1.0]]])
    env = VectorVelocityAviary(2, 1, initial_xyzs=start, pyb_freq=240, ctrl_freq=48, device=gpu_device)
    env.reset()
    pl = env.mppi_swarm(6, 64, sigma=(0.3, 0.3, 0.2, 0.3), lam=0.05, k=1, radius=1.0, intruders=1, seed=5)
    assert isinstance(pl, mppi.SwarmMPPI) and pl.nominal.shape == (6, 2, 4) and pl._r.k == 2
    goal = torch.as_tensor(start[:, 0], dtype=torch.float32, device=env.device)
    assert pl.plan(goal).shape == (2, 4) and torch.isinf(pl.min_separation).all()
    alone = pl.costs.clone()
    pl.reset()
    pl.iteration = 0
    beside = torch.tensor([5.0, 0.25, 1.0], device=env.device).expand(6, 1, 3)
    pl.plan(goal, intruder_paths=beside)
    sep = pl.min_separation.cpu().numpy()
    print("separation from the intruder:", sep)
    assert sep[0] > 4.0 and 0.1 < sep[1] < 0.3
    assert torch.equal(pl.costs[0], alone[0]) and (pl.costs[1] > alone[1]).all()
    env.close()


def test_swarm_example_collides_less_than_the_flight_blind_to_the_peers(gpu_device):
    spec = importlib.util.spec_from_file_location("example_mppi_swarm", os.path.join(REPO, "examples", "mppi_swarm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hit_blind, goal_blind, hit_swarm, goal_swarm = mod.run(drones=64, device=gpu_device)
    print(f"MEASURED 64 drones across the circle: blind {100 * hit_blind:.1f} % collided ({100 * goal_blind:.1f} % at the goal), "
          f"with the peers' paths {100 * hit_swarm:.1f} % collided ({100 * goal_swarm:.1f} % at the goal)")
    assert 0.0 <= hit_swarm < hit_blind <= 1.0

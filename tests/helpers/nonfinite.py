"""Drones that are not finite, what tests/test_gpu_nonfinite.py flies on the device and tests/test_host_nonfinite.py examines without one:
(1) the MPPI setups of all four planners with three of six start states poisoned, (2) the "hard wall" plans in which about half of a
drone's samples overflow float32, with the conditions the device comparison relies on, (3) the obstacle-task scenes with poisoned poses
and actions, (4) the poisoned kinematic states of the guard-byte test.  The yardsticks are those of mppi_f64 / mppi_ctbr_f64 /
mppi_peers_f64 / mppi_plant_f64 and obst_task_f64; nothing here touches their CASES.  Test infrastructure."""
import collections
import functools

import numpy as np

import mppi_ctbr_f64 as yc
import mppi_f64 as y
import mppi_peers_f64 as yp
import mppi_plant_f64 as yq
import obst_task_f64 as yo
import obstacles_f64 as obst_y

CEILING = y.CEILING
rel_err = y.rel_err
FLT_MAX = float(np.finfo(np.float32).max)
NAN, INF = float("nan"), float("inf")

# ---- 1. MPPI: drones without a finite sample -----------------------------------------------------------------------------------------------
#: six drones = two workgroups of four waves, the second ragged; the sample loop (3 batches); five steps of five sub-steps
N, M, H, S = 6, 192, 5, 5
#: drone 1: NaN in the quaternion; drone 3 (a workgroup shared with the clean 0 and 2): +inf in a velocity; drone 4 (the ragged
#: workgroup): -inf in z
POISONED, CLEAN = (1, 3, 4), (0, 2, 5)

Setup = collections.namedtuple("Setup", "entry case")
SETUPS = (
    Setup("mppi", y.Case("nonfinite-rpm", N, M, H, S, "rpm", "lists", True, 7)),
    Setup("mppi", y.Case("nonfinite-vel", N, M, H, S, "vel", "shared", False, 7)),
    Setup("ctbr", yc.Case("nonfinite-ctbr", "cf2x", N, M, H, S, "lists", True, 7, True)),
    Setup("peers", yp.Case("nonfinite-peers-rpm", "rpm", "cf2x", N, M, H, S, 3, 1, "shared", False, True, 7)),
    Setup("peers", yp.Case("nonfinite-peers-vel", "vel", "cf2x", N, M, H, S, 3, 1, "none", False, False, 7)),
    Setup("peers", yp.Case("nonfinite-peers-ctbr", "ctbr", "cf2x", N, M, H, S, 3, 1, "shared", True, True, 7)),
    # (no GPD_PHYS_GROUND here: the plane catches a drone at z = -inf in its first sub-step -- GROUNDED below flies that)
    Setup("plant", yq.Case("nonfinite-plant-rpm", "rpm", N, M, H, S, "shared", True, 7, yq.GND | yq.DRAG | yq.DAMP, True, 0.5)),
    Setup("plant", yq.Case("nonfinite-plant-vel", "vel", N, M, H, S, "lists", False, 7, yq.GND | yq.DRAG, True, 1.0)),
    Setup("plant", yq.Case("nonfinite-plant-ctbr", "ctbr", N, M, H, S, "none", True, 7, yq.GND | yq.DRAG | yq.DAMP, False, 0.5)),
)
#: the plant setups under the ground plane as well: drone 4 (z = -inf) is put on the plane and plans like any other drone
GROUNDED = ("nonfinite-plant-rpm", "nonfinite-plant-ctbr")
#: a height below every plane that float32 still adds a step to without a change
FAR_BELOW = -1e30
SETUP_IDS = [s.case.name for s in SETUPS]
YARDSTICK = {"mppi": y, "ctbr": yc, "peers": yp, "plant": yq}


def clean_inputs(setup):
    """the setup's inputs with every start state finite: those of the entry's own `make_inputs`, and -- besides the row of drone 0
    that `make_inputs` puts outside the bounds -- that row in the nominal of the drones 1 (step 0) and 4 (the last step), so that
    clamp(u_in) of a poisoned drone is not u_in.  Peers: the rows 1, 3, 4 are taken out of every CLEAN drone's index list (what is
    left: the other clean drones and the intruder row, in a random order; drone 2 keeps an entry naming itself), so that a clean
    drone's cost does not read them: with w_peer as it is, its outputs cannot depend on what those rows hold"""
    inp = YARDSTICK[setup.entry].make_inputs(setup.case)
    u_in = inp.u_in.copy()
    u_in[0, 1] = u_in[0, 0]
    u_in[H - 1, 4] = u_in[0, 0]
    inp = inp._replace(u_in=u_in)
    if setup.entry == "peers":
        rng = np.random.default_rng(5)
        idx = inp.idx.copy()
        n_rows = inp.table.shape[1]
        for n in CLEAN:
            allowed = [r for r in range(n_rows) if r != n and r not in POISONED]
            idx[n, :] = -1
            idx[n, :len(allowed)] = rng.permutation(allowed)
        idx[2, 0] = 2
        inp = inp._replace(idx=idx)
    return inp


def poisoned_inputs(setup, inp=None):
    """the clean inputs with the start states of POISONED made non-finite; peers: their rows of the table too (what such a drone
    would have published)"""
    inp = clean_inputs(setup) if inp is None else inp
    pos, quat, vel = inp.pos.copy(), inp.quat.copy(), inp.vel.copy()
    quat[1, 2] = NAN
    vel[3, 0] = INF
    pos[4, 2] = -INF
    inp = inp._replace(pos=pos, quat=quat, vel=vel)
    if setup.entry == "peers":
        table = inp.table.copy()
        table[:, 1, :] = NAN
        table[:, 3, 0] = INF
        table[:, 4, 2] = -INF
        inp = inp._replace(table=table)
    return inp


@functools.lru_cache(maxsize=None)
def clean_plan(name):
    """(setup, clean inputs, the yardstick's plan of them), once per session; left unchanged by its users"""
    setup = SETUPS[SETUP_IDS.index(name)]
    inp = clean_inputs(setup)
    return setup, inp, YARDSTICK[setup.entry].plan(setup.case, inp)


# ---- 2. MPPI: w_obs as a hard wall, about half of a drone's samples overflow float32 -------------------------------------------------------
#: one step of 48 sub-steps (5 Hz): the samples of a drone spread far enough in height that few of them sit at the threshold
WALL_N, WALL_M, WALL_H, WALL_S = 3, 192, 1, 48
W_OBS, OBST_MARGIN = 3e38, 2.0
#: at most this share of a drone's samples within a relative CEILING of FLT_MAX, at least this share in either class
BAND_CAP, CLASS_SHARE = 0.10, 0.25
WALLS = (Setup("mppi", y.Case("wall-rpm", WALL_N, WALL_M, WALL_H, WALL_S, "rpm", "lists", False, 0)),
         Setup("ctbr", yc.Case("wall-ctbr", "cf2x", WALL_N, WALL_M, WALL_H, WALL_S, "lists", False, 0, False)))
WALL_IDS = [s.case.name for s in WALLS]


def _costs(setup, inp, a):
    S = YARDSTICK[setup.entry].rollout_costs(setup.case, inp, a)
    return S[0] if isinstance(S, tuple) else S


def _floor(z):
    """[N, 1, 8]: per aviary one FLOOR record at the height z[n]"""
    rec = np.zeros((len(z), 1, 8), dtype=np.float32)
    rec[:, 0, 2], rec[:, 0, 3] = z, obst_y.FLOOR
    return rec


@functools.lru_cache(maxsize=None)
def wall_plan(name):
    """(setup, inputs, plan) of a wall case.  The list of aviary n is ONE floor; w_obs = 3e38 and obst_margin = 2 make
    the hinge term w_obs (2.06 - (z - floor))^2 exceed FLT_MAX for a sample that ends within ~0.995 m of it.  The floor of each
    aviary is put where that threshold falls into the WIDEST GAP between two neighbouring end heights of its samples among the middle
    half of them (the heights read off a probe run of the yardstick whose only cost term is the distance to a floor at 0), so that
    at least a quarter of the samples lie on either side and as few as possible at the threshold; lambda is the standard deviation of
    the finite costs (of the first drone), so the weights are neither all equal nor one sample's alone.  test_host_nonfinite.py checks
    all of that on the yardstick."""
    setup = WALLS[WALL_IDS.index(name)]
    case = setup.case
    yy = YARDSTICK[setup.entry]
    base = yy.make_inputs(case)
    lo, hi = base.lo.astype(np.float64), base.hi.astype(np.float64)
    a = y.perturbed(base.u_in, base.sigma, lo, hi, case.M, case.iteration, base.seed)
    f32 = lambda v: float(np.float32(v))       # noqa: E731
    r = base.weights.collision_radius
    probe = base._replace(obst=_floor(np.zeros(case.N)), weights=y.Weights(0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 10.0, r))
    z_end = (10.0 + r) - np.sqrt(_costs(setup, probe, a))                           # [N, M]: the height every sample ends at
    weights = base.weights._replace(w_obs=f32(W_OBS), obst_margin=f32(OBST_MARGIN))
    reach = (weights.obst_margin + r) - np.sqrt(FLT_MAX / weights.w_obs)            # overflow: z - floor < reach
    floor = np.empty(case.N)
    for n in range(case.N):
        z = np.sort(z_end[n])
        q = case.M // 4
        gaps = np.diff(z[q:case.M - q])
        i = q + int(gaps.argmax())
        floor[n] = 0.5 * (z[i] + z[i + 1]) - reach
    inp = base._replace(obst=_floor(floor), weights=weights)
    S = _costs(setup, inp, a)
    fin = S <= FLT_MAX
    inp = inp._replace(lam=f32(S[0][fin[0]].std()))
    u_out, stats = y.update(inp.u_in, a, np.where(fin, S, np.inf), inp.lam, lo, hi)
    return setup, inp, dict(a=a, costs=S, u_out=u_out, stats=stats)


def wall_classes(S):
    """(overflow [N, M], band [N, M]) of float64 costs: beyond FLT_MAX, and within a relative CEILING of it (either class there)"""
    S = np.asarray(S, dtype=np.float64)
    return S > FLT_MAX, np.abs(S - FLT_MAX) <= CEILING * FLT_MAX


# ---- 3. gpd_rollout_obst: poses that are not finite ----------------------------------------------------------------------------------------
OBST_SCENES = ("rpm_shared65_r16_world", "vel_lists_r64_body", "rpm_shared1_r0")
#: the values the poisoned start states hold, in turn: z = -inf (above a floor: clearance -inf and a contact without the guard),
#: x = +inf (a ray from there can return -inf), a NaN quaternion component
Poison = collections.namedtuple("Poison", "start action")


def obst_case(name):
    return next(c for c in yo.CASES if c.name == name)


def obst_scene(name, poisoned=True):
    """(case, scene, Poison): the scene of obst_task_f64 -- with a floor added to the one-record list of rpm_shared1_r0 -- and, when
    `poisoned`, drone 3 (whose step counter make_core lets run out: under the hover task it is reset inside the flight), drone 5,
    drone 64 and the last drone not finite in the start state; in the RPM scenes two more drones receive a NaN and a +inf action at
    step 1.  Drone 5 starts at z = -inf: without the ground plane it stays there (and so does drone 3); with GPD_PHYS_GROUND the plane
    catches it in the first sub-step -- it ends the step finite, lying on the plane below the floor record, in contact -- so there
    drone 3 carries a NaN vertical velocity instead, which nothing heals before its clock runs out"""
    case = obst_case(name)
    sc = yo.scene(case)
    if sc.n_obst == 1:                 # one sphere: add a floor 0.4 m below the course, as the longer lists have one
        table = np.concatenate([sc.table, np.float32([yo.record(yo.FLOOR, (0.0, 0.0, 0.6))])])
        sc = sc._replace(table=table, n_obst=2, records=None)
    kinds = sc.table[:, 3] if sc.obst_ld == 1 else sc.table.reshape(sc.n_obst, 8, -1)[:, 3, :case.N]
    assert (kinds == yo.FLOOR).any(axis=0).all(), "every list holds a floor"
    grounded = bool(case.flags & yo.GROUND)
    start = {3: "vz" if grounded else "pz", 5: "pz", 64: "px", case.N - 1: "q"}
    action = {10: NAN, 130 if case.N > 130 else 40: INF} if case.act == "rpm" else {}
    if not poisoned:
        return case, sc, Poison({}, {})
    kin, actions = sc.kin.copy(), sc.actions.copy()
    kin[2, 5] = -INF                    # rows of kin [13, N]: pos 0..2, quat 3..6, vel 7..9, body rates 10..12
    if grounded:
        kin[9, 3] = NAN
    else:
        kin[2, 3] = -INF
    kin[0, 64] = INF
    kin[4, case.N - 1] = NAN
    for n, v in action.items():
        actions[1, n, 0 if np.isnan(v) else 2] = v
    return case, sc._replace(kin=kin, actions=actions), Poison(start, action)


# ---- 4. the guard byte ---------------------------------------------------------------------------------------------------------------------
GUARD_N, GUARD_K = 300, 4
#: drone -> (row of kin [13, N], value): the first and last lane of a wave, of a workgroup, of the ragged workgroup, and one in between
GUARD_POISON = {0: (4, NAN), 63: (7, INF), 64: (9, -INF), 255: (0, INF), 256: (2, -INF), 299: (11, NAN), 150: (6, NAN)}


def guard_kin(seed=3):
    """(clean, poisoned) kin [13, N] float32: hovering starts near (0, 0, 1), slightly tilted, moving and turning"""
    rng = np.random.default_rng(seed)
    n = GUARD_N
    pos = rng.uniform([-0.3, -0.3, 0.8], [0.3, 0.3, 1.2], size=(n, 3))
    quat = yo.rpy_to_quat(rng.uniform(-0.1, 0.1, size=(n, 3)))
    kin = np.concatenate([pos, quat, rng.uniform(-0.2, 0.2, size=(n, 3)), rng.uniform(-0.3, 0.3, size=(n, 3))], axis=1).T.astype(np.float32)
    bad = kin.copy()
    for d, (row, v) in GUARD_POISON.items():
        bad[row, d] = v
    return kin, bad

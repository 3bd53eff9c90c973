"""Obstacle queries at degenerate geometry on the MI355X: `gpd_obstacles` and the fused `gpd_rollout_obst` on the scenes of
tests/helpers/obstacles_edges.py -- dyadic lattice points ON faces, edges, corners, axes, rims and centres, both zeros, a corridor
whose centre line is exactly as far from a wall as from its mirror image, duplicated records, skipped records, points and rays exactly
at `radius` and `max_range` -- under axis-parallel rays.  Nothing is left out of a comparison here: `nearest`, `hit` and `ray_hit` are
the float64 yardstick's at EVERY point and ray (a tie names the lower record), the class of every distance and range (negative / 0 /
positive / the cap) is identical, no NaN, rows beyond n keep their sentinel, and values agree within 1e-6 (obstacles_edges.BOUND: on
dyadic inputs every product and sum is exact, what remains is a square root, a division and a product).  The C text behind the
kernels passes the same comparison on the host (tests/test_host_obstacles.py).  Only the fans of non-axis rays from the shifted
lattice go through the grazing rule of tests/test_gpu_obstacles.py, with its bound.

The LEVEL frame at identity attitude gives the WORLD answers bit for bit: quat_to_rpy's yaw of (0, 0, 0, w) is atan2(0, w^2) = 0
whatever the reciprocal square root of w^2 rounds to, and sin 0 = 0, cos 0 = 1 leave the table's directions as they are.

MEASURED on an MI355X (|x32 - x64| / max(1, |x64|), the largest over the cases below; bound 1e-6 but for the fans, 1e-4):
    gpd_obstacles      d 5.3e-08   normal 1.0e-07   ranges 3.6e-08
    gpd_rollout_obst   d 5.3e-08   normal 7.2e-08   ranges 2.4e-08      (128 launches: 8 ray counts x 4 lists x 2 sizes x 2 list paths)
    fans (non-axis)    d 1.0e-07   normal 8.3e-07   ranges 1.4e-06
The first two are the figures of the host-compiled text on the same scenes (d 5.3e-08, normal 1.0e-07, ranges 2.4e-08)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import obstacles_edges as ed  # noqa: E402
import obstacles_f64 as y  # noqa: E402
from test_gpu_obstacles import device_table, query  # noqa: E402

pytestmark = pytest.mark.gpu

#: the largest errors seen so far in this session, per entry: printed by every test that adds to them
WORST = {}


def record(entry, name, err_d, err_n, err_r, bound=ed.BOUND):
    w = WORST.setdefault(entry, [0.0, 0.0, 0.0])
    w[:] = [max(a, b) for a, b in zip(w, (err_d, err_n, err_r))]
    print(f"MEASURED {entry} {name}: d {err_d:.3e} normal {err_n:.3e} ranges {err_r:.3e} (so far: d {w[0]:.3e} normal {w[1]:.3e} ranges {w[2]:.3e})")
    assert max(err_d, err_n, err_r) <= bound, name


def ask(dev, lists, shared, pos, D, dirs, frame=0, quat=None, **kw):
    """`gpd_obstacles` on one shared list (`lists` [M, 8]) or on field planes (`lists` [E, M, 8], a pitch above E) -> numpy outputs"""
    lists = lists[None] if shared else lists
    ld = 1 if shared else len(lists) + 5
    return query(dev, pos, quat, D, device_table(lists, shared, ld, dev), lists.shape[1], ld, dirs, frame, **kw)


# ---- gpd_obstacles: the list in LDS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (0, 1), ids=("one-world", "aviaries-of-one"))
@pytest.mark.parametrize("name", list(ed.scenes()))
def test_shared_list_on_degenerate_scenes_with_no_exclusion(gpu_device, name, D):
    s, dirs = ed.scenes()[name], ed.axis_dirs()
    assert len(s.pos) % 64 != 0
    got = ask(gpu_device, s.obst, True, s.pos, D, dirs)
    record("gpd_obstacles", f"shared {name} D={D}", *ed.compare_all(got, s.obst, s.pos, ed.per_point(dirs, len(s.pos))))
    assert (got["ray_hit"] >= 0).any() and (got["ray_hit"] < 0).any() and (got["ranges"] == 0).any() == name.startswith("lattice")


# ---- gpd_obstacles: field planes -------------------------------------------------------------------------------------------------------------
#: (scene, drones per aviary, every aviary's record order rotated by its index?)
PLANES = [("lattice", 1, False), ("lattice-none", 1, True), ("lattice-twins", 1, True), ("corridor", 1, True), ("lattice", 3, False),
          ("lattice-twins", 3, True)]


@pytest.mark.parametrize("name,D,rotate", PLANES, ids=[f"{n}-D{d}-{'rotated' if r else 'same'}" for n, d, r in PLANES])
def test_per_aviary_lists_on_degenerate_scenes_with_no_exclusion(gpu_device, name, D, rotate):
    s, dirs = ed.scenes()[name], ed.axis_dirs()
    n = len(s.pos)
    assert n % D == 0
    E = n // D
    lists = ed.rotated(s.obst, E) if rotate else np.ascontiguousarray(np.broadcast_to(s.obst, (E,) + s.obst.shape))
    if rotate and E >= 64:                                       # the 64 lanes of a wave hold different kinds at the same m
        assert len(set(lists[:64, 0, 3])) >= 3
    got = ask(gpu_device, lists, False, s.pos, D, dirs)
    record("gpd_obstacles", f"planes {name} D={D} rotated={rotate}", *ed.compare_all(got, lists[np.arange(n) // D], s.pos, ed.per_point(dirs, n)))


# ---- the frames --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", (True, False), ids=("shared", "planes"))
def test_body_frame_at_half_turns_gives_the_world_answers_of_the_flipped_table(gpu_device, shared):
    """identity and the half turns about x, y and z, each also with |q| = 2 and 0.5: the rotation matrices are exact sign flips, so the
    answers are those of the WORLD frame for the table with those signs -- the yardstick's everywhere, and the device's own"""
    s, dirs = ed.lattice(), ed.axis_dirs()
    n = len(s.pos)
    quats = np.array([np.array(q) * k for q, _ in ed.HALF_TURNS for k in ed.SCALES], dtype=np.float32)
    signs = np.array([sg for _, sg in ed.HALF_TURNS for _ in ed.SCALES], dtype=np.float32)
    which = np.arange(n) % len(quats)
    lists = s.obst if shared else ed.rotated(s.obst, n)
    per_row = s.obst if shared else lists
    got = ask(gpu_device, lists, shared, s.pos, 1, dirs, frame=2, quat=quats[which])
    world_dirs = dirs[None] * signs[which][:, None, :]
    np.testing.assert_array_equal(y.rotate(dirs, quats[which], 2), world_dirs)            # (the yardstick's matrices are exact too)
    record("gpd_obstacles", f"body frame shared={shared}", *ed.compare_all(got, per_row, s.pos, world_dirs))
    for sg in np.unique(signs, axis=0):
        rows = (signs[which] == sg).all(axis=1)
        world = ask(gpu_device, lists, shared, s.pos, 1, np.ascontiguousarray(dirs * sg), want=("ranges", "ray_hit"))
        np.testing.assert_array_equal(got["ray_hit"][rows], world["ray_hit"][rows])
        np.testing.assert_array_equal(ed.classes(got["ranges"][rows], y.MAX_RANGE), ed.classes(world["ranges"][rows], y.MAX_RANGE))
        assert y.rel_err(got["ranges"][rows], world["ranges"][rows]).max() <= ed.BOUND


def test_level_frame_at_identity_attitude_gives_the_world_answers(gpu_device):
    s, dirs = ed.lattice(), ed.axis_dirs()
    n = len(s.pos)
    quat = np.zeros((n, 4), dtype=np.float32)
    quat[:, 3] = np.array(ed.SCALES, dtype=np.float32)[np.arange(n) % 3]
    got = ask(gpu_device, s.obst, True, s.pos, 1, dirs, frame=1, quat=quat)
    record("gpd_obstacles", "level frame", *ed.compare_all(got, s.obst, s.pos, ed.per_point(dirs, n)))
    world = ask(gpu_device, s.obst, True, s.pos, 1, dirs, want=("ranges", "ray_hit"))
    for k in ("ranges", "ray_hit"):
        np.testing.assert_array_equal(got[k].view(np.uint32), world[k].view(np.uint32), err_msg=k)


# ---- exactly at the radius, exactly at max_range -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", (True, False), ids=("shared", "planes"))
def test_thresholds_are_strict(gpu_device, shared):
    """a point exactly `radius` outside a sphere, a box face, a cylinder's wall, its cap and the floor is no hit; one ulp nearer, or with
    a radius one ulp larger, it is.  An axis ray that enters at exactly max_range reports max_range and -1; with max_range one ulp
    larger it reports the record"""
    obst, cases = ed.thresholds()
    pts, org, dirs = ed.threshold_points(), ed.threshold_origins(), ed.axis_dirs()
    lists = (lambda n: obst) if shared else (lambda n: ed.rotated(obst, n))
    first = (lambda n: np.zeros(n, dtype=int)) if shared else (lambda n: np.arange(n))     # where record 0 sits in row i's list
    M = len(obst)
    for radius, hits in ((np.float32(ed.RADIUS), [0] * 5 + [1] * 5), (ed.up(ed.RADIUS), [1] * 10)):
        got = ask(gpu_device, lists(10), shared, pts, 1, dirs, radius=float(radius))
        assert list(got["hit"]) == hits
        assert list((got["nearest"] + first(10)) % M) == [k.record for k in cases] * 2
        assert list(got["clear4"][:5, 3]) == [ed.RADIUS] * 5 and (got["clear4"][5:, 3] < ed.RADIUS).all()
        record("gpd_obstacles", f"radius {radius!r} shared={shared}", *ed.compare_all(got, lists(10), pts, ed.per_point(dirs, 10), radius=float(radius)))
    for max_range, seen in ((np.float32(ed.RANGE), False), (ed.up(ed.RANGE), True)):
        got = ask(gpu_device, lists(5), shared, org, 1, dirs, max_range=float(max_range))
        for i, k in enumerate(cases):
            assert got["ranges"][i, k.ray] == (ed.RANGE if seen else max_range), k.name
            assert got["ray_hit"][i, k.ray] == ((k.record - first(5)[i]) % M if seen else -1), k.name
        record("gpd_obstacles", f"max_range {max_range!r} shared={shared}", *ed.compare_all(got, lists(5), org, ed.per_point(dirs, 5), max_range=float(max_range)))


# ---- non-axis rays: off the lattice, under the grazing rule -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fan", ("circle-16", "down-5"))
def test_fans_in_the_level_frame_from_the_shifted_lattice(gpu_device, fan):
    """fan(16, 2 pi) and fan(5, pi / 2, elevation -0.5) at 37 yaws from the lattice moved by obstacles_edges.SHIFT, compared as
    tests/test_gpu_obstacles.py compares (tests/test_host_obstacles.py holds the caps on what that leaves out)"""
    from gym_pybullet_drones_amd import obstacles as ob
    table = ob.fan(16, 2 * math.pi) if fan == "circle-16" else ob.fan(5, math.pi / 2, -0.5)
    obst = ed.lattice().obst
    pos, quat = ed.shifted_lattice()
    for shared in (True, False):
        lists = obst if shared else ed.rotated(obst, len(pos))
        got = ask(gpu_device, lists, shared, pos, 1, table, frame=1, quat=quat)
        world_dirs = y.rotate(table, quat, 1)
        err_d, err_n = y.compare_clearance(got, lists, pos)
        err_r = y.compare_scan(got, lists, pos, world_dirs)
        record("fans", f"{fan} shared={shared}", err_d, err_n, err_r, bound=y.CEILING)


# ---- gpd_rollout_obst: the clearance walk split over a group of G lanes ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def course(n):
    """n single-drone aviaries whose reset poses are the points of obstacles_edges.task_points at identity attitude, with a time limit
    of one step: whatever a step does, the next one ends the episode, and its row shows the reset pose"""
    from gym_pybullet_drones_amd import engine
    dev = torch.device("cuda", torch.cuda.current_device())
    pos = ed.task_points(n)
    core = engine.SimCore(num_envs=n, drones_per_env=1, physics=0, pyb_freq=240, ctrl_freq=240, act_code=0, task=1,
                          initial_xyzs=pos.astype(np.float64)[:, None, :], target_pos=np.array([[0.0, 0.0, 1.0]]), episode_len_sec=0.0,
                          auto_reset=True, device=dev)
    assert core._cfg.trunc_counter == 0
    return core, pos


def reset_rows(core, lists, shared, rays, frame=2):
    """K = 2 steps in one launch -> the rows of the second step [N, 16 + R]: every aviary auto-reset there"""
    from gym_pybullet_drones_amd import _native
    dev, N, R = core.device, core.N, 0 if rays is None else len(rays)
    lists3 = lists[None] if shared else lists
    ld = 1 if shared else N + 3
    task = _native.GpdObstTask(collision_radius=y.COLLISION_RADIUS, hit_terminates=1, hit_reward=-5.0, prox_margin=0.5, prox_weight=2.0, n_rays=R,
                               ray_frame=frame, max_range=y.MAX_RANGE)
    core.reset()
    rows, _, term, trunc, _ = core.rollout_obst(task, device_table(lists3, shared, ld, dev), lists3.shape[1], ld,
                                                None if rays is None else torch.as_tensor(rays, device=dev).contiguous(),
                                                torch.zeros((2, N, 4), device=dev))
    torch.cuda.synchronize()
    assert bool((term[1] | trunc[1]).all())
    return rows[1, :, :16 + R].cpu().numpy()


@pytest.mark.parametrize("shared", (True, False), ids=("shared", "planes"))
@pytest.mark.parametrize("n_rays", (0, 1, 2, 3, 5, 16, 33, 64))
def test_fused_kernel_split_walk_names_the_lower_record_at_every_group_size(gpu_device, n_rays, shared):
    """G = 1, 1, 2, 4, 8, 16, 64, 64 lanes per drone against lists of 5, 8, 9 and 65 records (shorter than G, equal to G, no multiple
    of G), 70 and 257 aviaries (a ragged last workgroup): the row's (nx, ny, nz, d) and ranges are the yardstick's at every point --
    on the corridor's centre line the normal of the wall at +y, never its mirror image's"""
    import obst_task_f64 as yo
    G = yo.group_lanes(n_rays)
    assert G == {0: 1, 1: 1, 2: 2, 3: 4, 5: 8, 16: 16, 33: 64, 64: 64}[n_rays]
    rays = np.ascontiguousarray(np.resize(ed.axis_dirs(), (n_rays, 3))) if n_rays else None
    for n in (70, 257):
        core, pos = course(n)
        for M, obst in ed.task_lists().items():
            lists = obst if shared else ed.rotated(obst, n)
            row = reset_rows(core, lists, shared, rays)
            np.testing.assert_array_equal(row[:, :3], pos)
            assert not row[:, 3:12].any()
            got = {"clear4": row[:, 12:16], "ranges": row[:, 16:] if n_rays else None}
            errs = ed.compare_all(got, lists, pos, ed.per_point(rays, n) if n_rays else None)
            record("gpd_rollout_obst", f"R={n_rays} G={G} M={M} N={n} shared={shared}", *errs)
            if shared and M in (5, 9):                            # the corridor: 40 centre-line points tie, the answer is the wall at +y
                want = y.clearance(obst, pos)
                tie = want["second"] == want["d"]
                walls = tie & (want["nearest"] == 0) & (np.arange(n) < 68)          # (of the corridor's own points)
                assert tie[:68].sum() == 40 and walls.sum() == 20
                assert (np.abs(row[walls, 12:15] - np.array([0, -1, 0])) <= ed.BOUND).all()       # ((1 / 0.75) * 0.75 may round below 1)

"""Obstacle fields, the part that needs no GPU: the float64 yardstick (tests/helpers/obstacles_f64.py) pinned by analytic known
answers, csrc/obstacle_math.inc compiled for the host under ASan + UBSan (tests/c/obstacle_host.c) against the yardstick on the
test scene and, with nothing left out, on the scenes of degenerate geometry (tests/helpers/obstacles_edges.py: axis rays, points on the
obstacle, exact ties and thresholds), every refusal of `gpd_obstacles` (all before the first device call), and the packing helpers of
`obstacles.py`."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import obstacles_edges as ed  # noqa: E402
import obstacles_f64 as y  # noqa: E402

INF = np.inf
S2, S3 = math.sqrt(2.0), math.sqrt(3.0)


def _sdf1(rec, p):
    d, g = y.sdf(np.array([rec]), np.array([p], dtype=np.float64))
    return d[0, 0], g[0, 0]


def _ray1(rec, p, d):
    d = np.asarray(d, dtype=np.float64)
    return y.ray(np.array([rec]), np.array([p], dtype=np.float64), (d / np.linalg.norm(d))[None, None])[0, 0, 0]


# ---- the yardstick against answers worked out by hand ----------------------------------------------------------------------------
def test_yardstick_sphere_distance():
    s = y.record(y.SPHERE, (1, 2, 3), (0.5, 0, 0))
    d, g = _sdf1(s, (1, 2 + 2, 3))
    assert d == pytest.approx(1.5) and g == pytest.approx([0, 1, 0])
    d, g = _sdf1(s, (1 + 0.1, 2, 3))                      # inside: negative, still pointing outwards
    assert d == pytest.approx(-0.4) and g == pytest.approx([1, 0, 0])
    d, g = _sdf1(s, (1 + 1, 2 + 2, 3 + 2))
    assert d == pytest.approx(3 - 0.5) and g == pytest.approx([1 / 3, 2 / 3, 2 / 3])
    d, g = _sdf1(s, (1, 2, 3))                            # the centre: the gradient is (0, 0, 1) by definition
    assert d == pytest.approx(-0.5) and list(g) == [0, 0, 1]


def test_yardstick_box_face_edge_corner_and_inside():
    b = y.record(y.BOX, (0, 0, 1), (1, 2, 0.5))
    d, g = _sdf1(b, (3, 1, 1.2))                          # face +x
    assert d == pytest.approx(2) and g == pytest.approx([1, 0, 0])
    d, g = _sdf1(b, (-1 - 3, 0.5, 1 + 0.5 + 4))           # edge -x / +z: 3 and 4 beyond
    assert d == pytest.approx(5) and g == pytest.approx([-0.6, 0, 0.8])
    d, g = _sdf1(b, (1 + 1, -2 - 1, 1 - 0.5 - 1))         # corner +x / -y / -z
    assert d == pytest.approx(S3) and g == pytest.approx([1 / S3, -1 / S3, -1 / S3])
    d, g = _sdf1(b, (0.2, 1.9, 1.1))                      # inside: 0.1 from the +y face, 0.4 from +z, 0.8 from +x
    assert d == pytest.approx(-0.1) and list(g) == [0, 1, 0]
    d, g = _sdf1(b, (-0.7, 0, 1 - 0.2))                   # inside: 0.3 from -x and 0.3 from -z: the tie goes to the lower axis
    assert d == pytest.approx(-0.3) and list(g) == [-1, 0, 0]
    d, g = _sdf1(b, (0, 0, 1))                            # the centre: z is the thinnest, +z the side of a point on the mid plane
    assert d == pytest.approx(-0.5) and list(g) == [0, 0, 1]


def test_yardstick_cylinder_side_cap_rim_and_inside():
    c = y.record(y.CYLINDER, (1, 1, 2), (0.5, 0, 1.5))
    d, g = _sdf1(c, (1 + 3, 1 + 4, 2.7))                  # side: rho = 5
    assert d == pytest.approx(4.5) and g == pytest.approx([0.6, 0.8, 0])
    d, g = _sdf1(c, (1.2, 1.1, 2 + 1.5 + 2))              # above the top cap
    assert d == pytest.approx(2) and g == pytest.approx([0, 0, 1])
    d, g = _sdf1(c, (1, 1 - 0.5 - 3, 2 - 1.5 - 4))        # the bottom rim: 3 out, 4 below
    assert d == pytest.approx(5) and g == pytest.approx([0, -0.6, -0.8])
    d, g = _sdf1(c, (1 + 0.4, 1, 2.2))                    # inside, the wall is nearest (0.1)
    assert d == pytest.approx(-0.1) and g == pytest.approx([1, 0, 0])
    d, g = _sdf1(c, (1.1, 1, 2 - 1.45))                   # inside, the bottom cap is nearest (0.05)
    assert d == pytest.approx(-0.05) and list(g) == [0, 0, -1]
    d, g = _sdf1(c, (1, 1, 2.3))                          # on the axis: the radial direction is (1, 0, 0) by definition
    assert d == pytest.approx(-0.5) and list(g) == [1, 0, 0]
    d, g = _sdf1(c, (1, 1, 2 + 1.5 + 1))                  # on the axis above the cap: no radial part at all
    assert d == pytest.approx(1) and list(g) == [0, 0, 1]


def test_yardstick_floor_and_none():
    f = y.record(y.FLOOR, (0, 0, 0.25))
    d, g = _sdf1(f, (3, -4, 1))
    assert d == pytest.approx(0.75) and list(g) == [0, 0, 1]
    assert _sdf1(f, (0, 0, 0))[0] == pytest.approx(-0.25)
    d, g = _sdf1(y.record(y.NONE, (0, 0, 0), (1, 1, 1)), (0, 0, 0))
    assert d == INF and list(g) == [0, 0, 0]
    assert _ray1(y.record(y.NONE), (0, 0, 1), (0, 0, -1)) == INF
    assert _ray1(f, (0, 0, 1.25), (0, 0, -1)) == pytest.approx(1)
    assert _ray1(f, (0, 0, 1.25), (3, 0, -4)) == pytest.approx(1.25)
    assert _ray1(f, (0, 0, 1.25), (1, 0, 0)) == INF and _ray1(f, (0, 0, 1.25), (0, 0, 1)) == INF      # level, and pointing away
    assert _ray1(f, (0, 0, 0.1), (0, 0, 1)) == 0                                                       # below it already


def test_yardstick_rays():
    s = y.record(y.SPHERE, (0, 0, 0), (1, 0, 0))
    assert _ray1(s, (-3, 0, 0), (1, 0, 0)) == pytest.approx(2)                   # axis-parallel, through the centre
    assert _ray1(s, (-3, 0.6, 0), (1, 0, 0)) == pytest.approx(3 - 0.8)           # a chord: enters at x = -0.8
    assert _ray1(s, (-3, 0, 0), (-1, 0, 0)) == INF                               # points away
    assert _ray1(s, (-3, 1.5, 0), (1, 0, 0)) == INF                              # passes by
    assert _ray1(s, (0.2, 0.1, 0), (0, 1, 0)) == 0                               # starts inside
    b = y.record(y.BOX, (0, 0, 0), (1, 2, 3))
    assert _ray1(b, (-4, 1, 1), (1, 0, 0)) == pytest.approx(3)                   # parallel to two slabs, inside both
    assert _ray1(b, (-4, 2.5, 1), (1, 0, 0)) == INF                              # parallel to a slab it is outside of
    assert _ray1(b, (-2, -3, 0), (1, 1, 0)) == pytest.approx(S2)                 # through the corner region: enters at (-1, -2)
    assert _ray1(b, (0.5, 0.5, 0.5), (0, 0, 1)) == 0                             # starts inside
    assert _ray1(b, (0, 0, 5), (0, 0, 1)) == INF                                 # points away
    c = y.record(y.CYLINDER, (0, 0, 0), (1, 0, 2))
    assert _ray1(c, (-3, 0, 1), (1, 0, 0)) == pytest.approx(2)                   # the wall
    assert _ray1(c, (0.5, 0, 5), (0, 0, -1)) == pytest.approx(3)                 # straight down onto the cap (a vertical ray)
    assert _ray1(c, (1.5, 0, 5), (0, 0, -1)) == INF                              # straight down beside it
    assert _ray1(c, (-3, 0, 5), (1, 0, -1)) == pytest.approx(3 * S2)             # over the rim onto the top cap at x = 0
    assert _ray1(c, (-3, 0, 2.5), (1, 0, 0)) == INF                              # above the cap, level
    assert _ray1(c, (0, 0.5, -1), (1, 1, 1)) == 0                                # starts inside
    assert _ray1(c, (-3, 0.6, 0), (1, 0, 0)) == pytest.approx(3 - 0.8)


def test_yardstick_reductions_and_the_tie_rule():
    s = y.record(y.SPHERE, (0, 0, 1), (0.5, 0, 0))
    obst = np.array([y.record(y.NONE), s, s, y.record(y.FLOOR)])                 # two identical records: the lower one wins
    p = np.array([[1.0, 0, 1], [0, 0, 0.2], [np.nan, 0, 1], [0, 0, 1.1]])
    c = y.clearance(obst, p, 0.06)
    assert list(c["nearest"]) == [1, 3, -1, 1] and c["d"][:2] == pytest.approx([0.5, 0.2]) and c["d"][2] == INF
    assert list(c["normal"][2]) == [0, 0, 0] and list(c["hit"]) == [False, False, False, True]
    dirs = np.broadcast_to(np.array([[-1.0, 0, 0], [0, 0, -1.0], [0, 0, 1.0]]), (4, 3, 3))
    r = y.scan(obst, p, dirs, 5.0)
    assert r["ranges"][0] == pytest.approx([0.5, 1.0, 5.0]) and list(r["ray_hit"][0]) == [1, 3, -1]
    assert list(r["ranges"][2]) == [5.0, 5.0, 5.0] and list(r["ray_hit"][2]) == [-1, -1, -1]       # no position
    assert list(r["ray_hit"][3]) == [1, 1, 1] and list(r["ranges"][3]) == [0, 0, 0]                # inside the first of the twins
    none = y.clearance(np.array([y.record(y.NONE)] * 3), p)
    assert (none["d"] == INF).all() and (none["nearest"] == -1).all() and not none["hit"].any() and not none["normal"].any()
    assert y.scan(obst, p, dirs, 0.8)["ranges"][0] == pytest.approx([0.5, 0.8, 0.8])                # the cap


def test_yardstick_frames():
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(4, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    yaw = 0.7
    q = np.array([[0, 0, math.sin(yaw / 2), math.cos(yaw / 2)]]) * 1.7                          # |q| does not matter
    Rz = np.array([[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]])
    np.testing.assert_allclose(y.rotate(dirs, q, 0)[0], dirs)
    np.testing.assert_allclose(y.rotate(dirs, q, 1)[0], dirs @ Rz.T, atol=1e-12)
    np.testing.assert_allclose(y.rotate(dirs, q, 2)[0], dirs @ Rz.T, atol=1e-12)                # a pure yaw: body = levelled
    roll = 0.4                                                                                 # a roll on top: only the body frame tilts
    q2 = np.array([[math.cos(yaw / 2) * math.sin(roll / 2), math.sin(yaw / 2) * math.sin(roll / 2), math.sin(yaw / 2) * math.cos(roll / 2),
                    math.cos(yaw / 2) * math.cos(roll / 2)]]) * 0.6
    Rx = np.array([[1, 0, 0], [0, math.cos(roll), -math.sin(roll)], [0, math.sin(roll), math.cos(roll)]])
    np.testing.assert_allclose(y.rotate(dirs, q2, 1)[0], dirs @ Rz.T, atol=1e-12)
    np.testing.assert_allclose(y.rotate(dirs, q2, 2)[0], dirs @ (Rz @ Rx).T, atol=1e-12)


# ---- the test scene: what the exclusion rules leave out of it, on the yardstick alone ----------------------------------------------
def test_scene_exercises_both_branches_and_stays_inside_the_caps():
    obst, pos, dirs = y.scene(0)
    assert obst.shape == (25, 8) and pos.shape == (210, 3) and dirs.shape == (210, 16, 3)
    c, s, g = y.clearance(obst, pos), y.scan(obst, pos, dirs), y.grazing(obst, pos, dirs)
    inside, seen = (c["d"] < 0).mean(), (s["ray_hit"] >= 0).mean()
    assert 0.02 <= inside <= 0.07 and 0.45 <= seen <= 0.55 and c["hit"].any() and not c["hit"].all()
    assert g.mean() <= y.CAP_RAYS / 3
    assert not (c["second"] - c["d"] < y.NEAR_TIE).any() and not (np.abs(c["d"] - y.COLLISION_RADIUS) < y.ON_THRESHOLD).any()
    assert set(np.unique(c["nearest"])) >= {0, 8, 16, 24}                     # every kind is somebody's nearest


# ---- csrc/obstacle_math.inc on the host against the yardstick ----------------------------------------------------------------------
#: 3 x the largest error the host-compiled fp32 math shows on the scene (1.7e-6, on `ranges`; d 1.5e-7, normal 1.2e-7): DESIGN.md 3.14
HOST_BOUND = 5.2e-6


def run_host_program(exe, tmp, obst, pos, dirs, max_range=y.MAX_RANGE, radius=y.COLLISION_RADIUS):
    """tests/c/obstacle_host.c on float32 inputs -> dict of its outputs"""
    import host_lib
    M, N, R = len(obst), len(pos), dirs.shape[1]
    src, dst = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "values.bin")
    with open(src, "wb") as f:
        f.write(np.array([M, N, R], dtype=np.int32).tobytes())
        f.write(np.array([max_range, radius], dtype=np.float32).tobytes())
        for a in (obst, pos, dirs):
            f.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    res = host_lib.run(exe, src, dst)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    raw, off, out = open(dst, "rb").read(), 0, {}
    for name, shape, dt in (("d", (N, M), np.float32), ("grad", (N, M, 3), np.float32), ("t", (N, M, R), np.float32), ("clear4", (N, 4), np.float32),
                            ("ranges", (N, R), np.float32), ("nearest", (N,), np.int32), ("hit", (N,), np.int32), ("ray_hit", (N, R), np.int32)):
        n = int(np.prod(shape)) * 4
        out[name] = np.frombuffer(raw[off:off + n], dtype=dt).reshape(shape)
        off += n
    assert off == len(raw)
    return out


def test_host_compiled_math_agrees_with_the_yardstick(tmp_path):
    """The text the kernels compile, built as a stand-alone program under ASan + UBSan and run on the scene: every pair's signed
    distance and gradient, and the reductions (clearance, nearest, hit, ranges, ray_hit) under the exclusion rules, within 3 x the error
    measured when this was written -- far below the project's 1e-4."""
    import host_lib
    from gym_pybullet_drones_amd import _native
    exe = host_lib.program("obstacle_host", include=(_native.CSRC,))
    obst, pos, dirs = (a.astype(np.float32) for a in y.scene(0))          # (the yardstick sees the rounded inputs)
    got = run_host_program(exe, str(tmp_path), obst, pos, dirs)
    d64, g64 = y.sdf(obst, pos)
    pair_d, pair_g = float(y.rel_err(got["d"], d64).max()), float(y.rel_err(got["grad"], g64).max())
    err_d, err_n = y.compare_clearance(got, obst, pos)
    err_r = y.compare_scan(got, obst, pos, dirs)
    print(f"MEASURED host obstacle math: pair d {pair_d:.3e} pair grad {pair_g:.3e} d {err_d:.3e} normal {err_n:.3e} ranges {err_r:.3e}")
    assert HOST_BOUND <= y.CEILING
    assert max(pair_d, pair_g, err_d, err_n, err_r) <= HOST_BOUND
    # a miss is +inf for every pair, and an origin inside is 0: never a NaN
    assert not np.isnan(got["t"]).any() and (got["t"] >= 0).all() and (got["t"] == 0).any() and np.isinf(got["t"]).any()


# ---- degenerate geometry: axis rays, points on the obstacle, exact ties and thresholds (tests/helpers/obstacles_edges.py) -----------
def test_edge_scenes_hold_every_category_they_exist_for():
    """a later edit of a scene cannot silently empty a category: the lattice holds every one, the corridor the ties and the rays along
    its walls; the counts the scenes were chosen by are pinned"""
    la, co = ed.census(ed.lattice()), ed.census(ed.corridor())
    print("MEASURED census of the lattice: " + ", ".join(f"{k} {v}" for k, v in la.items()))
    print("MEASURED census of the corridor: " + ", ".join(f"{k} {v}" for k, v in co.items()))
    assert ed.lattice().pos.shape == (1650, 3) and ed.corridor().pos.shape == (68, 3)
    empty = [k for k, v in la.items() if v == 0] + [f"corridor: {k}" for k in ed.CORRIDOR_CATEGORIES if co[k] == 0]
    assert not empty, empty
    assert la["tie_of_the_nearest"] == 90 and co["tie_of_the_nearest"] == 40
    for name, s in ed.scenes().items():                                     # (the variants keep what their scene has)
        c = ed.census(s)
        base = la if name.startswith("lattice") else co
        assert c["tie_of_the_nearest"] >= base["tie_of_the_nearest"] and c["negative_zero_coordinate"] == base["negative_zero_coordinate"], name
    # the inputs are dyadic: float32 holds them, and every difference point - centre, exactly
    for s in ed.scenes().values():
        assert (s.pos * 16 == np.round(s.pos * 16)).all() and (s.obst * 16 == np.round(s.obst * 16)).all(), s.name


def test_yardstick_on_the_edge_scenes_names_the_lower_record():
    la, co = ed.lattice(), ed.corridor()
    dirs = ed.per_point(ed.axis_dirs(), len(la.pos))
    base, base_s = y.clearance(la.obst, la.pos), y.scan(la.obst, la.pos, dirs)
    first = np.array([0, 2, 4, 6])                                           # where the twins list holds the lattice's records first
    tw, tw_s = y.clearance(ed.twins(la.obst), la.pos), y.scan(ed.twins(la.obst), la.pos, dirs)
    np.testing.assert_array_equal(tw["nearest"], first[base["nearest"]])
    np.testing.assert_array_equal(tw_s["ray_hit"], np.where(base_s["ray_hit"] >= 0, first[base_s["ray_hit"]], -1))
    assert (tw["second"][base["nearest"] != 3] == tw["d"][base["nearest"] != 3]).all()      # every solid nearest is an exact tie
    no, no_s = y.clearance(ed.with_none(la.obst), la.pos), y.scan(ed.with_none(la.obst), la.pos, dirs)
    np.testing.assert_array_equal(no["nearest"], 2 * base["nearest"] + 1)
    np.testing.assert_array_equal(no_s["ray_hit"], np.where(base_s["ray_hit"] >= 0, 2 * base_s["ray_hit"] + 1, -1))
    np.testing.assert_array_equal(no["d"], base["d"])
    c = y.clearance(co.obst, co.pos)
    tie = c["second"] == c["d"]
    assert tie.sum() == 40 and set(c["nearest"]) == {0, 2, 4} and set(c["nearest"][tie]) == {0, 2}
    assert (c["normal"][c["nearest"] == 0] == [0, -1, 0]).all()               # the wall at +y pushes towards -y, never its mirror image
    level = y.scan(co.obst, co.pos, ed.per_point(ed.axis_dirs(), len(co.pos)))
    assert (level["ray_hit"][:, :4] != 4).all() and (level["ray_hit"][:, 5] == 4).all()      # a level ray never sees the floor


def test_yardstick_at_the_thresholds():
    """a hit is d < radius and a ray sees what enters before max_range: exactly at either is neither"""
    obst, cases = ed.thresholds()
    pts, org, dirs = ed.threshold_points(), ed.threshold_origins(), ed.axis_dirs()
    c = y.clearance(obst, pts, ed.RADIUS)
    assert list(c["d"][:5]) == [ed.RADIUS] * 5 and (c["d"][5:] < ed.RADIUS).all() and (c["d"][5:] > ed.RADIUS - 1e-6).all()
    assert list(c["nearest"]) == [k.record for k in cases] * 2 and list(c["hit"]) == [False] * 5 + [True] * 5
    assert y.clearance(obst, pts, float(ed.up(ed.RADIUS)))["hit"].all()
    at, above = (y.scan(obst, org, ed.per_point(dirs, 5), float(r)) for r in (ed.RANGE, ed.up(ed.RANGE)))
    for i, k in enumerate(cases):
        assert at["entry"][i, k.ray] == ed.RANGE and at["ranges"][i, k.ray] == ed.RANGE and at["ray_hit"][i, k.ray] == -1, k.name
        assert above["ranges"][i, k.ray] == ed.RANGE and above["ray_hit"][i, k.ray] == k.record, k.name


def test_shifted_lattice_keeps_the_fans_inside_the_caps():
    """the non-axis scans of tests/test_gpu_obstacles_edges.py: with the lattice moved by SHIFT and 37 yaws the yardstick alone leaves out
    at most CAP_RAYS of the rays as grazing and CAP_DRONES of the drones for a near tie (unshifted, 19 % of diagonal rays graze)"""
    from gym_pybullet_drones_amd import obstacles as ob
    obst = ed.lattice().obst
    pos, quat = ed.shifted_lattice()
    assert len(np.unique(quat, axis=0)) == ed.N_YAWS
    assert y.compare_clearance({}, obst, pos) == (0.0, 0.0)                  # (its caps on near ties and on points near the radius hold)
    for fan in (ob.fan(16, 2 * math.pi), ob.fan(5, math.pi / 2, -0.5)):
        dirs = y.rotate(fan, quat, 1)
        graze, s = y.grazing(obst, pos, dirs), y.scan(obst, pos, dirs)
        with np.errstate(invalid="ignore"):
            tie = ((s["second"] - s["entry"] < y.NEAR_TIE) & ~graze).any(axis=1)
        print(f"MEASURED shifted lattice, {len(fan)} rays: grazing {graze.mean():.4f} tie drones {tie.mean():.4f} seen {(s['ray_hit'] >= 0).mean():.3f}")
        assert graze.mean() <= y.CAP_RAYS and tie.sum() <= y.CAP_DRONES * len(pos)
        assert 0.2 <= (s["ray_hit"] >= 0).mean() < 1.0                        # (the fan that looks down sees the floor with most rays)


def test_lists_of_the_fused_kernel_keep_their_ties():
    """what tests/test_gpu_obstacles_edges.py flies: lists of 5, 8, 9 and 65 records, each with exact ties among its 70 and 257 points,
    and rotating a list's order moves the answer with it"""
    import obst_task_f64 as yo
    assert [yo.group_lanes(r) for r in (0, 1, 2, 3, 5, 16, 33, 64)] == [1, 1, 2, 4, 8, 16, 64, 64]
    lists = ed.task_lists()
    assert sorted(lists) == [5, 8, 9, 65]
    for n in (70, 257):
        pos = ed.task_points(n)
        assert pos.shape == (n, 3) and n % 64 != 0
        for M, obst in lists.items():
            c = y.clearance(obst, pos)
            tie = c["second"] == c["d"]
            assert tie.sum() >= (40 if M != 8 else 1) and np.isfinite(c["d"]).all(), (n, M)
            assert (c["nearest"][tie] < c["nearest"].max()).any()
            rot = y.clearance(ed.rotated(obst, n), pos)
            np.testing.assert_array_equal(rot["d"], c["d"])
            moved = (c["nearest"] - np.arange(n)) % M
            assert (rot["nearest"] <= moved).all() and (rot["nearest"] == moved)[~tie].all()
    long = lists[65]
    assert long[64, 3] == y.FLOOR and (long[[0, 1], 3] == y.BOX).all() and (long[:, 3] == y.NONE).sum() == 54


@functools.lru_cache(maxsize=None)
def obstacle_host():
    import host_lib
    from gym_pybullet_drones_amd import _native
    return host_lib.program("obstacle_host", include=(_native.CSRC,))


@pytest.mark.parametrize("name", list(ed.scenes()))
def test_host_compiled_math_on_degenerate_scenes_with_no_exclusion(tmp_path, name):
    """The C text on the lattice, the corridor, the twins and the lists with skipped records, under the eight axis directions: the
    class of every t (inf / 0 / positive) and d (sign, == 0), `nearest`, `hit` and `ray_hit` equal to the yardstick's at EVERY point,
    record and ray -- ties go to the lower record, points on a surface are on it -- no NaN, and values within 1e-6 (ed.BOUND).
    MEASURED (clang -O1, the largest over the five scenes): pair d 1.1e-07, gradient 1.3e-07, t 6.8e-08"""
    s = ed.scenes()[name]
    dirs = ed.per_point(ed.axis_dirs(), len(s.pos))
    got = run_host_program(obstacle_host(), str(tmp_path), s.obst, s.pos, dirs)
    pair_d, pair_g, pair_t = ed.compare_pairs(got, s.obst, s.pos, dirs)
    err_d, err_n, err_r = ed.compare_all(got, s.obst, s.pos, dirs)
    print(f"MEASURED host obstacle math on {name}: pair d {pair_d:.3e} pair grad {pair_g:.3e} pair t {pair_t:.3e} d {err_d:.3e} "
          f"normal {err_n:.3e} ranges {err_r:.3e}")
    assert max(pair_d, pair_g, pair_t, err_d, err_n, err_r) <= ed.BOUND
    assert np.isinf(got["t"]).any() and (got["t"] < np.inf).any()
    if name.startswith("lattice"):
        assert (got["t"] == 0).any() and (got["d"] == 0).any() and (got["d"][np.isfinite(got["d"])] < 0).any()


def test_host_compiled_math_at_the_thresholds(tmp_path):
    """`hit` is d < radius, an entry AT max_range is not seen: the point exactly RADIUS outside every kind of surface is no hit, one
    ulp nearer (or with a radius one ulp larger) it is; the axis ray that enters at exactly RANGE reports max_range and -1, and the record
    with max_range one ulp larger"""
    obst, cases = ed.thresholds()
    pts, org = ed.threshold_points(), ed.threshold_origins()
    dirs = ed.axis_dirs()
    for radius, hits in ((np.float32(ed.RADIUS), [0] * 5 + [1] * 5), (ed.up(ed.RADIUS), [1] * 10)):
        got = run_host_program(obstacle_host(), str(tmp_path), obst, pts, ed.per_point(dirs, len(pts)), radius=radius)
        assert list(got["hit"]) == hits and list(got["nearest"]) == [k.record for k in cases] * 2
        assert list(got["clear4"][:5, 3]) == [ed.RADIUS] * 5 and (got["clear4"][5:, 3] < ed.RADIUS).all()
        assert max(ed.compare_all(got, obst, pts, ed.per_point(dirs, len(pts)), radius=float(radius))) <= ed.BOUND
    for max_range, seen in ((np.float32(ed.RANGE), False), (ed.up(ed.RANGE), True)):
        got = run_host_program(obstacle_host(), str(tmp_path), obst, org, ed.per_point(dirs, len(org)), max_range=max_range)
        for i, k in enumerate(cases):
            assert got["t"][i, k.record, k.ray] == ed.RANGE, k.name
            assert got["ranges"][i, k.ray] == (ed.RANGE if seen else max_range) and got["ray_hit"][i, k.ray] == (k.record if seen else -1), k.name
        assert max(ed.compare_all(got, obst, org, ed.per_point(dirs, len(org)), max_range=float(max_range))) <= ed.BOUND


# ---- the entry's refusals ---------------------------------------------------------------------------------------------------------------
def test_entry_rejects_bad_arguments_before_touching_a_device():
    """Every argument error of gpd_obstacles is found before the first HIP call: the code include/gpd.h states and a message that
    starts with the entry's name (host buffers stand in for device memory: nothing is launched)."""
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    assert "gpd_obstacles" in _native.exported_symbols() and L.gpd_abi_version() == 9
    buf = (ctypes.c_float * 16384)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ok = dict(pos4=base, quat4=base + 4096, n=60, drones_per_env=3, obst=base + 8192, n_obst=4, obst_ld=1, collision_radius=0.06,
              clear4=base + 12288, nearest=base + 16384, hit=base + 20480, ray_dirs=base + 24576, n_rays=8, ray_frame=2, max_range=5.0,
              ranges=base + 28672, ray_hit=base + 36864)

    def rc(**change):
        a = {**ok, **change}
        return L.gpd_obstacles(*[a[n] for n in ok], None)

    def rejected(code, **change):
        assert rc(**change) == code, change
        assert L.gpd_last_error().decode().startswith("gpd_obstacles"), change

    EINVAL, ERANGE = _native.GPD_EINVAL, _native.GPD_ERANGE
    rejected(EINVAL, pos4=None)
    rejected(EINVAL, obst=None)
    rejected(EINVAL, clear4=None, nearest=None, hit=None, ranges=None)            # nothing asked for
    rejected(EINVAL, clear4=None, nearest=None, hit=None, ranges=None, ray_hit=ok["ray_hit"])      # (ray_hit alone is not an output)
    rejected(EINVAL, pos4=base + 4)
    rejected(EINVAL, quat4=base + 4096 + 8)
    rejected(EINVAL, clear4=base + 12288 + 4)
    for n in (0, -3, 61):                                                         # 61 rows are not whole aviaries of 3
        rejected(EINVAL, n=n)
    rejected(EINVAL, drones_per_env=-1)
    rejected(ERANGE, n=2 ** 26 + 1, drones_per_env=1)
    for m in (0, -1, 1025):
        rejected(ERANGE, n_obst=m)
    for ld in (0, -1, 19, 2):                                                     # 20 aviaries: a list each needs a pitch of 20
        rejected(EINVAL, obst_ld=ld)
    rejected(EINVAL, obst_ld=60, drones_per_env=0)                                # one world has one list
    rejected(EINVAL, ray_dirs=None)
    for r in (0, -1, 65):
        rejected(ERANGE, n_rays=r)
    for f in (-1, 3):
        rejected(EINVAL, ray_frame=f)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        rejected(EINVAL, max_range=r)
    for f in (1, 2):
        rejected(EINVAL, quat4=None, ray_frame=f)


# ---- obstacles.py: packing and helpers -------------------------------------------------------------------------------------------------
def test_field_table_layout_shared_and_per_aviary():
    from gym_pybullet_drones_amd import obstacles as ob
    f = ob.ObstacleField().sphere((1, 2, 3), 0.5).box((0, 0, 1), (0.1, 0.2, 0.3)).cylinder((4, 5, 6), 0.25, 1.5).floor(0.125).none()
    t = f.table("cpu")
    assert t.dtype.is_floating_point and t.shape == (5, 8) and t.is_contiguous() and f.obst_ld == 1 and len(f) == 5
    np.testing.assert_array_equal(t.numpy(), np.array([[1, 2, 3, ob.SPHERE, 0.5, 0, 0, 0], [0, 0, 1, ob.BOX, 0.1, 0.2, 0.3, 0],
                                                       [4, 5, 6, ob.CYLINDER, 0.25, 0, 1.5, 0], [0, 0, 0.125, ob.FLOOR, 0, 0, 0, 0],
                                                       [0, 0, 0, ob.NONE, 0, 0, 0, 0]], dtype=np.float32))
    E = 3
    centres = np.arange(E * 3, dtype=np.float64).reshape(E, 3)
    g = ob.ObstacleField(E).floor(0.0).sphere(centres, [0.1, 0.2, 0.3]).none(where=[False, True, False]).box((1, 1, 1), (0.5, 0.5, 0.5))
    t = g.table("cpu").numpy()
    assert t.shape == (3 * 8, E) and g.obst_ld == E
    rec = g.records()                                                                              # [E, M, 8]
    for e in range(E):
        for m in range(3):
            for k in range(8):
                assert t[m * 8 + k, e] == np.float32(rec[e, m, k])                                 # float f of record m of aviary e
    assert list(t[1 * 8 + 3]) == [ob.SPHERE, ob.NONE, ob.SPHERE] and list(t[1 * 8 + 4]) == [np.float32(0.1), np.float32(0.2), np.float32(0.3)]
    assert list(t[2 * 8 + 3]) == [ob.BOX] * 3
    with pytest.raises(ValueError):
        ob.ObstacleField().table("cpu")
    with pytest.raises(ValueError):
        ob.ObstacleField().sphere((0, 0, 0), -1.0)
    with pytest.raises(ValueError):
        ob.ObstacleField(2).sphere(np.zeros((3, 3)), 1.0)


def test_random_cylinders_stand_on_the_ground_inside_the_area():
    from gym_pybullet_drones_amd import obstacles as ob
    f = ob.ObstacleField.random_cylinders(6, 5, (-1, -2, 3, 4), (0.1, 0.3), (1.0, 2.0), np.random.default_rng(1))
    rec = f.records()
    assert rec.shape == (6, 5, 8) and (rec[..., 3] == ob.CYLINDER).all()
    assert (rec[..., 0] >= -1).all() and (rec[..., 0] <= 3).all() and (rec[..., 1] >= -2).all() and (rec[..., 1] <= 4).all()
    assert (rec[..., 4] >= 0.1).all() and (rec[..., 4] <= 0.3).all() and (rec[..., 6] >= 0.5).all() and (rec[..., 6] <= 1.0).all()
    np.testing.assert_allclose(rec[..., 2], rec[..., 6])                                          # the base is on z = 0
    again = ob.ObstacleField.random_cylinders(6, 5, (-1, -2, 3, 4), (0.1, 0.3), (1.0, 2.0), np.random.default_rng(1)).records()
    np.testing.assert_array_equal(rec, again)


def test_fan_returns_unit_vectors():
    from gym_pybullet_drones_amd import obstacles as ob
    for n, fov, el in ((1, 1.0, 0.0), (5, math.pi / 2, 0.0), (16, 2 * math.pi, 0.0), (64, math.pi, 0.3), (7, 1.0, -0.5)):
        d = ob.fan(n, fov, el)
        assert d.shape == (n, 3) and d.dtype == np.float32
        np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=2e-7)
        np.testing.assert_allclose(d[:, 2], math.sin(el), atol=1e-6)
    d = ob.fan(5, math.pi / 2)
    np.testing.assert_allclose(d[2], [1, 0, 0], atol=1e-7)                                       # the middle ray looks ahead
    np.testing.assert_allclose(d[0], [math.cos(math.pi / 4), -math.sin(math.pi / 4), 0], atol=1e-6)
    full = ob.fan(8, 2 * math.pi)
    assert np.linalg.norm(full[0] - full[-1]) > 0.5                                             # a full circle does not double its end
    for bad in (0, 65):
        with pytest.raises(ValueError):
            ob.fan(bad, 1.0)


def test_python_methods_reject_bad_arguments_before_any_device_work():
    from gym_pybullet_drones_amd.envs.SwarmAviary import SwarmAviary
    from gym_pybullet_drones_amd.envs.VectorAviary import VectorAviary
    from gym_pybullet_drones_amd import obstacles as ob
    env = object.__new__(VectorAviary)
    for call in (env.clearance, env.obstacle_hits, lambda: env.range_scan(ob.fan(3, 1.0), 5.0)):
        with pytest.raises(ValueError, match="set_obstacles"):
            call()
    world = object.__new__(SwarmAviary)
    with pytest.raises(ValueError, match="one world"):
        world.set_obstacles(ob.ObstacleField(4).floor())
    with pytest.raises(ValueError, match="set_obstacles"):
        world.clearance()

"""Obstacle fields on the MI355X: `gpd_obstacles` against the float64 yardstick (tests/helpers/obstacles_f64.py, pinned in
tests/test_host_obstacles.py) over the shapes at which the kernels take another path -- shared lists in LDS and per-aviary field
planes, a partial last wave, aviaries of three, one world with rows that have no position, 1 to 300 records with skipped ones in
between, 1 to 64 rays, the three frames with quaternions that are not normalised -- the pinned single cases, the layout and
repeatability of the outputs, the methods of the two batched classes, and the example.

MEASURED on an MI355X (|x32 - x64| / max(1, |x64|), the largest over the cases below; bound 1e-4):
    d 1.2e-07   normal 1.7e-07   ranges 2.9e-06"""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import obstacles_f64 as y  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -77


def make_lists(rng, n_lists, n_obst):
    """[n_lists, n_obst, 8] float32: spheres, boxes and cylinders with skipped records in between and a floor at the end (a lone record
    is a box), sized so that a list of any length fills about the share of the volume the 24 bodies of the test scene do"""
    scale = min(1.0, (24.0 / n_obst) ** (1.0 / 3.0))
    out = np.zeros((n_lists, n_obst, 8))
    kind = rng.choice([y.SPHERE, y.BOX, y.CYLINDER, y.NONE], size=(n_lists, n_obst), p=[0.3, 0.3, 0.3, 0.1])
    if n_obst == 1:
        kind[:] = y.BOX
    else:
        kind[:, -1] = y.FLOOR
    out[..., 0:3] = rng.uniform([-4.0, -4.0, 0.3], [4.0, 4.0, 2.7], size=(n_lists, n_obst, 3))
    out[..., 3] = kind
    sph, box, cyl = (scale * rng.uniform(lo, hi, size=(n_lists, n_obst, 3)) for lo, hi in
                     (([0.2, 0, 0], [0.6, 0, 0]), ([0.15] * 3, [0.6] * 3), ([0.15, 0, 0.5], [0.4, 0, 1.5])))
    out[..., 4:7] = np.where((kind == y.SPHERE)[..., None], sph, np.where((kind == y.BOX)[..., None], box, np.where((kind == y.CYLINDER)[..., None], cyl, 0.0)))
    floor = kind == y.FLOOR
    out[floor, 0:3] = 0.0
    return out.astype(np.float32)


def make_poses(rng, n, nan_rows=()):
    pos = rng.uniform([-4.0, -4.0, 0.05], [4.0, 4.0, 3.0], size=(n, 3)).astype(np.float32)
    q = rng.normal(size=(n, 4))
    q *= (rng.uniform(0.5, 2.0, size=(n, 1)) / np.linalg.norm(q, axis=1, keepdims=True))        # |q| in 0.5 .. 2: DYN never renormalises
    for i, r in enumerate(nan_rows):
        pos[r, i % 3] = np.nan if i % 2 == 0 else np.inf
    return pos, q.astype(np.float32)


def make_dirs(rng, n_rays):
    d = rng.normal(size=(n_rays, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def device_table(lists, shared, ld, dev):
    """[n_lists, M, 8] -> the entry's tensor: [M, 8] for the one shared list, else field planes [M * 8, ld] (ld >= n_lists; the
    columns beyond are NaN: never read)"""
    if shared:
        return torch.as_tensor(lists[0], device=dev).contiguous()
    E, M, _ = lists.shape
    t = np.full((M * 8, ld), np.nan, dtype=np.float32)
    t[:, :E] = lists.transpose(1, 2, 0).reshape(M * 8, E)
    return torch.as_tensor(t, device=dev).contiguous()


def query(dev, pos, quat, D, table, n_obst, ld, dirs=None, frame=0, max_range=y.MAX_RANGE, radius=y.COLLISION_RADIUS,
          want=("clear4", "nearest", "hit", "ranges", "ray_hit"), pad=5, garbage_rays=False):
    """the entry on numpy poses -> dict of numpy outputs; every output has `pad` rows beyond n that must keep their sentinel"""
    from gym_pybullet_drones_amd import _native
    n = len(pos)
    R = 0 if dirs is None else len(dirs)
    pos4 = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    pos4[:, :3] = torch.as_tensor(pos, device=dev)
    quat4 = None if quat is None else torch.as_tensor(quat, device=dev).contiguous()
    dirs_t = None if dirs is None else torch.as_tensor(dirs, device=dev).contiguous()
    shapes = dict(clear4=((n + pad, 4), torch.float32), nearest=((n + pad,), torch.int32), hit=((n + pad,), torch.uint8),
                  ranges=((n + pad, max(R, 1)), torch.float32), ray_hit=((n + pad, max(R, 1)), torch.int32))
    out = {k: torch.full(shapes[k][0], SENTINEL % 256 if k == "hit" else SENTINEL, dtype=shapes[k][1], device=dev) if k in want else None for k in shapes}
    rays = (dirs_t, -5, 7, float("nan")) if garbage_rays else (dirs_t, R, frame, max_range)
    _native.call("gpd_obstacles", dev, None, pos4, quat4, n, D, table, n_obst, ld, radius, out["clear4"], out["nearest"], out["hit"],
                 *rays, out["ranges"], out["ray_hit"])
    torch.cuda.synchronize()
    res = {}
    for k, t in out.items():
        if t is None:
            res[k] = None
            continue
        a = t.cpu().numpy()
        assert (a[n:] == (SENTINEL % 256 if k == "hit" else SENTINEL)).all(), f"{k}: rows beyond n were written"
        res[k] = a[:n]
    return res


#: (name, E, D (0: one world of E rows), shared list?, n_obst, n_rays, frame, rows without a position)
CASES = [
    ("partial-wave-shared-65-body", 70, 1, True, 65, 16, 2, ()),
    ("partial-wave-lists-7-level", 70, 1, False, 7, 5, 1, ()),
    ("partial-wave-lists-300-world", 70, 1, False, 300, 1, 0, ()),
    ("threes-lists-65-world", 5, 3, False, 65, 64, 0, ()),
    ("threes-shared-1-body", 5, 3, True, 1, 1, 2, ()),
    ("world-shared-300-level", 130, 0, True, 300, 16, 1, (3, 64, 129)),
    ("world-shared-7-body", 130, 0, True, 7, 64, 2, (0, 77)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_entry_agrees_with_the_yardstick(gpu_device, case):
    name, E, D, shared, M, R, frame, nan_rows = case
    rng = np.random.default_rng(sum(map(ord, name)))
    n = E * max(D, 1)
    lists = make_lists(rng, 1 if shared else E, M)
    pos, quat = make_poses(rng, n, nan_rows)
    dirs = make_dirs(rng, R)
    ld = 1 if shared else E + 5                                  # a pitch larger than the number of aviaries
    got = query(gpu_device, pos, quat, D, device_table(lists, shared, ld, gpu_device), M, ld, dirs, frame)
    per_row = lists[0] if shared else lists[np.arange(n) // D]   # the list every row sees
    world_dirs = y.rotate(dirs, quat, frame)
    err_d, err_n = y.compare_clearance(got, per_row, pos)
    err_r = y.compare_scan(got, per_row, pos, world_dirs)
    print(f"MEASURED {name}: d {err_d:.3e} normal {err_n:.3e} ranges {err_r:.3e}")
    assert max(err_d, err_n, err_r) <= y.CEILING
    for r in nan_rows:                                            # a row without a position: the specified answers
        assert list(got["clear4"][r]) == [0, 0, 0, np.inf] and got["nearest"][r] == -1 and got["hit"][r] == 0
        assert (got["ranges"][r] == np.float32(y.MAX_RANGE)).all() and (got["ray_hit"][r] == -1).all()
    fin = np.isfinite(pos).all(axis=1)
    assert (got["ranges"][fin] <= np.float32(y.MAX_RANGE)).all() and (got["ranges"] >= 0).all()
    assert ((got["ray_hit"] >= 0) == (got["ranges"] < np.float32(y.MAX_RANGE))).all()
    if M > 1:                                                     # rays that see something and (a lone ray may look down) rays that see nothing
        assert (got["ray_hit"] >= 0).any() and ((got["ray_hit"] < 0).any() or R == 1)


def test_pinned_single_cases(gpu_device):
    dev = gpu_device
    obst = np.array([y.record(y.NONE, (0, 0, 0), (9, 9, 9)), y.record(y.SPHERE, (1, 2, 3), (0.5, 0, 0)), y.record(y.CYLINDER, (-2, 0, 1), (0.25, 0, 1.0))],
                    dtype=np.float32)
    pos = np.array([[1, 2, 3], [-2, 0, 1.5], [np.nan, 0, 0], [1, 2, 3 + 2]], dtype=np.float32)
    table = torch.as_tensor(obst, device=dev)
    dirs = np.array([[0, 0, -1], [1, 0, 0]], dtype=np.float32)
    got = query(dev, pos, None, 0, table, 3, 1, dirs, 0)
    assert list(got["clear4"][0]) == [0, 0, 1, -0.5] and got["nearest"][0] == 1 and got["hit"][0] == 1       # the sphere's centre
    assert list(got["clear4"][1]) == [1, 0, 0, -0.25] and got["nearest"][1] == 2 and got["hit"][1] == 1      # on the cylinder's axis
    assert list(got["clear4"][2]) == [0, 0, 0, np.inf] and got["nearest"][2] == -1 and got["hit"][2] == 0    # the NaN row ...
    assert list(got["ranges"][2]) == [5, 5] and list(got["ray_hit"][2]) == [-1, -1]
    assert list(got["clear4"][3]) == [0, 0, 1, 1.5] and got["nearest"][3] == 1 and got["hit"][3] == 0        # ... and its neighbour
    assert list(got["ranges"][3]) == [1.5, 5] and list(got["ray_hit"][3]) == [1, -1]
    assert list(got["ranges"][0]) == [0, 0] and list(got["ray_hit"][0]) == [1, 1]                            # an origin inside: 0
    # every record NONE
    none = torch.as_tensor(np.array([y.record(y.NONE, (0, 0, 0), (1, 1, 1))] * 4, dtype=np.float32), device=dev)
    got = query(dev, pos, None, 0, none, 4, 1, dirs, 0)
    assert (got["clear4"] == np.array([0, 0, 0, np.inf], dtype=np.float32)).all() and (got["nearest"] == -1).all() and not got["hit"].any()
    assert (got["ranges"] == 5).all() and (got["ray_hit"] == -1).all()
    # a hit is strictly below the radius: a drone exactly `radius` above the floor does not collide, one ulp lower does
    floor = torch.as_tensor(np.array([y.record(y.FLOOR)], dtype=np.float32), device=dev)
    edge = np.array([[0, 0, 0.0625], [0, 0, np.nextafter(np.float32(0.0625), np.float32(0))]], dtype=np.float32)
    got = query(dev, edge, None, 0, floor, 1, 1, None, 0, radius=0.0625, want=("hit", "clear4"))
    assert list(got["hit"]) == [0, 1] and got["clear4"][0, 3] == np.float32(0.0625)


def test_outputs_alone_and_together_and_twice_give_the_same_bits(gpu_device):
    rng = np.random.default_rng(11)
    E, D, M, R = 70, 1, 65, 5
    n = E * D
    pos, quat = make_poses(rng, n, (9,))
    dirs = make_dirs(rng, R)
    for shared in (True, False):
        lists = make_lists(rng, 1 if shared else E, M)
        ld = 1 if shared else E + 2
        table = device_table(lists, shared, ld, gpu_device)
        every = query(gpu_device, pos, quat, D, table, M, ld, dirs, 2)
        again = query(gpu_device, pos, quat, D, table, M, ld, dirs, 2)
        for k in every:
            np.testing.assert_array_equal(every[k].view(np.uint8), again[k].view(np.uint8), err_msg=k)
        for k in ("clear4", "nearest", "hit", "ranges"):
            alone = query(gpu_device, pos, quat, D, table, M, ld, dirs, 2, want=(k,))
            assert all(v is None for kk, v in alone.items() if kk != k)
            np.testing.assert_array_equal(alone[k].view(np.uint8), every[k].view(np.uint8), err_msg=k)
        # without `ranges` the ray arguments are not looked at, whatever they hold
        blind = query(gpu_device, pos, None, D, table, M, ld, None, 0, want=("clear4", "nearest", "hit"), garbage_rays=True)
        for k in ("clear4", "nearest", "hit"):
            np.testing.assert_array_equal(blind[k].view(np.uint8), every[k].view(np.uint8), err_msg=k)


def _entry_on(env_pos, env_quat, D, field, dirs, frame, radius, dev):
    lists = field.records().astype(np.float32)
    shared = field.num_envs is None
    lists = lists[None] if shared else lists
    ld = field.obst_ld
    return query(dev, env_pos.cpu().numpy(), env_quat.cpu().numpy(), D, device_table(lists, shared, ld, dev), lists.shape[1], ld, dirs, frame,
                 radius=radius, pad=0)


def test_vector_aviary_methods_are_the_entry_on_its_state(gpu_device):
    from gym_pybullet_drones_amd import obstacles as ob
    from gym_pybullet_drones_amd.envs import VectorCtrlAviary
    E, D = 6, 2
    rng = np.random.default_rng(2)
    xyz = rng.uniform([-1, -1, 0.5], [1, 1, 1.5], size=(D, 3))
    env = VectorCtrlAviary(E, D, initial_xyzs=xyz, device=gpu_device)
    env.reset()
    with pytest.raises(ValueError, match="set_obstacles"):
        env.clearance()
    rpm = torch.full((E, D, 4), float(env.HOVER_RPM), device=gpu_device)
    rpm[..., 0] *= 1.05                                                        # the attitudes leave level
    for _ in range(20):
        env.step(rpm)
    dirs = ob.fan(5, np.pi / 2)
    for field in (ob.ObstacleField().floor(0.0).sphere((0.3, 0.2, 1.0), 0.4).cylinder((-0.5, 0.5, 1.0), 0.2, 1.0),
                  ob.ObstacleField.random_cylinders(E, 4, (-1.5, -1.5, 1.5, 1.5), (0.1, 0.3), (1.0, 2.0), np.random.default_rng(3)).floor(0.0)):
        env.set_obstacles(field)
        want = _entry_on(env.core.positions(), env.core.quaternions(), D, field, dirs, 2, env.core.P.COLLISION_R, gpu_device)
        c = env.clearance()
        assert c.normal.shape == (E, D, 3) and c.dist.shape == (E, D) and c.nearest.shape == (E, D) and c.hit.shape == (E, D) and c.hit.dtype == torch.bool
        first = c.dist.data_ptr()
        np.testing.assert_array_equal(torch.cat([c.normal, c.dist.unsqueeze(-1)], dim=-1).cpu().numpy().reshape(-1, 4).view(np.uint32), want["clear4"].view(np.uint32))
        np.testing.assert_array_equal(c.nearest.cpu().numpy().reshape(-1), want["nearest"])
        np.testing.assert_array_equal(c.hit.cpu().numpy().reshape(-1), want["hit"].astype(bool))
        np.testing.assert_array_equal(env.obstacle_hits().cpu().numpy().reshape(-1), want["hit"].astype(bool))
        ranges, ids = env.range_scan(dirs, y.MAX_RANGE, want_ids=True)
        assert ranges.shape == (E, D, 5) and ids.shape == (E, D, 5)
        np.testing.assert_array_equal(ranges.cpu().numpy().reshape(-1, 5).view(np.uint32), want["ranges"].view(np.uint32))
        np.testing.assert_array_equal(ids.cpu().numpy().reshape(-1, 5), want["ray_hit"])
        assert env.range_scan(torch.as_tensor(dirs, device=gpu_device), y.MAX_RANGE).data_ptr() == env.range_scan(dirs, y.MAX_RANGE, frame="level").data_ptr()
        assert env.clearance().dist.data_ptr() == first                        # the tensors are reused
        assert np.isfinite(want["clear4"]).all() and (want["ray_hit"] >= 0).any()
    with pytest.raises(ValueError, match="frame"):
        env.range_scan(dirs, 5.0, frame="nose")
    with pytest.raises(ValueError, match="max_range"):
        env.range_scan(dirs, 0.0)
    with pytest.raises(ValueError, match="aviaries"):
        env.set_obstacles(ob.ObstacleField(E + 1).floor())


def test_swarm_aviary_methods_are_the_entry_on_its_state(gpu_device):
    from gym_pybullet_drones_amd import obstacles as ob
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    n = 70
    rng = np.random.default_rng(4)
    xyz = rng.uniform([-3, -3, 0.3], [3, 3, 2.5], size=(n, 3))
    env = SwarmAviary(n, initial_xyzs=xyz, physics=Physics.DYN, device=gpu_device)
    env.reset()
    rpm = torch.full((n, 4), float(env.HOVER_RPM), device=gpu_device)
    rpm[:, 1] *= 1.04
    for _ in range(10):
        env.step(rpm)
    field = ob.ObstacleField().floor(0.0).box((0, 0, 1), (0.5, 1.0, 1.0)).sphere((2, 2, 1.5), 0.6).none().cylinder((-2, 1, 1), 0.4, 1.0)
    env.set_obstacles(field)
    dirs = ob.fan(16, 2 * np.pi)
    want = _entry_on(env.core.positions(n), env.core.quaternions(n), 0, field, dirs, 2, env.COLLISION_R, gpu_device)
    c = env.clearance()
    assert c.normal.shape == (n, 3) and c.dist.shape == (n,)
    np.testing.assert_array_equal(torch.cat([c.normal, c.dist.unsqueeze(-1)], dim=-1).cpu().numpy().view(np.uint32), want["clear4"].view(np.uint32))
    np.testing.assert_array_equal(c.nearest.cpu().numpy(), want["nearest"])
    np.testing.assert_array_equal(env.obstacle_hits().cpu().numpy(), want["hit"].astype(bool))
    ranges, ids = env.range_scan(dirs, y.MAX_RANGE, want_ids=True)
    np.testing.assert_array_equal(ranges.cpu().numpy().view(np.uint32), want["ranges"].view(np.uint32))
    np.testing.assert_array_equal(ids.cpu().numpy(), want["ray_hit"])
    assert (want["ray_hit"] >= 0).any() and (want["ray_hit"] < 0).any() and len(np.unique(want["nearest"])) > 1


def test_avoid_example(gpu_device):
    spec = importlib.util.spec_from_file_location("example_avoid", os.path.join(REPO, "examples", "avoid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    blind, steered = mod.run(drones=128, device=gpu_device)
    assert 0.0 <= steered < blind <= 1.0

"""Neighbour queries on the MI355X: `gpd_neighbors` and the methods built on it against the reference's matrices, an exact
brute force on inputs whose fp32 arithmetic is exact, float64 on random inputs, and the edges."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from test_host_neighbors import brute_force

pytestmark = pytest.mark.gpu


def _pos4(pos, dev):
    p = torch.zeros((len(pos), 4), dtype=torch.float32, device=dev)
    p[:, :3] = torch.as_tensor(np.asarray(pos), dtype=torch.float32, device=dev)
    return p


def _world(pos, radius, k, dev, cell=0.0, box=None, first=0, count=None, search=None):
    """the entry on an (n, 3) array as ONE world -> numpy (count, idx, rel)"""
    from gym_pybullet_drones_amd import neighbors as nb
    p = _pos4(pos, dev)
    n = len(pos)
    if box is None:
        f = np.asarray(pos, dtype=np.float64)
        f = f[np.isfinite(f).all(axis=1)]
        box = (f[:, 0].min(), f[:, 1].min(), f[:, 0].max(), f[:, 1].max()) if len(f) else (0.0, 0.0, 1.0, 1.0)
    q = search or nb.WorldSearch(dev, n, first, n - first if count is None else count, radius, k, box, cell=cell)
    o = q(p, None)
    torch.cuda.synchronize()
    return o.count.cpu().numpy(), o.idx.cpu().numpy(), o.rel.cpu().numpy()


def _aviaries(pos, E, D, radius, k, dev, adjacency=False):
    from gym_pybullet_drones_amd import neighbors as nb
    o, adj = nb.aviary_query(_pos4(pos, dev), E, D, radius, k, None, want_adjacency=adjacency)
    torch.cuda.synchronize()
    return o.count.cpu().numpy(), o.idx.cpu().numpy(), o.rel.cpu().numpy(), None if adj is None else adj.cpu().numpy()


def _exact(pos32, radius, k, chunk=512):
    """The brute force for inputs whose squared distances are exact in fp32 (so float64 and fp32 agree on every decision):
    `(count, idx [n, k], rel [n, k, 4] float32)`, ordered by (squared distance, row)."""
    p = np.asarray(pos32, dtype=np.float64)
    n = len(p)
    count = np.zeros(n, dtype=np.int64)
    idx = np.full((n, k), -1, dtype=np.int64)
    rel = np.zeros((n, k, 4), dtype=np.float32)
    rel[..., 3] = np.inf
    r2 = float(radius) ** 2
    for lo in range(0, n, chunk):
        d2 = ((p[lo:lo + chunk, None, :] - p[None, :, :]) ** 2).sum(axis=-1)
        for a in range(d2.shape[0]):
            i = lo + a
            js = np.flatnonzero(d2[a] < r2)
            js = js[js != i]
            count[i] = len(js)
            js = js[np.lexsort((js, d2[a, js]))][:k]
            idx[i, :len(js)] = js
            rel[i, :len(js), :3] = (p[js] - p[i]).astype(np.float32)
            rel[i, :len(js), 3] = np.sqrt(d2[a, js].astype(np.float32))
    return count, idx, rel


def _lattice(n=8192):
    rng = np.random.default_rng(0)
    xy = rng.integers(0, 4096, (n, 2)) / 64
    z = rng.integers(0, 512, (n, 1)) / 64
    return np.concatenate([xy, z], axis=1)


def _same_bits(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(np.ascontiguousarray(got[2], dtype=np.float32).view(np.int32),
                                  np.ascontiguousarray(want[2], dtype=np.float32).view(np.int32))


# ---- 1. the reference's matrices ---------------------------------------------------------------------------------------------
def test_reference_adjacency_fixture(gpu_device):
    from gym_pybullet_drones_amd.envs import SwarmAviary, VectorCtrlAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    g = golden("adjacency_ctrl24")
    r = float(g["radius"])
    vec = VectorCtrlAviary(1, 24, initial_xyzs=g["pos"][0], neighbourhood_radius=r, device=gpu_device)
    assert vec.NEIGHBOURHOOD_RADIUS == r
    vec.reset()
    swarm = SwarmAviary(24, initial_xyzs=g["pos"][0], physics=Physics.DYN, device=gpu_device)
    swarm.reset()
    off = ~np.eye(24, dtype=bool)
    for pos, want in zip(g["pos"], g["adjacency"]):
        p = torch.as_tensor(pos, dtype=torch.float32, device=gpu_device)
        vec.core.kin_P[:24, :3] = p
        swarm.core.kin_P[:24, :3] = p
        swarm.invalidate()
        adj = vec.adjacency().cpu().numpy()
        assert adj.shape == (1, 24, 24) and adj.dtype == np.uint8
        np.testing.assert_array_equal(adj[0], want)
        for nb in (vec.neighbors(k=32), swarm.neighbors(r, k=32)):
            count, idx = nb.count.cpu().numpy().reshape(24), nb.idx.cpu().numpy().reshape(24, 32)
            mask = nb.mask.cpu().numpy().reshape(24, 32)
            np.testing.assert_array_equal(count, want.sum(axis=1) - 1)
            for i in range(24):
                got = idx[i][mask[i]]
                assert len(got) == len(set(got)) and set(got) == set(np.flatnonzero(want[i].astype(bool) & off[i]))


# ---- 2. exact inputs, exact answer -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice_truth():
    pos = _lattice()
    return pos, _exact(pos, 2.5, 32)


def test_lattice_world_is_the_brute_force_element_for_element(gpu_device, lattice_truth):
    pos, (count, idx, rel) = lattice_truth
    assert len(np.unique(pos, axis=0)) == len(pos) and count.max() <= 32 and count.min() == 0 and (count > 16).mean() > 0.2
    d16 = rel[:, :16, 3]
    assert (np.isfinite(d16[:, 1:]) & (d16[:, 1:] == d16[:, :-1])).any(axis=1).sum() >= 10          # exact ties inside the lists
    for k in (4, 16, 32):
        _same_bits(_world(pos, 2.5, k, gpu_device), (count, idx[:, :k], rel[:, :k]))


def test_lattice_as_aviaries_is_the_per_aviary_brute_force(gpu_device, lattice_truth):
    pos, _ = lattice_truth
    want = [_exact(pos[e * 64:(e + 1) * 64], 2.5, 32) for e in range(128)]
    count, idx, rel = (np.stack([w[j] for w in want]) for j in range(3))
    assert count.max() > 0
    for k in (4, 16, 32):
        got = _aviaries(pos, 128, 64, 2.5, k, gpu_device, adjacency=True)
        _same_bits(got[:3], (count, idx[:, :, :k], rel[:, :, :k]))
        for e in (0, 77, 127):
            np.testing.assert_array_equal(got[3][e], brute_force(pos[e * 64:(e + 1) * 64], 2.5, 1)[3])
    # (64 drones of a 64 m world hardly see each other.)  The same drones folded into 8 m cubes -- still on the lattice -- have
    # eight neighbours each: lists that truncate at k = 4, aviaries of 48 and of 256 rows (several per workgroup / one)
    dense = pos % 8.0
    for D in (48, 64, 256):
        E = (len(dense) // D)
        want = [_exact(dense[e * D:(e + 1) * D], 2.5, 32) for e in range(E)]
        count, idx, rel = (np.stack([w[j] for w in want]) for j in range(3))
        assert count.max() > 8
        for k in (4, 32):
            _same_bits(_aviaries(dense[:E * D], E, D, 2.5, k, gpu_device)[:3], (count, idx[:, :, :k], rel[:, :, :k]))


# ---- 3. independence of the binning ------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_numbering_cell_size_or_visit_order(gpu_device, lattice_truth):
    from gym_pybullet_drones_amd import neighbors as nb
    pos, (count, idx, rel) = lattice_truth
    base = _world(pos, 2.5, 16, gpu_device)
    for cell in (2.6, 4.0, 7.3, 40.0):
        _same_bits(_world(pos, 2.5, 16, gpu_device, cell=cell), base)
    _same_bits(_world(pos, 2.5, 16, gpu_device, box=(10.0, 20.0, 30.0, 25.0)), base)        # most drones outside the box: wrapped
    # renumbered: drone perm[i] sits in row i.  Ties are broken by ROW, so the lists are compared as sets of equal distance
    perm = np.random.default_rng(5).permutation(len(pos))
    c2, i2, r2 = _world(pos[perm], 2.5, 32, gpu_device)
    np.testing.assert_array_equal(c2, count[perm])
    back = np.where(i2 >= 0, perm[np.clip(i2, 0, None)], -1)
    np.testing.assert_array_equal(r2[..., 3].view(np.int32), rel[perm][..., 3].view(np.int32))
    np.testing.assert_array_equal(np.sort(back, axis=1), np.sort(idx[perm], axis=1))        # (k = 32 holds every list completely)
    # one search object used again and again while the drones move: it visits the rows in the order the PREVIOUS call's sort
    # left (stale), a fresh one visits them in row order
    rng = np.random.default_rng(6)
    q = nb.WorldSearch(gpu_device, len(pos), 0, len(pos), 2.5, 16, (0.0, 0.0, 64.0, 64.0))
    moved = pos.copy()
    for _ in range(4):
        moved = moved + rng.integers(-64, 65, moved.shape) / 64            # (still on the lattice: still exact)
        got = _world(moved, 2.5, 16, gpu_device, search=q)
        got = tuple(np.array(a) for a in got)
        _same_bits(got, _world(moved, 2.5, 16, gpu_device))
    _same_bits(got, _exact(moved, 2.5, 16))


# ---- 4. random positions against float64 -------------------------------------------------------------------------------------
def test_random_world_against_float64(gpu_device):
    """65 536 drones uniform in 181 x 181 x 8 m, radius 2.5, k = 16, against float64 (scipy's cKDTree on the same float32 values).
    Every drone: the distance lists agree to rtol 1e-6, every index points at a drone at the reported distance, and the count
    differs by at most the number of its pairs within 1e-5 r of the radius.  The largest relative distance error is printed:
    1.64e-7 on the MI355X (864 204 list entries; 62 drones have a pair inside the band) -- the fp32 rounding of a squared distance
    and its root, six times below the rule, not orders of magnitude."""
    from scipy.spatial import cKDTree
    n, r, k = 65536, 2.5, 16
    rng = np.random.default_rng(1)
    pos32 = (rng.uniform(0, 1, (n, 3)) * [181.0, 181.0, 8.0]).astype(np.float32)
    pos = pos32.astype(np.float64)
    count, idx, rel = _world(pos32, r, k, gpu_device)
    tree = cKDTree(pos)
    d64, i64 = tree.query(pos, k=k + 1)
    assert (i64[:, 0] == np.arange(n)).all()
    d64 = np.where(d64[:, 1:] < r, d64[:, 1:], np.inf)
    c64 = tree.query_ball_point(pos, r, return_length=True) - 1
    band = tree.query_ball_point(pos, r * (1 + 1e-5), return_length=True) - tree.query_ball_point(pos, r * (1 - 1e-5), return_length=True)
    assert np.all(np.abs(count - c64) <= band), int((np.abs(count - c64) > band).sum())
    dg = rel[..., 3].astype(np.float64)
    both = np.isfinite(dg) & np.isfinite(d64)
    err = np.abs(dg[both] - d64[both]) / d64[both]
    print(f"\nrandom world: {int(both.sum())} list entries, largest relative distance error {err.max():.3e}; "
          f"{int((band > 0).sum())} drones with a pair within 1e-5 r of the radius; mean count {count.mean():.2f}")
    assert err.max() <= 1e-6
    one = np.isfinite(dg) != np.isfinite(d64)            # an entry only one side has: a pair on the radius, inside the band
    lone = np.where(np.isfinite(dg), dg, d64)[one]
    assert np.all(np.abs(lone - r) < 1e-5 * r) and np.all(one.sum(axis=1) <= band)
    # every index: the float64 distance to THAT drone is the reported one; the relative position is the fp32 difference
    m = idx >= 0
    assert (m == np.isfinite(dg)).all() and (m.sum(axis=1) == np.minimum(count, k)).all()
    ii, kk = np.nonzero(m)
    jj = idx[ii, kk]
    true = np.linalg.norm(pos[jj] - pos[ii], axis=1)
    assert np.all(np.abs(dg[ii, kk] - true) <= 1e-6 * true)
    np.testing.assert_array_equal(rel[ii, kk, :3], pos32[jj] - pos32[ii])
    with np.errstate(invalid="ignore"):                  # (inf - inf in the padding)
        assert (jj != ii).all() and np.all(np.diff(dg, axis=1)[np.isfinite(dg[:, 1:])] >= 0)
    assert (rel[~m] == np.array([0, 0, 0, np.inf], dtype=np.float32)).all()


# ---- 5. non-finite rows and the edges ----------------------------------------------------------------------------------------
def test_non_finite_rows_take_no_part(gpu_device):
    rng = np.random.default_rng(2)
    pos = np.concatenate([rng.integers(0, 1024, (3000, 2)) / 64, rng.integers(0, 256, (3000, 1)) / 64], axis=1)
    bad = rng.permutation(3000)[:200]
    holes = pos.copy()
    holes[bad[:100], 0] = np.nan
    holes[bad[100:150], 2] = np.inf
    holes[bad[150:], 1] = -np.inf
    keep = np.setdiff1d(np.arange(3000), bad)
    count, idx, rel = _world(holes, 1.5, 16, gpu_device)
    wc, wi, wr = _exact(pos[keep], 1.5, 16)
    assert (count[bad] == 0).all() and (idx[bad] == -1).all() and np.isinf(rel[bad][..., 3]).all() and (rel[bad][..., :3] == 0).all()
    np.testing.assert_array_equal(count[keep], wc)
    np.testing.assert_array_equal(idx[keep], np.where(wi >= 0, keep[np.clip(wi, 0, None)], -1))
    np.testing.assert_array_equal(rel[keep].view(np.int32), wr.view(np.int32))
    # the same rows as aviaries of 30
    count, idx, rel, adj = _aviaries(holes, 100, 30, 1.5, 8, gpu_device, adjacency=True)
    for e in (0, 13, 99):
        c, i, d, a = brute_force(holes[e * 30:(e + 1) * 30], 1.5, 8)
        np.testing.assert_array_equal(count[e], c)
        np.testing.assert_array_equal(idx[e], i)
        np.testing.assert_array_equal(adj[e], a)


def test_edges(gpu_device):
    # a drone alone in the world
    count, idx, rel = _world([[1.0, 2.0, 3.0]], 2.5, 4, gpu_device)
    assert count.tolist() == [0] and (idx == -1).all() and np.isinf(rel[0, :, 3]).all()
    # exactly the radius apart: not neighbours (strictly below, envs/BaseAviary.py:673); one lattice step closer: neighbours
    count, idx, _ = _world([[0.0, 0.0, 1.0], [2.5, 0.0, 1.0], [0.0, 10.0, 1.0], [0.0, 12.484375, 1.0]], 2.5, 4, gpu_device)
    assert count.tolist() == [0, 0, 1, 1] and idx[2, 0] == 3 and idx[3, 0] == 2
    count, idx, _, adj = _aviaries([[0.0, 0.0, 1.0], [2.5, 0.0, 1.0], [0.0, 10.0, 1.0], [0.0, 12.484375, 1.0]], 2, 2, 2.5, 1, gpu_device, True)
    assert count.tolist() == [[0, 0], [1, 1]] and adj.tolist() == [[[1, 0], [0, 1]], [[1, 1], [1, 1]]]
    # two drones at the same position: distance 0, neighbours, the lower row first
    same = [[5.0, 5.0, 1.0], [6.0, 5.0, 1.0], [5.0, 5.0, 1.0], [5.0, 5.0, 1.0]]
    count, idx, rel = _world(same, 2.5, 4, gpu_device)
    assert count.tolist() == [3, 3, 3, 3]
    assert idx[:, :3].tolist() == [[2, 3, 1], [0, 2, 3], [0, 3, 1], [0, 2, 1]] and (idx[:, 3] == -1).all()
    assert rel[0, 0].tolist() == [0.0, 0.0, 0.0, 0.0] and rel[0, 2].tolist() == [1.0, 0.0, 0.0, 1.0]
    # a world narrower than three cells, drones far outside the box, every pair exactly representable: periodic aliasing (x and
    # x + 3 cells share a cell) produces neither false nor duplicate neighbours
    rng = np.random.default_rng(3)
    pos = np.concatenate([rng.integers(-4096, 4096, (2000, 2)) / 16, rng.integers(0, 64, (2000, 1)) / 16], axis=1)
    want = _exact(pos, 8.0, 32)
    assert want[0].max() <= 32 and want[0].max() > 3
    for box in ((0.0, 0.0, 1.0, 1.0), (3.0, -7.0, 3.0, -7.0), (-300.0, -300.0, 300.0, 300.0), (-1.0e6, 0.0, 1.0e6, 10.0)):
        got = _world(pos, 8.0, 32, gpu_device, box=box)
        _same_bits(got, want)
        for i in range(0, 2000, 97):
            assert len(set(got[1][i][got[1][i] >= 0])) == got[0][i]
    # a query range: a rank of a shared world asks for its own slab
    sub = _world(pos, 8.0, 32, gpu_device, first=700, count=450)
    _same_bits(sub, tuple(a[700:1150] for a in want))
    # an infinite radius inside an aviary: everybody
    count, idx, _, adj = _aviaries(pos[:60], 2, 30, np.inf, 32, gpu_device, True)
    assert (count == 29).all() and (adj == 1).all() and (np.sort(idx[0, 4][:29]) == np.delete(np.arange(30), 4)).all()


# ---- 6. the surface ----------------------------------------------------------------------------------------------------------
def _cloud(n, seed=4, side=12.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (n, 3)) * [side, side, 3.0] + [0, 0, 0.5]


def _entry_on_core(env, radius, k):
    pos = env.core.positions(env.NUM_DRONES).cpu().numpy()
    return _world(pos, radius, k, env.device)


def _as_numpy(nb):
    torch.cuda.synchronize()
    return nb.count.cpu().numpy(), nb.idx.cpu().numpy(), nb.rel.cpu().numpy()


@pytest.mark.parametrize("physics", ["DYN", "PYB_DW"])
def test_swarm_neighbors_follow_the_state(gpu_device, physics):
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    n = 1500
    env = SwarmAviary(n, initial_xyzs=_cloud(n), physics=getattr(Physics, physics), device=gpu_device)
    env.reset()
    _same_bits(_as_numpy(env.neighbors(1.0, 8)), _entry_on_core(env, 1.0, 8))
    snap = env.get_state()
    rpm = torch.full((n, 4), float(env.HOVER_RPM), device=gpu_device) * (1 + 0.05 * torch.rand((n, 4), device=gpu_device))
    for _ in range(30):
        env.step(rpm)
    after = _as_numpy(env.neighbors(1.0, 8))
    _same_bits(after, _entry_on_core(env, 1.0, 8))
    assert (after[2] != _as_numpy(env.neighbors(1.0, 8, rel=True))[2]).sum() == 0
    env.set_state(snap)
    back = _as_numpy(env.neighbors(1.0, 8))
    _same_bits(back, _entry_on_core(env, 1.0, 8))
    assert not np.array_equal(back[2], after[2])
    env.core.kin_P[:n, 2] += 0.25 * torch.rand(n, device=gpu_device)       # behind the aviary's back
    env.invalidate()
    _same_bits(_as_numpy(env.neighbors(1.0, 8)), _entry_on_core(env, 1.0, 8))
    # ... and the query leaves the trajectory alone: the same steps with and without queries in between
    ref = SwarmAviary(n, initial_xyzs=_cloud(n), physics=getattr(Physics, physics), device=gpu_device)
    ref.reset(), env.reset()
    for i in range(20):
        a, b = ref.step(rpm)[0], env.step(rpm)[0]
        if i % 3 == 0:
            env.neighbors(1.0, 8), env.collisions()
    assert torch.equal(a, b)


def test_collisions_flag_the_pairs_a_brute_force_finds(gpu_device):
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    n = 4000
    pos = _cloud(n, seed=8, side=6.0)
    env = SwarmAviary(n, initial_xyzs=pos, physics=Physics.DYN, device=gpu_device)
    env.reset()
    p32 = env.core.positions(n).cpu().numpy()
    for dist in (None, 0.3):
        r = 2 * env.COLLISION_R if dist is None else dist
        want = brute_force(p32, r, 1)[0] > 0
        d = np.linalg.norm(p32[:, None].astype(np.float64) - p32[None].astype(np.float64), axis=-1)
        assert np.abs(d[~np.eye(n, dtype=bool)] - r).min() > 1e-6 * r      # nothing fp32 could decide differently
        got = env.collisions(dist).cpu().numpy()
        assert got.dtype == bool and got.shape == (n,) and want.any() and not want.all()
        np.testing.assert_array_equal(got, want)


def test_two_ranks_return_the_rows_of_the_one_rank_answer(gpu_device):
    from gym_pybullet_drones_amd.envs import LocalSwarmGroup, SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    n = 1201
    pos = _cloud(n, seed=9, side=40.0)
    kw = dict(initial_xyzs=pos, physics=Physics.PYB_DW, device=gpu_device)
    one, grp = SwarmAviary(n, **kw), LocalSwarmGroup(n, 2, **kw)
    one.reset(), grp.reset()
    rpm = torch.full((n, 4), float(one.HOVER_RPM), device=gpu_device)
    for phase in range(2):
        want = _as_numpy(one.neighbors(2.0, 8))
        assert want[0].max() > 2
        for e, got in zip(grp.ranks, grp.neighbors(2.0, 8)):
            ids = e.GLOBAL_IDS
            assert not np.array_equal(ids, np.arange(len(ids)))                 # (dealt spatially: not the caller's order)
            _same_bits(_as_numpy(got), tuple(a[ids] for a in want))
        for _ in range(10):
            one.step(rpm), grp.step(rpm)
    halo = LocalSwarmGroup(n, 2, exchange="halo", **kw)
    halo.reset()
    with pytest.raises(ValueError, match="halo"):
        halo.ranks[0].neighbors(2.0)


def test_vector_aviary_neighbors_and_adjacency(gpu_device):
    from gym_pybullet_drones_amd.envs import VectorCtrlAviary, VectorMultiHoverAviary
    E, D = 300, 7
    init = _cloud(D, seed=10, side=1.5)
    env = VectorMultiHoverAviary(E, D, initial_xyzs=init, neighbourhood_radius=0.9, device=gpu_device)
    env.reset()
    act = 0.3 * torch.rand((E, D, 4), device=gpu_device) - 0.1
    for _ in range(5):
        env.step(act)
    pos = env.core.positions(E * D).cpu().numpy().reshape(E, D, 3)
    nb, adj = env.neighbors(), env.adjacency()
    assert nb.idx.shape == (E, D, 6) and nb.rel.shape == (E, D, 6, 4) and adj.shape == (E, D, D)
    count, idx, rel = _as_numpy(nb)
    for e in (0, 150, 299):
        c, i, d, a = brute_force(pos[e], 0.9, 6)
        np.testing.assert_array_equal(count[e], c)
        np.testing.assert_array_equal(idx[e], i)
        np.testing.assert_allclose(rel[e, ..., 3], d, rtol=1e-6)
        np.testing.assert_array_equal(adj[e].cpu().numpy(), a)
    assert (env.adjacency(radius=1e-3).cpu().numpy() == np.eye(D, dtype=np.uint8)).all()
    everybody = VectorCtrlAviary(4, 3, device=gpu_device)                   # the reference's default radius: np.inf
    everybody.reset()
    assert everybody.NEIGHBOURHOOD_RADIUS == np.inf and (everybody.adjacency() == 1).all() and (everybody.neighbors().count == 2).all()
    with pytest.raises(ValueError, match="at least two drones"):
        VectorCtrlAviary(4, 1, device=gpu_device).adjacency()


def test_neighbors_replay_in_a_captured_graph_with_a_step(gpu_device):
    """A step and a neighbour query captured as ONE linear chain on one stream; every replay answers for the state it left."""
    from gym_pybullet_drones_amd.envs import SwarmAviary
    from gym_pybullet_drones_amd.utils.enums import Physics
    n = 2000
    env = SwarmAviary(n, initial_xyzs=_cloud(n, seed=11), physics=Physics.DYN, device=gpu_device)
    env.reset()
    rpm = torch.full((n, 4), float(env.HOVER_RPM), device=gpu_device) * (1 + 0.05 * torch.rand((n, 4), device=gpu_device))
    stream = torch.cuda.Stream(device=gpu_device)
    stream.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(stream):
        for _ in range(3):                                   # warm-up: allocations happen outside the capture
            env.step(rpm)
            env.neighbors(1.0, 8)
    torch.cuda.current_stream(gpu_device).wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        vec = env.step(rpm)[0]
        out = env.neighbors(1.0, 8)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = tuple(np.array(a) for a in _as_numpy(out))
        assert np.array_equal(vec[:, :3].cpu().numpy(), env.core.positions(n).cpu().numpy())
        _same_bits(got, _entry_on_core(env, 1.0, 8))
    assert got[0].max() > 0


def test_flock_example_collides_less_with_the_rule(gpu_device):
    spec = importlib.util.spec_from_file_location("example_flock", os.path.join(REPO, "examples", "flock.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    blind, ruled = mod.run(drones=256, duration_sec=3, device=gpu_device)
    assert blind > 0 and ruled < blind

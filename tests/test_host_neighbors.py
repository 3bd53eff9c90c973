"""Neighbour queries, the part that needs no GPU: the export and its argument checks (all before the first device call), the
argument errors of the Python methods, and the test suite's own yardstick -- a float64 brute force -- pinned to the matrices the
reference's `_getAdjacencyMatrix` produced (tests/golden/adjacency_ctrl24.npz, tests/golden/make_golden_adjacency.py)."""
import ctypes

import numpy as np
import pytest

from conftest import golden


def brute_force(pos, radius, k):
    """float64 yardstick for one world / one aviary: `(count [n], idx [n, k], dist [n, k], adjacency [n, n])` -- neighbour =
    distance STRICTLY below the radius (envs/BaseAviary.py:673), the list ordered by (squared distance, row), diagonal 1.
    Rows with a non-finite position take no part."""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    fin = np.isfinite(pos).all(axis=1)
    with np.errstate(invalid="ignore"):                  # (inf - inf of two rows without a position)
        diff = pos[:, None, :] - pos[None, :, :]
        d2 = (diff ** 2).sum(axis=-1)
    near = (d2 < float(radius) ** 2) & fin[:, None] & fin[None, :]
    np.fill_diagonal(near, False)
    count = near.sum(axis=1)
    idx = np.full((n, k), -1, dtype=np.int64)
    dist = np.full((n, k), np.inf)
    for i in range(n):
        js = np.flatnonzero(near[i])
        js = js[np.lexsort((js, d2[i, js]))][:k]
        idx[i, :len(js)] = js
        dist[i, :len(js)] = np.sqrt(d2[i, js])
    adj = near.astype(np.uint8)
    np.fill_diagonal(adj, 1)
    return count, idx, dist, adj


def test_brute_force_reproduces_the_reference_matrices():
    g = golden("adjacency_ctrl24")
    r = float(g["radius"])
    assert g["pos"].shape[1:] == (24, 3) and len(g["steps"]) >= 5
    for pos, want in zip(g["pos"], g["adjacency"]):
        count, idx, dist, adj = brute_force(pos, r, 23)
        np.testing.assert_array_equal(adj, want)
        np.testing.assert_array_equal(count, want.sum(axis=1) - 1)
        off = want.astype(bool) & ~np.eye(24, dtype=bool)
        assert off.any() and (~want.astype(bool)).any()                       # neither empty nor full
        for i in range(24):
            assert set(idx[i][idx[i] >= 0]) == set(np.flatnonzero(off[i]))
        d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
        assert np.abs(d[~np.eye(24, dtype=bool)] - r).min() > 1e-4           # no pair a float32 restatement could decide differently


def _entry():
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    assert "gpd_neighbors" in _native.exported_symbols() and L.gpd_abi_version() == 9
    return _native, L


def test_entry_rejects_bad_arguments_before_touching_a_device():
    """Every argument error of gpd_neighbors is found before the first HIP call: the code include/gpd.h states and a message that
    starts with the entry's name (host buffers stand in for device memory: nothing is launched)."""
    _native, L = _entry()
    buf = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ok = dict(pos4=base, n_rows=64, query_first=0, query_count=64, radius=1.0, k=8, drones_per_env=0, cell=0.0, x0=0.0, y0=0.0,
              x1=10.0, y1=10.0, visit_order=None, cell_count=base + 4096, cell_start=base + 8192, order=base + 12288,
              sorted_xyzc=base + 16384, nbr_count=base + 20480, nbr_idx=None, nbr_rel=None, adjacency=None)

    def rc(**change):
        a = {**ok, **change}
        return L.gpd_neighbors(*[a[n] for n in ok], None)

    def rejected(code, **change):
        assert rc(**change) == code, change
        assert L.gpd_last_error().decode().startswith("gpd_neighbors"), change

    EINVAL, ERANGE = _native.GPD_EINVAL, _native.GPD_ERANGE
    rejected(EINVAL, pos4=None)
    rejected(EINVAL, nbr_count=None)
    rejected(EINVAL, n_rows=0)
    for k in (0, -1, 33):
        rejected(ERANGE, k=k)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        rejected(EINVAL, radius=r)
    rejected(ERANGE, query_first=-1)
    rejected(ERANGE, query_count=0)
    rejected(ERANGE, query_first=1)                        # 1 + 64 > 64
    rejected(ERANGE, query_first=2 ** 31 - 1, query_count=2 ** 31 - 1, n_rows=2 ** 31 - 1)
    rejected(EINVAL, pos4=base + 4)                        # not 16-byte aligned
    rejected(EINVAL, nbr_rel=base + 24576 + 8)
    rejected(EINVAL, adjacency=base + 24576)               # one world has no dense matrix
    for d in (1, -2, 257):
        rejected(EINVAL, drones_per_env=d)
    rejected(EINVAL, drones_per_env=6)                     # 64 rows are not whole aviaries of 6
    rejected(EINVAL, drones_per_env=16, query_first=8, query_count=16)
    for name in ("cell_count", "cell_start", "order", "sorted_xyzc"):
        rejected(EINVAL, **{name: None})
    rejected(EINVAL, visit_order=ok["order"])
    rejected(EINVAL, x1=-1.0)
    rejected(EINVAL, y0=float("nan"))
    rejected(EINVAL, cell=-1.0)


def test_python_methods_reject_bad_arguments_before_any_device_work():
    from gym_pybullet_drones_amd import neighbors as nb
    from gym_pybullet_drones_amd.envs.SwarmAviary import SwarmAviary
    from gym_pybullet_drones_amd.envs.VectorAviary import VectorAviary
    for k in (0, 33, -1):
        with pytest.raises(ValueError, match="k must be"):
            nb.check_args(1.0, k)
    for r in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            nb.check_args(r, 4)
    assert nb.check_args(float("inf"), 4) == (np.finfo(np.float32).max, 4)    # "everybody": the largest finite float
    # (objects without a core: the checks come before anything touches a device)
    halo = object.__new__(SwarmAviary)
    halo._halo = True
    with pytest.raises(ValueError, match="halo"):
        halo.neighbors(1.0)
    with pytest.raises(ValueError, match="halo"):
        halo.collisions(0.1)
    world = object.__new__(SwarmAviary)
    world._halo = False
    with pytest.raises(ValueError, match="k must be"):
        world.neighbors(1.0, k=64)
    single = object.__new__(VectorAviary)
    single.NUM_ENVS, single.NUM_DRONES, single.NEIGHBOURHOOD_RADIUS = 4, 1, np.inf
    with pytest.raises(ValueError, match="at least two drones"):
        single.neighbors()
    with pytest.raises(ValueError, match="at least two drones"):
        single.adjacency(1.0)
    multi = object.__new__(VectorAviary)
    multi.NUM_ENVS, multi.NUM_DRONES, multi.NEIGHBOURHOOD_RADIUS = 4, 3, np.inf
    with pytest.raises(ValueError, match="k must be"):
        multi.neighbors(k=40)
    with pytest.raises(ValueError, match="radius"):
        multi.adjacency(radius=-1.0)


def test_new_kernels_need_no_scratch_memory():
    """`-Rpass-analysis=kernel-resource-usage` on the one-world unit: every instantiation of the two neighbour kernels (K = 4, 8, 16,
    32 keys in registers, all indices compile-time constants) reports ScratchSize 0."""
    import os
    import re
    import subprocess
    import tempfile
    from gym_pybullet_drones_amd import _native
    from conftest import REPO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    unit, extra = next(u for u in _native.UNITS if u[0] == "swarm.hip")
    flags = [f for f in _native.COMMON_FLAGS if f != "-fPIC"] + extra
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I",
                                                os.path.join(REPO, "include"), os.path.join(_native.CSRC, unit), "-o", os.path.join(d, "u.s")],
                             check=True, capture_output=True, text=True)
    found = {}
    name = None
    for line in res.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and ("nbr_world_kernel" in name or "nbr_env_kernel" in name):
            found[name] = int(m.group(1))
    assert len(found) == 8, sorted(found)
    assert all(v == 0 for v in found.values()), found

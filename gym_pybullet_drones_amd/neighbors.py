"""Neighbour queries on the device: the binding of `gpd_neighbors` (include/gpd.h) shared by `SwarmAviary.neighbors()` /
`collisions()` and `VectorAviary.neighbors()` / `adjacency()`.

The reference has `BaseAviary._getAdjacencyMatrix()` (`envs/BaseAviary.py:658-675`): an O(N^2) Python loop over the pairs of one
aviary on the host.  Here a drone gets the NUMBER of other drones closer than `radius` and the nearest `k` of them, ordered by
(squared distance, row) -- ties go to the lower row, whatever the sort did -- as device tensors, with no host synchronisation.
"""
import math

import torch

from . import _native

MAX_K = 32
#: entries of the sort's scratch arrays (include/gpd.h: the grid has at most 65 536 cells, whatever the entry chooses)
_KEYS = 65536
_FLT_MAX = 3.4028234663852886e38


def check_args(radius, k) -> tuple:
    """`(radius, k)` as the entry takes them, or ValueError -- before any device work.  An infinite radius ("everybody": the
    reference's default NEIGHBOURHOOD_RADIUS) becomes the largest finite float."""
    radius = float(radius)
    if math.isnan(radius) or not radius > 0.0:
        raise ValueError(f"radius must be positive, got {radius}")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
    return min(radius, _FLT_MAX), k


class Neighbors:
    """What a neighbour query returns (device tensors, shapes `(..., k)`):
    `idx`   int32: the nearest `min(k, count)` other drones within the radius, nearest first; the rest -1
    `count` int32: how many other drones are within the radius, however many (may exceed k)
    `rel`   float32 `(..., k, 4)`: (xj - xi, yj - yi, zj - zi, distance) of those entries, padding (0, 0, 0, +inf); None if not asked for
    `mask`  bool: `idx >= 0`"""
    __slots__ = ("idx", "count", "rel")

    def __init__(self, idx, count, rel):
        self.idx, self.count, self.rel = idx, count, rel

    @property
    def mask(self):
        return self.idx >= 0


class WorldSearch:
    """One world (`drones_per_env = 0`): the scratch of the counting sort and the output tensors of one (radius, k), allocated
    once; every call sorts the rows of `pos4` by grid cell and searches.  The sort visits the rows in the order the previous call
    left (two `order` buffers in turn: neighbouring lanes then share a cell and the sort issues one atomic per run of equal cells)."""

    def __init__(self, device, n_rows: int, query_first: int, query_count: int, radius: float, k: int, box, rel: bool = True,
                 cell: float = 0.0):
        self.radius, self.k = check_args(radius, k)
        self.device, self.n_rows, self.qf, self.qc = device, int(n_rows), int(query_first), int(query_count)
        self.box, self.cell = tuple(float(v) for v in box), float(cell)
        i32 = dict(dtype=torch.int32, device=device)
        self._count, self._start = torch.zeros(2 * (_KEYS + 1), **i32), torch.zeros(_KEYS + 1, **i32)
        self._order, self._visit = torch.arange(self.n_rows, **i32), torch.arange(self.n_rows, **i32)
        self._sorted = torch.zeros((self.n_rows, 4), dtype=torch.float32, device=device)
        self.out = Neighbors(torch.full((self.qc, self.k), -1, **i32), torch.zeros(self.qc, **i32),
                             torch.zeros((self.qc, self.k, 4), dtype=torch.float32, device=device) if rel else None)

    def __call__(self, pos4: torch.Tensor, stream) -> Neighbors:
        self._order, self._visit = self._visit, self._order
        o = self.out
        _native.call("gpd_neighbors", self.device, stream, pos4, self.n_rows, self.qf, self.qc, self.radius, self.k, 0, self.cell, *self.box,
                     self._visit, self._count, self._start, self._order, self._sorted, o.count, o.idx, o.rel, None)
        return o


def aviary_query(pos4: torch.Tensor, num_envs: int, drones_per_env: int, radius, k: int, stream, rel: bool = True,
                 want_adjacency: bool = False):
    """E aviaries of D consecutive rows of `pos4` (`drones_per_env = D`, 2 .. 256): `(Neighbors, adjacency)` with shapes
    `(E, D, k)` / `(E, D)` / `(E, D, k, 4)` and `(E, D, D)` uint8 (None unless asked for).  `idx` counts inside the aviary."""
    E, D = int(num_envs), int(drones_per_env)
    if not 2 <= D <= 256:
        raise ValueError(f"neighbour queries inside an aviary need 2..256 drones per aviary, got {D}")
    radius, k = check_args(radius, k)
    dev = pos4.device
    idx = torch.empty((E, D, k), dtype=torch.int32, device=dev)
    count = torch.empty((E, D), dtype=torch.int32, device=dev)
    relt = torch.empty((E, D, k, 4), dtype=torch.float32, device=dev) if rel else None
    adj = torch.empty((E, D, D), dtype=torch.uint8, device=dev) if want_adjacency else None
    _native.call("gpd_neighbors", dev, stream, pos4, E * D, 0, E * D, radius, k, D, 0.0, 0.0, 0.0, 0.0, 0.0, None, None, None, None, None,
                 count, idx, relt, adj)
    return Neighbors(idx, count, relt), adj

"""CPU oracle of the flight field (csrc/flight.hip, gnbv_flight_field / gnbv_flight_path).  Test infrastructure.

Dijkstra with heapq over the 26-connected lattice and the SAME integer edge costs (millimetres) the kernel gets: another
algorithm than the kernel's in-place relaxation, and with integer sums the two must agree on every u32.  Node id
c = (k ny + j) nx + i; blocked nodes and nodes no route reaches hold INF.
"""
from __future__ import annotations

import heapq

import numpy as np

INF = 0xFFFFFFFF
# the kernel's neighbour order: dz, dy, dx in (-1, 0, 1), dx fastest
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def cost_index(dx, dy, dz):
    return (dx != 0) | ((dy != 0) << 1) | ((dz != 0) << 2)


def neighbours(c, dims):
    """[(node, cost index)] of node c's in-bounds neighbours, in the kernel's order."""
    nx, ny, nz = dims
    i, j, k = c % nx, (c // nx) % ny, c // (nx * ny)
    out = []
    for dx, dy, dz in OFFSETS:
        a, b, d = i + dx, j + dy, k + dz
        if 0 <= a < nx and 0 <= b < ny and 0 <= d < nz:
            out.append(((d * ny + b) * nx + a, cost_index(dx, dy, dz)))
    return out


def dijkstra(blocked, dims, cost, src):
    """blocked bool [M], cost [8] ints, src a node id or -1 (no node) -> uint32 [M]."""
    m = dims[0] * dims[1] * dims[2]
    blocked = np.asarray(blocked, bool).reshape(m)
    cost = [int(c) for c in cost]
    dist = [INF] * m
    if src < 0 or blocked[src]:
        return np.full(m, INF, np.uint32)
    dist[src] = 0
    heap = [(0, src)]
    free = (~blocked).tolist()
    while heap:
        d, c = heapq.heappop(heap)
        if d > dist[c]:
            continue
        for nb, ci in neighbours(c, dims):
            if free[nb]:
                nd = d + cost[ci]
                if nd < dist[nb]:
                    dist[nb] = nd
                    heapq.heappush(heap, (nd, nb))
    return np.array(dist, np.uint64).astype(np.uint32)


def walk(field, dims, cost, target):
    """The kernel's walk from `target` down the field: node ids target -> source ([] where there is no route)."""
    field = np.asarray(field, np.uint32).astype(np.int64)
    if target < 0 or field[target] == INF:
        return []
    out, cur = [target], target
    while field[cur] != 0:
        for nb, ci in neighbours(cur, dims):
            if field[nb] != INF and field[nb] + int(cost[ci]) == field[cur]:
                cur = nb
                break
        else:
            raise AssertionError(f"node {cur} has no predecessor: not a field")
        out.append(cur)
    return out


def scipy_field(blocked, dims, cost, src):
    """The same table from scipy.sparse.csgraph.dijkstra (cross-check of the heapq oracle)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra as sp_dijkstra
    m = dims[0] * dims[1] * dims[2]
    blocked = np.asarray(blocked, bool).reshape(m)
    rows, cols, w = [], [], []
    for c in range(m):
        if blocked[c]:
            continue
        for nb, ci in neighbours(c, dims):
            if not blocked[nb]:
                rows.append(c)
                cols.append(nb)
                w.append(float(cost[ci]))
    if src < 0 or blocked[src]:
        return np.full(m, INF, np.uint32)
    g = csr_matrix((w, (rows, cols)), shape=(m, m))
    d = sp_dijkstra(g, directed=True, indices=src)
    return np.where(np.isfinite(d), d, float(INF)).astype(np.uint64).astype(np.uint32)


def unpack_bits(words, m):
    """int32 / uint32 [N, W] -> bool [N, m]."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(w.shape[0], -1)[:, :m].astype(bool)


def serpentine(dims):
    """bool [M]: every odd x column is a wall over all y and z, open at alternating ends (y = ny - 1, then y = 0, ...), so the only
    route from (0, 0, *) to the last column snakes through every even column."""
    nx, ny, nz = dims
    b = np.zeros((nz, ny, nx), bool)
    for i in range(1, nx, 2):
        b[:, :, i] = True
        gap = ny - 1 if (i // 2) % 2 == 0 else 0
        b[:, gap, i] = False
    return b.reshape(-1)

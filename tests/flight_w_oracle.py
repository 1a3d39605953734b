"""CPU oracle of the penalised flight field (csrc/flight.hip, gnbv_flight_field_w / gnbv_flight_path_w).  Test infrastructure.

tests/flight_oracle.py's Dijkstra with a price on entering a node: the route's cost is the sum of its integer edge costs plus
`penalty` for every costly node entered (the target included, the source not).  Another algorithm than the kernel's in-place
relaxation; with integer sums (Python ints: nothing wraps) the two must agree on every u32.
"""
from __future__ import annotations

import heapq

import numpy as np

from tests.flight_oracle import INF, neighbours


def dijkstra_w(blocked, costly, dims, cost, src, penalty):
    """blocked, costly bool [M], cost [8] ints, src a node id or -1 (no node), penalty an int -> uint32 [M]."""
    m = dims[0] * dims[1] * dims[2]
    blocked, costly = np.asarray(blocked, bool).reshape(m), np.asarray(costly, bool).reshape(m)
    cost, penalty = [int(c) for c in cost], int(penalty)
    if src < 0 or blocked[src]:
        return np.full(m, INF, np.uint32)
    dist = [INF] * m
    dist[src] = 0
    heap = [(0, src)]
    free, pen = (~blocked).tolist(), [penalty if c else 0 for c in costly.tolist()]
    while heap:
        d, c = heapq.heappop(heap)
        if d > dist[c]:
            continue
        for nb, ci in neighbours(c, dims):
            if free[nb]:
                nd = d + cost[ci] + pen[nb]
                if nd < dist[nb]:
                    dist[nb] = nd
                    heapq.heappush(heap, (nd, nb))
    assert all(d == INF or d < INF - 1 for d in dist)  # the entry point's bound keeps every route below 0xFFFFFFFE
    return np.array(dist, np.uint64).astype(np.uint32)


def scipy_field_w(blocked, costly, dims, cost, src, penalty):
    """The same table from scipy.sparse.csgraph.dijkstra over the DIRECTED graph whose edge u -> v weighs cost + penalty * costly[v]
    (cross-check of the heapq oracle; fp64 holds these integers exactly)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra as sp_dijkstra
    m = dims[0] * dims[1] * dims[2]
    blocked, costly = np.asarray(blocked, bool).reshape(m), np.asarray(costly, bool).reshape(m)
    if src < 0 or blocked[src]:
        return np.full(m, INF, np.uint32)
    rows, cols, w = [], [], []
    for c in range(m):
        if blocked[c]:
            continue
        for nb, ci in neighbours(c, dims):
            if not blocked[nb]:
                rows.append(c)
                cols.append(nb)
                w.append(float(int(cost[ci]) + (int(penalty) if costly[nb] else 0)))
    g = csr_matrix((w, (rows, cols)), shape=(m, m))
    d = sp_dijkstra(g, directed=True, indices=src)
    return np.where(np.isfinite(d), d, float(INF)).astype(np.uint64).astype(np.uint32)


def walk_w(field, costly, dims, cost, penalty, target):
    """The kernel's walk from `target` down a penalised field: from each node the first neighbour, in the kernel's order, with
    field[nb] < field[node] and field[nb] + cost + penalty * costly[node] == field[node].  Node ids target -> source ([] where
    there is no route)."""
    field = [int(v) for v in np.asarray(field, np.uint32)]
    costly = np.asarray(costly, bool).reshape(-1)
    if target < 0 or field[target] == INF:
        return []
    out, cur = [target], target
    while field[cur] != 0:
        pen = int(penalty) if costly[cur] else 0
        for nb, ci in neighbours(cur, dims):
            if field[nb] < field[cur] and field[nb] + int(cost[ci]) + pen == field[cur]:
                cur = nb
                break
        else:
            raise AssertionError(f"node {cur} has no predecessor: not a field")
        out.append(cur)
    return out


def route_cost(path, costly, dims, cost, penalty):
    """The cost of a walked route (node ids target -> source): its edge costs plus the penalties of the nodes entered."""
    costly = np.asarray(costly, bool).reshape(-1)
    total = 0
    for a, b in zip(path[:-1], path[1:]):  # the drone flies b -> a
        ci = dict(neighbours(b, dims))[a]  # KeyError: not 26-adjacent
        total += int(cost[ci]) + (int(penalty) if costly[a] else 0)
    return total

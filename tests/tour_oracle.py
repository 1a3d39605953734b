"""CPU oracle of the tour kernel (csrc/tour.hip, gnbv_tour_route), of FlightField.pairwise_mm and of euclid_mm.  Test
infrastructure.

`route` restates the rule of include/gennbv_hip.h in plain Python loops over Python integers: the route set, nearest neighbour
from point 0 (ties to the lowest index), best-improvement 2-opt on the open path (ties to the lowest i, then the lowest j), the
length, and the status bits.  Everything is integer, so the kernel must agree on every int.  `pairwise` goes over
tests/flight_oracle.dijkstra, another algorithm than the kernel's relaxation.
"""
from __future__ import annotations

import itertools

import numpy as np

from tests import flight_oracle as FO

INF = 0xFFFFFFFF
MISSING_LEG, CAPPED, BAD_COUNT = 1, 2, 4


def route(D, count=None, max_moves=None):
    """D uint32 [P,P] -> (order [P] int32, routed, length, status, moves)."""
    D = np.asarray(D)
    p = D.shape[0]
    d = [[int(v) for v in row] for row in D.astype(np.uint32).tolist()]
    count = p if count is None else int(count)
    max_moves = p * p if max_moves is None else int(max_moves)
    if not 1 <= count <= p:
        return np.arange(p, dtype=np.int32), 1, 0, BAD_COUNT, 0
    members = [j for j in range(1, count) if d[0][j] != INF]
    tail = [j for j in range(1, p) if j not in members]
    seen_inf = False

    def read(a, b):
        nonlocal seen_inf
        v = d[a][b]
        if v == INF:
            seen_inf = True
        return v
    t, left = [0], list(members)
    while left:
        cur = t[-1]
        keys = [(read(cur, j), j) for j in left]  # every unvisited route point is read
        j = min(keys)[1]
        t.append(j)
        left.remove(j)
    r = len(t)
    moves = status = 0
    while True:
        best = None
        for i in range(1, r):
            for j in range(i + 1, r):
                delta = read(t[i - 1], t[j]) - read(t[i - 1], t[i])
                if j + 1 < r:
                    delta += read(t[i], t[j + 1]) - read(t[j], t[j + 1])
                if best is None or (delta, i, j) < best:
                    best = (delta, i, j)
        if best is None or best[0] >= 0:
            break
        if moves >= max_moves:
            status |= CAPPED
            break
        _, i, j = best
        t[i:j + 1] = t[i:j + 1][::-1]
        moves += 1
    length = sum(read(t[q], t[q + 1]) for q in range(r - 1))
    if seen_inf:
        status |= MISSING_LEG
    return np.array(t + tail, np.int32), r, length, status, moves


def route_batch(D, count=None, max_moves=None):
    """D uint32 [N,P,P] -> (order int32 [N,P], routed int32 [N], length int64 [N], status int32 [N])."""
    out = [route(D[e], None if count is None else count[e], max_moves) for e in range(D.shape[0])]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.int64),
            np.array([o[3] for o in out], np.int32))


def path_length(D, seq):
    return sum(int(D[a, b]) for a, b in zip(seq[:-1], seq[1:]))


def brute_force(D):
    """The shortest open path from point 0 through every point (P <= 8)."""
    p = D.shape[0]
    return min(path_length(D, (0,) + q) for q in itertools.permutations(range(1, p)))


def nearest_neighbour_length(D):
    return route(D, max_moves=0)[2]


def stubs_mm(lat, points):
    """rint(1000 * ||p - its nearest node||) in fp64 [..], and the node ids (-1: none)."""
    pts = np.asarray(points)[..., :3].astype(np.float64)
    node = lat.nearest_np(pts)
    pos = lat.node_positions()[np.maximum(node, 0)]
    d = pts - pos
    with np.errstate(invalid="ignore"):
        mm = np.rint(1000.0 * np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))
    return np.where(node >= 0, mm, 0).astype(np.int64), node


def pairwise(lat, blocked, points, count=None):
    """FlightField.pairwise_mm over Dijkstra: blocked bool [N,M], points [N,P,>=3] -> uint32 [N,P,P]."""
    points = np.asarray(points)
    n, p = points.shape[:2]
    stub, node = stubs_mm(lat, points)
    out = np.full((n, p, p), INF, np.uint32)
    for e in range(n):
        c = p if count is None else int(count[e])
        fields = {}
        for a in range(c):
            if node[e, a] < 0:
                continue
            src = int(node[e, a])
            if src not in fields:
                fields[src] = FO.dijkstra(blocked[e], lat.dims, lat.cost, src)
            for b in range(c):
                if a == b:
                    out[e, a, b] = 0
                elif node[e, b] >= 0 and fields[src][node[e, b]] != INF:
                    total = int(fields[src][node[e, b]]) + int(stub[e, a]) + int(stub[e, b])
                    assert total < INF - 1
                    out[e, a, b] = total
    return out


def euclid(points, count=None):
    """euclid_mm: rint(1000 * ||a - b||) in fp64 -> uint32 [N,P,P]."""
    pts = np.asarray(points)[..., :3].astype(np.float64)
    n, p = pts.shape[:2]
    d = pts[:, :, None] - pts[:, None]
    with np.errstate(invalid="ignore"):
        mm = np.rint(1000.0 * np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))
    ok = np.isfinite(mm) & (mm < INF - 1)
    if count is not None:
        inside = np.arange(p)[None] < np.asarray(count)[:, None]
        ok &= inside[:, :, None] & inside[:, None, :]
    return np.where(ok, mm, float(INF)).astype(np.uint64).astype(np.uint32)

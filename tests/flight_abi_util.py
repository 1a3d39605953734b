"""Shared by tests/test_flight_abi_regimes_cpu.py and tests/test_flight_abi_gpu.py: the six entry points of csrc/flight.hip at the
C ABI -- gnbv_flight_field, gnbv_flight_field_w, gnbv_flight_query, gnbv_flight_path, gnbv_flight_path_w and
gnbv_flight_lds_max_nodes -- at every way k_flight_field deals nodes to lanes and past one block of the query and the walk.
TEST INFRASTRUCTURE.

  * the launch shape restated from launch_field and the kernels: nodes per lane, LDS or global table, the tail word, the axes of
    one node, the blocks of the query and path launches; and the nearest-node rule in fp64;
  * the field cases, ids naming the regime, and check_field_case(): from the numbers alone a case reaches what its id names;
  * three mutants of the oracle, each what one plausible slip in the weighted LDS kernel's `mine` register would compute, so that
    the CPU file can show that the cases tell them from the truth;
  * a restatement of one wave's sweep on a line lattice (all loads before any store: a Jacobi step), which pins the sweep cap;
  * the seven distinct 9 x 7 x 5 envs that the query and path cases cycle through, their targets, and the expected rows;
  * raw ctypes callers: every output buffer is filled with 0x5A5A5A5A first and carries GUARD words of the same after its last row.

The oracles are the existing ones, unchanged: tests/flight_oracle.py and tests/flight_w_oracle.py (heapq Dijkstra and walks in
Python ints).  Every comparison built on them is exact.  Only the callers at the end touch the GPU.
"""
import ctypes as C
import functools
import heapq
from types import SimpleNamespace

import numpy as np

from tests import flight_oracle as FO
from tests import flight_w_oracle as WO

f32, f64 = np.float32, np.float64
INF = FO.INF
K_FREE = 0xFFFFFFFE       # kFree: every route sum, and every candidate the kernel forms, stays below it
K_FIELD_LANES = 1024      # kFieldLanes
K_WAVE = 64               # kWave: the path kernel's block
K_QUERY_LANES = 256       # the query kernel's block
K_LDS_HEADER = 16         # kLdsHeader
K_LDS_BYTES = 160 * 1024  # kLdsBytes
K_LDS_DEFAULT = 64 * 1024  # what a launch may ask for before hipFuncSetAttribute
POISON = 0x5A5A5A5A
STATUS_POISON = -7
GUARD = 64                # words after every output
INVALID = 1               # hipErrorInvalidValue
DEV = "cuda:0"


def _ceil(a, b):
    return -(-a // b)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------
# the launch shape, from the numbers alone
# ---------------------------------------------------------------------------
def lds_max_nodes():
    return (K_LDS_BYTES - K_LDS_HEADER) // 4


def field_regime(dims, mode):
    """launch_field and k_flight_field restated: what (nx, ny, nz, mode) decide."""
    assert mode in (0, 1, 2)
    m = dims[0] * dims[1] * dims[2]
    fits = m <= lds_max_nodes()
    refused = mode == 1 and not fits
    lds = not refused and (mode == 1 or (mode == 0 and fits))
    per_lane = _ceil(m, K_FIELD_LANES)
    lds_bytes = K_LDS_HEADER + 4 * m if lds else K_LDS_HEADER
    return SimpleNamespace(m=m, words=_ceil(m, 32), per_lane=per_lane, lds=lds, refused=refused, tail_word=m % 32 != 0,
                           unit_axes=tuple(a for a in range(3) if dims[a] == 1), last_chunk_nodes=m - (per_lane - 1) * K_FIELD_LANES,
                           one_wave=m <= K_WAVE, lds_bytes=lds_bytes, needs_attribute=lds and lds_bytes > K_LDS_DEFAULT,
                           mine_bits=per_lane if lds else 0)  # (the weighted LDS kernel: bits 0 .. per_lane - 1 of `mine`)


def accepted_modes(dims):
    return tuple(mode for mode in (1, 2, 0) if not field_regime(dims, mode).refused)


def path_blocks(n):
    return _ceil(n, K_WAVE)


def query_blocks(n, k):
    return _ceil(n * k, K_QUERY_LANES)


# ---------------------------------------------------------------------------
# lattices, bits, the nearest node
# ---------------------------------------------------------------------------
def edge_costs(h):
    """gennbv_amd/env/flight.py edge_costs: rint(1000 * ||d * h||) millimetres, 0 where every axis of the index has one node."""
    h = np.asarray(h, f64)
    return np.array([int(np.rint(1000.0 * np.sqrt(sum(h[a] ** 2 for a in range(3) if (b >> a) & 1)))) for b in range(8)], np.uint32)


def lattice(dims, unit=(0.2, 0.3, 0.25), lo=(-1.0, 2.0, 0.1), cost=None):
    """What the C ABI needs of a lattice: dims, lo, h (0 on an axis of one node, as FlightLattice has it), the 8 edge costs."""
    dims = tuple(int(d) for d in dims)
    h = np.array([unit[a] if dims[a] > 1 else 0.0 for a in range(3)], f64)
    m = dims[0] * dims[1] * dims[2]
    cost = edge_costs(h) if cost is None else np.array(cost, np.uint32)
    return SimpleNamespace(dims=dims, lo=np.array(lo, f64), h=h, cost=cost, num_nodes=m, words=_ceil(m, 32))


def node_index(lat):
    nx, ny, _ = lat.dims
    c = np.arange(lat.num_nodes, dtype=np.int64)
    return np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], -1)


def node_positions(lat):
    return lat.lo[None] + lat.h[None] * node_index(lat)


def nearest(lat, p):
    """nearest_node of csrc/flight.hip in fp64, the same operations in the same order: per axis clamp(floor((p - lo) / h + 0.5), 0,
    n - 1), 0 on an axis of one node whatever the (finite) coordinate; -1 for a non-finite coordinate."""
    p = np.asarray(p)[..., :3].astype(f64)
    fin = np.isfinite(p).all(-1)
    idx = []
    for a in range(3):
        n = lat.dims[a]
        if n == 1:
            idx.append(np.zeros(p.shape[:-1], np.int64))
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.floor((p[..., a] - lat.lo[a]) / lat.h[a] + 0.5)
        idx.append(np.clip(np.where(fin, f, 0.0), 0, n - 1).astype(np.int64))
    nx, ny, _ = lat.dims
    return np.where(fin, (idx[2] * ny + idx[1]) * nx + idx[0], -1)


def poses_at(lat, nodes, off_axis=123.0):
    """fp32 poses [N, 6] a little off the given nodes (the nearest-node rule has work to do); on an axis of one node the coordinate
    is `off_axis` away: such an axis ignores it."""
    p = np.zeros((len(nodes), 6), f32)
    pos = node_positions(lat)[np.asarray(nodes)] + 0.3 * lat.h * np.array([1, -1, 1])
    pos[:, [a for a in range(3) if lat.dims[a] == 1]] += off_axis
    p[:, :3] = pos
    return p


def pack_words(mask):
    """bool [N, M] -> uint32 [N, ceil(M / 32)], bit c & 31 of word c >> 5; the padding bits SET: they must not be read."""
    mask = np.asarray(mask, bool)
    n, m = mask.shape
    words = _ceil(m, 32)
    full = np.ones((n, words * 32), bool)
    full[:, :m] = mask
    w = (full.reshape(n, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32)


# ---------------------------------------------------------------------------
# the field cases
# ---------------------------------------------------------------------------
def _bound_sum(m):
    """The largest cmax + penalty that M * (cmax + penalty) < 0xFFFFFFFE admits."""
    return (K_FREE - 1) // m


_K64 = _bound_sum(64)  # 67108863: 64 * _K64 = 0xFFFFFFC0
UNIT36 = (0.2, 0.2, 0.2)  # the spacing of the existing threshold tests
# id -> dims, n envs, seed; `line`: nothing blocked and the sources at given nodes; cost / plain_cost: cost[8] of the weighted and the
# plain call where they are not the lattice's own; penalty of the weighted call
FIELD_CASES = {
    "pl1-full-deal-32x32x1": dict(dims=(32, 32, 1), n=2, seed=11),
    "pl2-one-node-chunk-41x25x1": dict(dims=(41, 25, 1), n=2, seed=12),
    "nx1-tail-1x33x31": dict(dims=(1, 33, 31), n=2, seed=13),
    "ny1-tail-33x1x31": dict(dims=(33, 1, 31), n=2, seed=14),
    "line-2-cap": dict(dims=(2, 1, 1), n=2, seed=15, line=(0, 1)),
    "line-64-cap": dict(dims=(64, 1, 1), n=2, seed=16, line=(0, 63)),
    "line-1024-mid": dict(dims=(1024, 1, 1), n=1, seed=17, line=(512,)),
    "pl33-lds-36x36x26": dict(dims=(36, 36, 26), n=1, seed=18, unit=UNIT36),
    "pl40-capacity-36x36x31": dict(dims=(36, 36, 31), n=2, seed=19, unit=UNIT36),
    "above-capacity-36x36x32": dict(dims=(36, 36, 32), n=2, seed=20, unit=UNIT36),
    # every sum at the edge of 32 bits: each hop of the line costs _K64 (env 0: every node entered is costly), the farthest node holds
    # 63 * _K64 > 2^31 and relaxing its neighbour from it forms 64 * _K64 = 0xFFFFFFC0, the closest a candidate comes to wrapping
    "bound-line-64": dict(dims=(64, 1, 1), n=2, seed=21, line=(0, 63), all_costly=(0,), penalty=_K64 - 1000,
                          cost=(0, 1000, 0, 0, 0, 0, 0, 0), plain_cost=(0, _K64, 0, 0, 0, 0, 0, 0)),
    "bound-4x4x4": dict(dims=(4, 4, 4), n=2, seed=22, penalty=1000000,
                        cost=(0, 38167970, 38167971, 53977661, 38167972, 53977662, 53977663, _K64 - 1000000),
                        plain_cost=(0, 38745320, 38745321, 54794156, 38745322, 54794157, 54794158, _K64)),
}
PENALTY = 777
SMALL_DIMS = (9, 7, 5)  # M = 315: the lattice of the kernel-level tests


@functools.lru_cache(maxsize=None)
def field_case(cid):
    """A case's inputs, read-only: lat (weighted costs), plain_lat, blocked / costly bool [n, M], src [n], poses f32 [n, 6], penalty.
    Masks are random at 30 % blocked and 40 % costly; the source is a free node, a third (env 1: two thirds) of the way through
    the free ones."""
    c = FIELD_CASES[cid]
    dims, n = c["dims"], c["n"]
    unit = c.get("unit", (0.2, 0.3, 0.25))
    lat, plain_lat = lattice(dims, unit, cost=c.get("cost")), lattice(dims, unit, cost=c.get("plain_cost", c.get("cost")))
    m, rs = lat.num_nodes, np.random.RandomState(c["seed"])
    blocked, costly = rs.rand(n, m) < 0.3, rs.rand(n, m) < 0.4
    if "line" in c:
        blocked[:] = False
        src = np.array(c["line"])
        if m == 2:  # two nodes: the node entered is costly, the source is not
            costly[np.arange(n), src] = False
            costly[np.arange(n), 1 - src] = True
    else:
        src = np.array([int(np.nonzero(~blocked[e])[0][((e + 1) * int((~blocked[e]).sum())) // 3]) for e in range(n)])
    for e in c.get("all_costly", ()):  # every node entered is costly; the source, which no route enters, is not
        costly[e] = True
        costly[e, src[e]] = False
    assert len(src) == n and not blocked[np.arange(n), src].any()
    return SimpleNamespace(id=cid, lat=lat, plain_lat=plain_lat, n=n, blocked=_frozen(blocked), costly=_frozen(costly), src=_frozen(src),
                           poses=_frozen(poses_at(lat, src)), penalty=int(c.get("penalty", PENALTY)))


@functools.lru_cache(maxsize=None)
def field_want(cid, weighted):
    """uint32 [n, M] of the oracle, once per case.  dijkstra_w asserts that every route stays below 0xFFFFFFFE."""
    s = field_case(cid)
    if weighted:
        rows = [WO.dijkstra_w(s.blocked[e], s.costly[e], s.lat.dims, s.lat.cost, int(s.src[e]), s.penalty) for e in range(s.n)]
    else:
        rows = [FO.dijkstra(s.blocked[e], s.plain_lat.dims, s.plain_lat.cost, int(s.src[e])) for e in range(s.n)]
    return _frozen(np.stack(rows))


def cost_sum_at_the_bound(lat, penalty):
    """M * (max used cost + penalty) is the largest such product below 0xFFFFFFFE."""
    used = [b for b in range(1, 8) if not any((b >> a) & 1 and lat.dims[a] == 1 for a in range(3))]
    top = max(int(lat.cost[b]) for b in used) + int(penalty)
    return lat.num_nodes * top < K_FREE <= lat.num_nodes * (top + 1)


def largest_candidate(lat, field, blocked, penalty):
    """The largest cand = d[n] + cost + pen that k_flight_field can form on a settled table: over every free node's reached
    neighbours, with the penalty (an upper bound where the node is not costly)."""
    best = 0
    for c in np.nonzero(~blocked)[0].tolist():
        for nb, ci in FO.neighbours(c, lat.dims):
            if field[nb] != INF:
                best = max(best, int(field[nb]) + int(lat.cost[ci]) + int(penalty))
    return best


# ---------------------------------------------------------------------------
# mutants of the oracle: what a slip in the weighted kernel would compute
# ---------------------------------------------------------------------------
def clear_high_bits(costly):
    """A 32-bit `mine`: the bits of chunks 32 .. 39 (nodes >= 32768) are lost."""
    out = np.array(costly, bool)
    out[32 * K_FIELD_LANES:] = False
    return out


def swap_chunks(costly):
    """`mine >> q` where `mine >> chunk` is meant: the bit of (chunk q, lane t) is taken from chunk per_lane - 1 - q (0 where that
    node does not exist)."""
    costly = np.asarray(costly, bool)
    m = costly.shape[0]
    per_lane = _ceil(m, K_FIELD_LANES)
    c = np.arange(m)
    other = (per_lane - 1 - c // K_FIELD_LANES) * K_FIELD_LANES + c % K_FIELD_LANES
    return np.where(other < m, costly[np.minimum(other, m - 1)], False)


def dijkstra_leaving(blocked, costly, dims, cost, src, penalty):
    """tests/flight_w_oracle.py dijkstra_w with the penalty charged for the node LEFT (the source included, the target not)."""
    m = dims[0] * dims[1] * dims[2]
    free, pen = (~np.asarray(blocked, bool)).tolist(), [int(penalty) if c else 0 for c in np.asarray(costly, bool).tolist()]
    cost = [int(c) for c in cost]
    dist = [INF] * m
    dist[src] = 0
    heap = [(0, src)]
    while heap:
        d, c = heapq.heappop(heap)
        if d > dist[c]:
            continue
        for nb, ci in FO.neighbours(c, dims):
            if free[nb]:
                nd = d + cost[ci] + pen[c]
                if nd < dist[nb]:
                    dist[nb] = nd
                    heapq.heappush(heap, (nd, nb))
    return np.array(dist, np.uint64).astype(np.uint32)


def mutant_fields(cid, e):
    """{name: uint32 [M]} of env e: every mutant that is one for this lattice (a 32-bit register loses nothing below 32768 nodes;
    with one node per lane there is one chunk)."""
    s = field_case(cid)
    lat, src = s.lat, int(s.src[e])
    out = {"penalty-on-the-node-left": dijkstra_leaving(s.blocked[e], s.costly[e], lat.dims, lat.cost, src, s.penalty)}
    if lat.num_nodes > K_FIELD_LANES:
        out["chunk-mix-up"] = WO.dijkstra_w(s.blocked[e], swap_chunks(s.costly[e]), lat.dims, lat.cost, src, s.penalty)
    if lat.num_nodes > 32 * K_FIELD_LANES:
        out["32-bit-mine"] = WO.dijkstra_w(s.blocked[e], clear_high_bits(s.costly[e]), lat.dims, lat.cost, src, s.penalty)
    return out


# ---------------------------------------------------------------------------
# one wave on a line: the sweep cap
# ---------------------------------------------------------------------------
def line_sweeps(m, src, step, costly, penalty):
    """k_flight_field on (m, 1, 1) with m <= 64 and nothing blocked: every node sits in one wave and one chunk, and a lane's loads
    are issued before any lane's store, so a sweep reads the table the sweep before left (a Jacobi step).  -> (the sweeps run
    until one changes nothing, that one included; the table)."""
    assert m <= K_WAVE
    d = [K_FREE] * m
    d[src] = 0
    sweeps = 0
    while True:
        old, changed = list(d), False
        for c in range(m):
            if old[c] == 0:
                continue
            pen = int(penalty) if costly[c] else 0
            for nb in (c - 1, c + 1):
                if 0 <= nb < m and old[nb] < K_FREE and old[nb] + step + pen < d[c]:
                    assert old[nb] + step + pen < K_FREE
                    d[c], changed = old[nb] + step + pen, True
        sweeps += 1
        if not changed:
            return sweeps, np.array(d, np.uint64).astype(np.uint32)


# ---------------------------------------------------------------------------
# check_field_case: the case reaches the regime its id names
# ---------------------------------------------------------------------------
def check_field_case(cid):
    c = FIELD_CASES[cid]
    dims = c["dims"]
    modes = accepted_modes(dims)
    r = {mode: field_regime(dims, mode) for mode in modes}
    any_r = r[2]
    m, per_lane = any_r.m, any_r.per_lane
    assert all(1 <= d <= 1024 for d in dims) and m == int(np.prod(dims))
    assert 2 in modes and 0 in modes and r[2].lds is False and r[0].lds == (m <= lds_max_nodes())
    if 1 in modes:
        assert r[1].lds and vars(r[0]) == vars(r[1]) and r[1].lds_bytes <= K_LDS_BYTES and r[1].mine_bits <= 40
    if cid.startswith("pl1-full-deal"):
        assert per_lane == 1 and m == K_FIELD_LANES and not any_r.tail_word and any_r.last_chunk_nodes == K_FIELD_LANES
        assert any_r.unit_axes == (2,)
    if cid.startswith("pl2-one-node-chunk"):
        assert per_lane == 2 and any_r.last_chunk_nodes == 1 and any_r.tail_word
    if cid.startswith("nx1"):
        assert any_r.unit_axes == (0,) and any_r.tail_word and m == 1023
    if cid.startswith("ny1"):
        assert any_r.unit_axes == (1,) and any_r.tail_word and m == 1023
    if cid.startswith("line") or cid.startswith("bound-line"):
        assert any_r.unit_axes == (1, 2) and dims[0] == m
    if cid.endswith("-cap"):
        assert any_r.one_wave and per_lane == 1 and set(c["line"]) == {0, m - 1}
    if cid == "line-1024-mid":
        assert m == K_FIELD_LANES and c["line"] == (m // 2,)
    if cid.startswith("pl33-lds"):
        assert per_lane == 33 and 1 in modes and r[1].needs_attribute and m > 32 * K_FIELD_LANES
        assert _ceil(m - 36 * 36, K_FIELD_LANES) < 33  # the smallest 36 x 36 x nz that reaches bit 32
    if cid.startswith("pl40-capacity"):
        assert per_lane == 40 == _ceil(lds_max_nodes(), K_FIELD_LANES) and 1 in modes and m + 36 * 36 > lds_max_nodes() and c["n"] == 2
        assert r[1].needs_attribute
    if cid.startswith("above-capacity"):
        assert modes == (2, 0) and not r[0].lds and lds_max_nodes() < m <= lds_max_nodes() + 36 * 36 and c["n"] == 2
    if cid.startswith("bound"):
        s = field_case(cid)
        assert 1 in modes and cost_sum_at_the_bound(s.lat, s.penalty) and cost_sum_at_the_bound(s.plain_lat, 0)
        assert not cost_sum_at_the_bound(s.lat, s.penalty - 1)
    return dict(m=m, per_lane=per_lane, modes=modes, lds_bytes=r[0].lds_bytes, tail_word=any_r.tail_word, unit_axes=any_r.unit_axes,
                last_chunk_nodes=any_r.last_chunk_nodes)


# ---------------------------------------------------------------------------
# the seven distinct 9 x 7 x 5 envs of the query and path cases
# ---------------------------------------------------------------------------
D = 7
SEALED_SET, SEALED_NODE = 1, 157  # (4, 3, 2): an interior node behind a closed shell
QUERY_SHAPES = ((1, 1), (32, 8), (257, 1), (3, 171))
QUERY_STRIDES = (3, 6, 8)
PATH_NS = (64, 65, 130)
PATH_PENALTIES = (None, 777, 0)  # None: the plain entry points


@functools.lru_cache(maxsize=None)
def small_sets():
    """The recipe of tests/test_flight_gpu.py's small case with costly bits beside it: three random masks (10 / 30 / 50 % blocked; the
    second with a sealed free node), nothing blocked, everything blocked, a blocked source, a NaN source pose."""
    lat = lattice(SMALL_DIMS)
    m, rs = lat.num_nodes, np.random.RandomState(5)
    blocked = np.stack([rs.rand(m) < 0.1, rs.rand(m) < 0.3, rs.rand(m) < 0.5, np.zeros(m, bool), np.ones(m, bool), rs.rand(m) < 0.3,
                        rs.rand(m) < 0.3])
    costly = rs.rand(D, m) < 0.4
    src = np.array([17, 200, 314, 0, 100, 150, 42])
    for e in (0, 1, 2, 6):
        blocked[e, src[e]] = False
    blocked[5, src[5]] = True
    idx = node_index(lat)
    blocked[SEALED_SET, np.abs(idx - idx[SEALED_NODE]).max(1) == 1] = True
    blocked[SEALED_SET, SEALED_NODE] = False
    poses = poses_at(lat, src)
    poses[6, 1] = np.nan
    return SimpleNamespace(lat=lat, blocked=_frozen(blocked), costly=_frozen(costly), src=_frozen(src), poses=_frozen(poses))


@functools.lru_cache(maxsize=None)
def small_want(penalty):
    """uint32 [7, 315]; penalty None: the plain field."""
    s = small_sets()
    rows = []
    for e in range(D):
        src = -1 if e == 6 else int(s.src[e])
        rows.append(FO.dijkstra(s.blocked[e], s.lat.dims, s.lat.cost, src) if penalty is None else
                    WO.dijkstra_w(s.blocked[e], s.costly[e], s.lat.dims, s.lat.cost, src, penalty))
    return _frozen(np.stack(rows))


def cycle(n):
    """int [n]: env e holds distinct set e mod 7, so two neighbours never share a table and a row index off by one shows."""
    return np.arange(n) % D


@functools.lru_cache(maxsize=None)
def query_targets(n, k, dims=SMALL_DIMS, seed=2):
    """f32 [n * k, 3], and per item its kind: of every 32 consecutive items six lie outside the lattice (one per side), nine have a
    NaN, +inf or -inf in one coordinate, the rest are random inside and up to a fifth of the span outside."""
    lat = lattice(dims)
    rs = np.random.RandomState(seed + 1000 * n + k)
    span = lat.h * (np.array(lat.dims) - 1)
    t = lat.lo + span * rs.uniform(-0.2, 1.2, (n * k, 3))
    kind = np.arange(n * k) % 32
    for i in range(n * k):
        if kind[i] < 6:
            a, low = kind[i] // 2, kind[i] % 2 == 0
            t[i, a] = lat.lo[a] - 3.7 * lat.h[a] if low else lat.lo[a] + span[a] + 2.2 * lat.h[a]
        elif kind[i] < 15:
            t[i, (kind[i] - 6) // 3] = (np.nan, np.inf, -np.inf)[(kind[i] - 6) % 3]
    return _frozen(t.astype(f32), kind)


def query_want(field, lat, targets, k):
    """field uint32 [n, M], targets [n * k, >= 3] -> uint32 [n * k]."""
    node = nearest(lat, targets)
    e = np.arange(len(node)) // k
    return np.where(node >= 0, field[e, np.maximum(node, 0)], INF).astype(np.uint32)


DYADIC = dict(unit=(0.5, 0.5, 0.5), lo=(0.0, 0.0, 0.0))  # every node and every half-way point is a dyadic rational: exact in fp32


def tie_targets(dims=SMALL_DIMS):
    """f32 [T, 3] on the dyadic lattice and the node that must win each: for every axis and every pair of neighbouring nodes on it the
    point exactly half-way, the other two coordinates on a node; then a point half-way on all three axes at once."""
    lat = lattice(dims, **DYADIC)
    rows, want = [], []
    base = [2, 3, 1]
    for a in range(3):
        for i in range(dims[a] - 1):
            idx = list(base)
            p = [0.5 * v for v in idx]
            p[a] = 0.5 * i + 0.25
            idx[a] = i + 1  # floor(x + 0.5): the higher node
            rows.append(p)
            want.append((idx[2] * dims[1] + idx[1]) * dims[0] + idx[0])
    rows.append([0.25, 0.25, 0.25])
    want.append((1 * dims[1] + 1) * dims[0] + 1)
    t = np.array(rows, f32)
    assert np.array_equal(t.astype(f64), np.array(rows, f64))
    return lat, t, np.array(want)


@functools.lru_cache(maxsize=None)
def path_case(n, penalty):
    """The walk's inputs and expected rows for n envs cycling through the seven sets: targets f32 [n, 6] (even envs: the set's
    farthest reached node; odd envs in turn a blocked node, a free node no route reaches, a NaN coordinate), the oracle's walks."""
    s = small_sets()
    lat = s.lat
    field = small_want(penalty)
    sets = cycle(n)
    tnode, kinds = np.zeros(n, np.int64), []
    for e in range(n):
        d = sets[e]
        reached = field[d] != INF
        if e % 2 == 0:
            tnode[e], kind = int(np.argmax(np.where(reached, field[d], 0))), "farthest"
        else:
            kind = ("blocked", "cut-off", "nan")[(e // 2) % 3]
            pool = np.nonzero(s.blocked[d])[0] if kind == "blocked" else np.nonzero(~s.blocked[d] & ~reached)[0]
            if kind == "nan" or len(pool) == 0:
                tnode[e], kind = e % lat.num_nodes, "nan"
            else:
                tnode[e] = int(pool[e % len(pool)])
        kinds.append(kind)
    targets = poses_at(lat, tnode)
    walks = []
    for e in range(n):
        d = sets[e]
        if kinds[e] == "nan":
            targets[e, e % 3] = np.nan
            walks.append([])
        elif penalty is None:
            walks.append(FO.walk(field[d], lat.dims, lat.cost, int(tnode[e])))
        else:
            walks.append(WO.walk_w(field[d], s.costly[d], lat.dims, lat.cost, penalty, int(tnode[e])))
    return SimpleNamespace(n=n, sets=sets, targets=_frozen(targets), tnode=_frozen(tnode), kinds=tuple(kinds), walks=walks,
                           longest=max(len(w) for w in walks))


def path_rows(case, max_len):
    """The expected nodes_out [n, max_len] over the poison and len_out [n]."""
    nodes = np.full((case.n, max_len), POISON, np.int32)
    count = np.zeros(case.n, np.int32)
    for e, w in enumerate(case.walks):
        nodes[e, :min(len(w), max_len)] = w[:max_len]
        count[e] = len(w) if len(w) <= max_len else -len(w)
    return nodes, count


# ---------------------------------------------------------------------------
# raw ctypes callers (GPU): poisoned outputs, GUARD words after each
# ---------------------------------------------------------------------------
def load_lib():
    from gennbv_amd import _lib
    return _lib.load()


def _torch():
    import torch
    return torch


def to_dev(a):
    """numpy (uint32 as its int32 bits) -> a contiguous device tensor."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return _torch().tensor(a).to(DEV)


def _out(words, fill):
    return _torch().full((words + GUARD,), fill, dtype=_torch().int32, device=DEV)


def _split(t, words, fill):
    a = t.cpu().numpy()
    return a[:words], bool((a[words:].view(np.uint32) == np.uint32(fill & 0xFFFFFFFF)).all())


def _lat_ptrs(lat):
    return (C.c_uint32 * 8)(*[int(c) for c in lat.cost]), (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)


def call_field(lat, blocked_t, poses_t, mode, costly_t=None, penalty=0, n=None, lib=None):
    """gnbv_flight_field (costly_t None) or gnbv_flight_field_w -> (return code, field uint32 [n, M], status int32 [n], both guards
    untouched).  poses_t [n, >= 3] may be strided."""
    lib = lib or load_lib()
    n = blocked_t.shape[0] if n is None else n
    m = lat.num_nodes
    cost, lo, h = _lat_ptrs(lat)
    field, status = _out(n * m, POISON), _out(n, STATUS_POISON)
    tail = (n, *lat.dims, cost, poses_t.data_ptr(), int(poses_t.stride(0)), lo, h, field.data_ptr(), status.data_ptr(), mode, None)
    if costly_t is None:
        err = lib.gnbv_flight_field(blocked_t.data_ptr(), *tail)
    else:
        err = lib.gnbv_flight_field_w(blocked_t.data_ptr(), costly_t.data_ptr(), int(penalty), *tail)
    _torch().cuda.synchronize()
    got, ok_f = _split(field, n * m, POISON)
    st, ok_s = _split(status, n, STATUS_POISON)
    return err, got.view(np.uint32).reshape(n, m), st, ok_f and ok_s


def call_query(lat, field_t, targets_t, n, k, row_stride):
    """gnbv_flight_query -> (return code, uint32 [n * k], the guard untouched).  targets_t holds n * k rows of row_stride floats."""
    _, lo, h = _lat_ptrs(lat)
    out = _out(n * k, POISON)
    err = load_lib().gnbv_flight_query(field_t.data_ptr(), n, *lat.dims, lo, h, targets_t.data_ptr(), k, row_stride, out.data_ptr(), None)
    _torch().cuda.synchronize()
    got, ok = _split(out, n * k, POISON)
    return err, got.view(np.uint32), ok


def call_path(lat, field_t, targets_t, max_len, costly_t=None, penalty=0):
    """gnbv_flight_path (costly_t None) or gnbv_flight_path_w -> (return code, nodes int32 [n, max_len], len int32 [n], both guards
    untouched): whatever the kernel did not write still holds the poison."""
    n = targets_t.shape[0]
    cost, lo, h = _lat_ptrs(lat)
    nodes, count = _out(n * max_len, POISON), _out(n, POISON)
    tail = (n, *lat.dims, cost, lo, h, targets_t.data_ptr(), int(targets_t.stride(0)), nodes.data_ptr(), max_len, count.data_ptr(), None)
    if costly_t is None:
        err = load_lib().gnbv_flight_path(field_t.data_ptr(), *tail)
    else:
        err = load_lib().gnbv_flight_path_w(field_t.data_ptr(), costly_t.data_ptr(), int(penalty), *tail)
    _torch().cuda.synchronize()
    got, ok_n = _split(nodes, n * max_len, POISON)
    cnt, ok_c = _split(count, n, POISON)
    return err, got.reshape(n, max_len), cnt, ok_n and ok_c

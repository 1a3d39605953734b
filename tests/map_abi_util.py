"""Shared by tests/test_map_abi_regimes_cpu.py and tests/test_map_abi_gpu.py: the four belief-map entry points at the C ABI --
gnbv_flight_blocked_tri, gnbv_flight_classify_tri (csrc/flightmap.hip), gnbv_sweep_tri (csrc/sweepmap.hip) and
gnbv_frontier_viewpoints (csrc/frontview.hip) -- past one workgroup's one turn and at every swizzle shift.  TEST INFRASTRUCTURE.

  * the host launch shape of the four entry points restated from make_map_args, gnbv_sweep_tri and gnbv_frontier_viewpoints, and
    the LDS pack of csrc/map_bits.h (map_lds_bytes, the three LDS limits, map_swizzle_shift, map_swizzle);
  * a restatement of the node kernels' store loop (which wave stores which word) and of the pack / read word maps, so that the CPU
    file can show that every word is written once and what a wrong chunk term or a wrong pack shift would leave behind;
  * the case tables, ids naming the regime, and check_*(): from the restated formulas and the oracles alone, a case reaches what
    its id names;
  * D = 6 distinct (grid, voxel frame, legs or targets, field) sets and a seeded assignment of n envs to them: the oracle runs once
    per distinct set and is gathered to n rows.  Oracle results are cached and returned read-only.

The oracles are the existing ones, unchanged: tests/flightmap_oracle.py, the composition of tests/test_flight_cautious_gpu.py,
tests/sweepmap_oracle.py, tests/frontview_oracle.py.  Every comparison built on them is exact.  Nothing here touches the GPU.
"""
import functools
from types import SimpleNamespace

import numpy as np

from tests import flightmap_oracle as MO
from tests import frontview_cases as FC
from tests import frontview_oracle as VO
from tests import sweepmap_oracle as SO

f32, f64 = np.float32, np.float64

# ---------------------------------------------------------------------------
# csrc/map_bits.h and the three hosts: constants, LDS sizes, swizzle, launch shape
# ---------------------------------------------------------------------------
K_WAVE = 64               # kWave
K_LANES = 512             # kMapLanes, kSweepLanes, kViewLanes
K_WAVES = K_LANES // K_WAVE
K_LDS_BYTES = 160 * 1024  # kMapLdsBytes
K_MAX_GRID = 128          # kMapMaxGrid
K_VIEW_SCRATCH = K_WAVES * 16  # kViewScratchBytes, in front of the viewpoint kernel's planes
K_WG_TARGET = 512         # the LDS modes aim at about this many workgroups over all envs


def _ceil(a, b):
    return -(-a // b)


def map_lds_bytes(g):
    words = 2 * _ceil(g ** 3, 64)
    return 4 * (_ceil(words, 32) * 32)


def _max_grid(planes, extra=0):
    g = 1
    while g < K_MAX_GRID and planes * map_lds_bytes(g + 1) + extra <= K_LDS_BYTES:
        g += 1
    return g


def map_lds_max_grid():
    return _max_grid(1)


def map_planes_max_grid():
    return _max_grid(2)


def view_lds_max_grid():
    return _max_grid(2, K_VIEW_SCRATCH)


def map_swizzle_shift(g):
    shift = 5
    while shift < 20 and (2 << shift) * 3 <= (g * g // 32) * 4:
        shift += 1
    return shift


def map_swizzle(w, shift):
    return w ^ ((w >> shift) & 31)


def grid_words(g):
    """Word indices below this hold a voxel (or the rest of the last ballot): two words per 64-voxel ballot."""
    return 2 * _ceil(g ** 3, 64)


def chunk_cap(n):
    """The most workgroups an env gets in the LDS modes."""
    return max(1, _ceil(K_WG_TARGET, n))


def _uses_lds(mode, g, limit):
    assert mode in (0, 1, 2) and (mode != 1 or g <= limit), "the host refuses this"
    return mode == 1 or (mode == 0 and g <= limit)


def node_shape(n, m, mode, g, planes=1):
    """make_map_args: gnbv_flight_blocked_tri (planes 1) and gnbv_flight_classify_tri (planes 2) on a lattice of m nodes."""
    lds = _uses_lds(mode, g, map_lds_max_grid() if planes == 1 else map_planes_max_grid())
    groups = _ceil(m, K_WAVE)
    uncapped = _ceil(groups, K_WAVES)
    cap = chunk_cap(n)
    chunks = min(uncapped, cap) if lds else uncapped
    chunk_waves = _ceil(groups, chunks)
    chunks = _ceil(groups, chunk_waves)
    return SimpleNamespace(lds=lds, groups=groups, uncapped=uncapped, cap=cap, cap_binds=lds and cap < uncapped, chunks=chunks,
                           chunk_waves=chunk_waves, turns=_ceil(chunk_waves, K_WAVES), m=m, words=_ceil(m, 32),
                           shift=map_swizzle_shift(g), lds_bytes=planes * map_lds_bytes(g) if lds else 0, tail=m % K_WAVE,
                           dead_groups=chunks * chunk_waves - groups)


def sweep_shape(n, k, mode, g):
    """gnbv_sweep_tri: K items per env, a wave owns an item at a time."""
    lds = _uses_lds(mode, g, map_lds_max_grid())
    uncapped = _ceil(k, K_WAVES)
    cap = chunk_cap(n)
    chunks = min(uncapped, cap) if lds else uncapped
    chunk_items = _ceil(k, chunks)
    chunks = _ceil(k, chunk_items)
    return SimpleNamespace(lds=lds, uncapped=uncapped, cap=cap, cap_binds=lds and cap < uncapped, chunks=chunks, chunk_items=chunk_items,
                           turns=_ceil(chunk_items, K_WAVES), last_items=k - (chunks - 1) * chunk_items, shift=map_swizzle_shift(g),
                           lds_bytes=map_lds_bytes(g) if lds else 0)


def view_shape(n, t, mode, g, chunk=0, window=1):
    """gnbv_frontier_viewpoints: T targets per env; mode 0 is the grid in place; `window` the most nodes any target's index window
    holds (view_window), of which a lane takes ceil(window / 512) turns."""
    assert mode in (0, 1, 2) and (mode != 1 or g <= view_lds_max_grid()), "the host refuses this"
    lds = mode == 1
    if chunk == 0:
        want = chunk_cap(n) if lds else t
        chunk = _ceil(t, want)
    chunk = min(max(chunk, 1), t)
    chunks = _ceil(t, chunk)
    return SimpleNamespace(lds=lds, cap=chunk_cap(n), chunks=chunks, chunk_items=chunk, last_items=t - (chunks - 1) * chunk,
                           turns=_ceil(window, K_LANES), shift=map_swizzle_shift(g), plane_words=map_lds_bytes(g) // 4 if lds else 0,
                           lds_bytes=K_VIEW_SCRATCH + (2 * map_lds_bytes(g) if lds else 0))


def store_words(shape, blocked, poison, drop_chunk_term=False):
    """The store loop of k_flight_blocked_tri for one env, restated: blocked bool [m] -> (words uint32 [words] over `poison`, how
    often each word was written).  drop_chunk_term: c0 = t * 64 in every chunk -- what the kernel would do without it."""
    out = np.full(shape.words, poison, np.uint32)
    writes = np.zeros(shape.words, np.int64)
    padded = np.ones((shape.chunks * shape.chunk_waves + K_WAVES) * K_WAVE, bool)
    padded[:shape.m] = blocked
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    for chunk in range(shape.chunks):
        for wave in range(K_WAVES):
            for t in range(wave, shape.chunk_waves, K_WAVES):
                c0 = ((0 if drop_chunk_term else chunk * shape.chunk_waves) + t) * K_WAVE
                for half in range(2):
                    w = (c0 >> 5) + half
                    if w < shape.words:
                        out[w] = np.uint32((padded[c0 + 32 * half:c0 + 32 * half + 32].astype(np.uint64) * weights).sum())
                        writes[w] += 1
    return out, writes


def misplaced_words(g, pack_shift, read_shift):
    """The words of a G^3 grid that a pack with one shift and a reader with another disagree about."""
    return [w for w in range(grid_words(g)) if map_swizzle(w, pack_shift) != map_swizzle(w, read_shift)]


# ---------------------------------------------------------------------------
# the six distinct sets of the node and sweep kernels, and the assignment of n envs to them
# ---------------------------------------------------------------------------
D = 6
RHO = 0.23
BIG_LO, BIG_HI = np.array([-1.4, 1.6, -0.3]), np.array([1.0, 4.2, 1.5])  # tests/sweepmap_cases.py's frames
SMALL_LO, SMALL_HI = np.array([-0.5, 2.5, 0.3]), np.array([0.1, 3.0, 0.7])
RANDOM, FREE, UNKNOWN, OCCUPIED, SMALL, SPARSE = range(D)
FLAGS8 = tuple((u, o, gr) for u in (0, 1) for o in (0, 1) for gr in (0, 1))
FLAGS2 = ((0, 0, 0), (1, 1, 1))


def frames(g):
    """range_gt [6,6] (max, min per axis: voxel centres) and voxel_size [6,3], anisotropic: sets 0-3 and 5 hold the lattice and its
    balls, set 4's grid is far smaller than the lattice."""
    rng, vox = np.zeros((D, 6), f32), np.zeros((D, 3), f32)
    for e in range(D):
        lo, hi = (SMALL_LO, SMALL_HI) if e == SMALL else (BIG_LO - 0.01 * e, BIG_HI + 0.013 * e)
        v = (hi - lo) / g
        vox[e] = v
        rng[e, 1::2] = lo + 0.5 * v
        rng[e, 0::2] = hi - 0.5 * v
    return rng, vox


def ball_voxels(vox, rho=RHO):
    """About how many voxels a ball of radius rho touches: its box of voxels times the share a ball takes of its box."""
    return 0.55 * float(np.prod(2.0 * rho / np.asarray(vox, f64) + 1.0))


@functools.lru_cache(maxsize=None)
def map_sets(g):
    """(tri int8 [6,G,G,G], range_gt, voxel_size): random thirds of -1 / 0 / 1, all free, all unknown, all occupied, the small grid
    (random thirds), a sparse grid; 30 % of the non-zero voxels at the int8 extremes -128 / 127.  The densities are those of
    tests/test_flightmap_gpu.py at G = 12 and fall with the voxels a ball holds above it: the sparse grid keeps an expected half
    occupied (0.3 unknown) voxel per ball, so that every answer occurs at every G; the random grids keep at most 700 voxels of a
    class.  G = 1 and 2 are set by hand: one voxel has one class."""
    rs = np.random.RandomState(300 + g)
    rng, vox = frames(g)
    dense = min(1.0 / 3.0, 700.0 / g ** 3)
    u = rs.rand(D, g, g, g)
    tri = np.where(u < dense, 1, np.where(u < 2.0 * dense, 0, -1)).astype(np.int8)
    tri[FREE], tri[UNKNOWN], tri[OCCUPIED] = -1, 0, 1
    p = min(0.025, 0.5 / ball_voxels(vox[SPARSE]))
    u = rs.rand(g, g, g)
    tri[SPARSE] = np.where(u < p, 1, np.where(u < 1.6 * p, 0, -1))
    if g == 1:
        tri[RANDOM], tri[SMALL], tri[SPARSE] = 0, 1, -1
    if g == 2:  # the small grid: one occupied corner voxel in unknown space
        tri[SMALL] = 0
        tri[SMALL, 0, 0, 0] = 1
    ext = rs.rand(D, g, g, g) < 0.3
    tri = np.where(ext & (tri < 0), -128, np.where(ext & (tri > 0), 127, tri)).astype(np.int8)
    assert g < 8 or ((tri == -128).any() and (tri == 127).any() and (tri == 0).any())
    for a in (tri, rng, vox):
        a.setflags(write=False)
    return tri, rng, vox


@functools.lru_cache(maxsize=None)
def assign(n, d=D, seed=0):
    """int [n]: which distinct set env e holds.  n == d: the identity.  Else seeded, every set occurs and no two consecutive envs
    hold the same set, so an env index off by one shows."""
    if n == d:
        a = np.arange(d)
    else:
        assert n > 2 * d
        rs = np.random.RandomState(1000 * n + seed)
        a = np.empty(n, np.int64)
        a[:d] = rs.permutation(d)
        for e in range(d, n):
            a[e] = (a[e - 1] + 1 + rs.randint(d - 1)) % d
    assert set(a.tolist()) == set(range(d)) and (n == 1 or (a[1:] != a[:-1]).all())
    a.setflags(write=False)
    return a


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------
# node kernels: lattices, oracle words, cases
# ---------------------------------------------------------------------------
LAT_LO, LAT_SPAN = np.array([-1.0, 2.0, 0.1]), np.array([1.6, 1.8, 1.0])  # tests/test_flightmap_gpu.py's lattice, resampled


def lattice(dims):
    """What the C ABI needs of a lattice (and what the `_launch` helpers of the existing GPU tests read): dims, lo, h (0 on a
    single-node axis), num_nodes, words."""
    dims = tuple(int(d) for d in dims)
    h = np.array([LAT_SPAN[a] / (dims[a] - 1) if dims[a] > 1 else 0.0 for a in range(3)])
    m = dims[0] * dims[1] * dims[2]
    return SimpleNamespace(dims=dims, lo=LAT_LO.copy(), h=h, num_nodes=m, words=_ceil(m, 32))


@functools.lru_cache(maxsize=None)
def node_want(g, dims, sets, flags):
    """uint32 [len(sets), words]: the oracle's blocked words of the distinct sets `sets` (a tuple), once per (grid, lattice, flags)."""
    tri, rng, vox = map_sets(g)
    lat = lattice(dims)
    s = list(sets)
    return _frozen(MO.blocked_words(tri[s], rng[s], vox[s], lat.dims, lat.lo, lat.h, RHO, *[bool(f) for f in flags]))


def classify_want(g, dims, sets, outside, ground):
    """(blocked, costly) words: the oracle called with unknown_blocks 0 and 1 and composed as tests/test_flight_cautious_gpu.py does."""
    from tests.test_flight_cautious_gpu import _compose
    return _compose(node_want(g, dims, sets, (0, outside, ground)), node_want(g, dims, sets, (1, outside, ground)))


def bits_of(words, m):
    """uint32 [..., words] -> bool [..., m]."""
    c = np.arange(m)
    return ((words[..., c >> 5] >> (c & 31).astype(np.uint32)) & 1).astype(bool)


SWIZZLE_GS = (1, 2, 33, 45, 64, 85)  # shifts 5, 5, 5, 6, 7, 8; 85 fits two planes; G^3 mod 64 != 0 but at 64
SWIZZLE_SETS = (SPARSE, SMALL, RANDOM)
ALL_SETS = tuple(range(D))

# id -> dims, n, the mode under test (mode 0 runs too where it resolves to it), grids, flag sets, the distinct sets
NODE_CASES = {}
for _name, _dims in (("567-ragged-last-chunk", (9, 9, 7)), ("1024-whole-chunks", (8, 8, 16)), ("595-tail-1-to-32", (17, 5, 7)),
                     ("693-tail-33-to-63", (11, 9, 7)), ("609-single-node-axis", (29, 21, 1))):
    NODE_CASES["m2-" + _name] = dict(dims=_dims, n=6, mode=2, gs=(12, 13), flags=FLAGS8, sets=ALL_SETS)
    NODE_CASES["m1-cap-free-" + _name] = dict(dims=_dims, n=6, mode=1, gs=(12, 13), flags=FLAGS8, sets=ALL_SETS)
NODE_CASES["m1-n171-2431-cap-binds-two-turns"] = dict(dims=(17, 13, 11), n=171, mode=1, gs=(12,), flags=FLAGS2, sets=ALL_SETS)
NODE_CASES["m2-n171-2431-five-chunks"] = dict(dims=(17, 13, 11), n=171, mode=2, gs=(12,), flags=FLAGS2, sets=ALL_SETS)
NODE_CASES["m1-n512-567-one-chunk-two-turns"] = dict(dims=(9, 9, 7), n=512, mode=1, gs=(12,), flags=FLAGS2, sets=ALL_SETS)
for _g in SWIZZLE_GS:
    for _mode in (1, 2):
        NODE_CASES[f"m{_mode}-swizzle-g{_g}"] = dict(dims=(9, 9, 7), n=3, mode=_mode, gs=(_g,), flags=FLAGS2, sets=SWIZZLE_SETS)


def case_rows(case):
    """int [n]: for every env of a case, the row of its distinct set in the case's `sets` (and in the oracle results over them)."""
    d = len(case["sets"])
    return np.arange(d) if case["n"] == d else assign(case["n"], d)


def node_case_sets(case):
    """int [n]: the distinct set of every env of a case."""
    return np.array(case["sets"])[case_rows(case)]


def check_node_case(cid):
    """From the restated formulas alone: the case reaches the regime its id names, for both kernels (the classify kernel has the
    same launch shape; only its LDS limit differs)."""
    c = NODE_CASES[cid]
    m = int(np.prod(c["dims"]))
    info = {}
    for g in c["gs"]:
        for planes in (1, 2):
            s = node_shape(c["n"], m, c["mode"], g, planes)
            assert s.lds == (c["mode"] == 1) and s.lds_bytes <= K_LDS_BYTES
            if c["mode"] == 1:
                assert vars(node_shape(c["n"], m, 0, g, planes)) == vars(s)  # mode 0 resolves to it
            last_c0 = (s.chunks * s.chunk_waves - 1) * K_WAVE  # the first node of the last group the launch holds
            if "ragged-last-chunk" in cid:
                assert s.chunks == 2 and s.dead_groups >= 1 and last_c0 >= m and (last_c0 >> 5) >= s.words
            if "whole-chunks" in cid:
                assert s.chunks >= 2 and s.tail == 0 and s.dead_groups == 0 and s.chunk_waves == K_WAVES
            if "tail-1-to-32" in cid:
                assert s.chunks >= 2 and 1 <= s.tail <= 32 and s.words % 2 == 1  # the last ballot's high word does not exist
            if "tail-33-to-63" in cid:
                assert s.chunks >= 2 and 33 <= s.tail <= 63 and s.words % 2 == 0
            if "single-node-axis" in cid:
                assert 1 in c["dims"] and m > K_LANES and s.chunks >= 2
            if "cap-free" in cid:
                assert not s.cap_binds and s.chunks == s.uncapped >= 2 and s.turns == 1
            if "cap-binds" in cid:
                assert s.cap_binds and 1 < s.cap < s.uncapped and s.chunks == s.cap and s.turns == 2
            if "five-chunks" in cid:
                assert s.chunks == 5 and c["n"] * s.chunks > 512
            if "one-chunk" in cid:
                assert s.cap == 1 and s.chunks == 1 and s.chunk_waves > K_WAVES and s.turns == 2
            if "swizzle" in cid:
                assert s.chunks == 2 and g <= map_planes_max_grid()
            info[(g, planes)] = dict(chunks=s.chunks, chunk_waves=s.chunk_waves, turns=s.turns, tail=s.tail, cap=s.cap if s.lds else None,
                                     shift=s.shift, lds_bytes=s.lds_bytes)
    if c["n"] > len(c["sets"]):
        assert set(node_case_sets(c).tolist()) == set(c["sets"])
    return info


# ---------------------------------------------------------------------------
# gnbv_sweep_tri: legs, oracle codes, cases
# ---------------------------------------------------------------------------
K_POOL = 57
RADII = (0.23, 0.06)  # tests/sweepmap_cases.py's
SWIZZLE_RADIUS = 0.12
SWEEP_G = 12


@functools.lru_cache(maxsize=None)
def leg_pool(g):
    """(from f32 [6,57,6], to f32 [6,57,6], start f32 [6,6]): tests/sweepmap_cases.py legs()'s recipe, continued past 40 rows (row j
    is of the kind of row j mod 40).  Pose rows whose first three floats are the point; `start` is the broadcast form's one start
    per set."""
    rs = np.random.RandomState(400 + g)
    k = K_POOL
    frm, to = np.full((D, k, 6), 7.0, f32), np.full((D, k, 6), -7.0, f32)
    size = BIG_HI - BIG_LO
    for e in range(D):
        a, b = BIG_LO + size * rs.rand(k, 3), BIG_LO + size * rs.rand(k, 3)
        for j in range(k):
            kind, ax = j % 40, j % 3
            if 16 <= kind < 22:  # across: from beyond one face to beyond the opposite one
                a[j, ax], b[j, ax] = BIG_LO[ax] - 0.2 - 0.5 * rs.rand(), BIG_HI[ax] + 0.2 + 0.5 * rs.rand()
            elif 22 <= kind < 28:  # one end outside
                end = b if j % 2 else a
                end[j, ax] = (BIG_HI[ax] + 0.1 + rs.rand()) if kind < 25 else (BIG_LO[ax] - 0.1 - rs.rand())
            elif 28 <= kind < 31:  # wholly outside, one of them passing close by a face
                a[j, ax] = b[j, ax] = BIG_HI[ax] + (0.15 if kind == 28 else 0.9) + 0.1 * rs.rand()
            elif 31 <= kind < 37:  # axis-parallel: the two other coordinates equal
                keep = a[j, ax]
                a[j] = b[j]
                a[j, ax] = keep
            elif kind == 37:  # zero length, inside
                b[j] = a[j]
            elif kind == 38:  # zero length, just outside two faces
                a[j] = b[j] = BIG_HI + np.array([0.05, -0.4, 0.05])
            elif kind == 39:
                b[j, 1] = np.nan
        frm[e, :, :3], to[e, :, :3] = a, b
    start = np.ascontiguousarray(frm[:, 3])
    return _frozen(frm, to, start)


def pick(k):
    """The rows of the pool a case of K items takes: all kinds of leg at every K."""
    return np.arange(k) if k >= 40 else (np.arange(k) * 40) // k


@functools.lru_cache(maxsize=None)
def sweep_dist(g, sets, broadcast):
    """The oracle's least distances of the whole pool to the grids of the distinct sets `sets`, once per (grid, sets, from-form)."""
    tri, rng, vox = map_sets(g)
    frm, to, start = leg_pool(g)
    s = list(sets)
    return SO.min_dist(tri[s], rng[s], vox[s], (start if broadcast else frm)[s], to[s])


@functools.lru_cache(maxsize=None)
def sweep_want(g, k, sets, broadcast, radius, flags):
    """(code uint8 [len(sets), K], robust bool [len(sets), K]) of the oracle for the distinct sets `sets` (a tuple)."""
    _, rng, vox = map_sets(g)
    frm, to, start = leg_pool(g)
    s, rows = list(sets), pick(k)
    dist = {unk: d[:, rows] for unk, d in sweep_dist(g, sets, broadcast).items()}
    f = start[s] if broadcast else frm[s][:, rows]
    return _frozen(*SO.codes_from(dist, g, rng[s], vox[s], f, to[s][:, rows], radius, *[bool(x) for x in flags]))


SWEEP_SWIZZLE_SETS = (SPARSE, SMALL)
SWEEP_CASES = {
    "k5-fewer-items-than-waves": dict(n=6, k=5, gs=(SWEEP_G,), modes=(1, 2, 0), radii=RADII, flags=FLAGS8, sets=ALL_SETS),
    "k8-one-item-per-wave": dict(n=6, k=8, gs=(SWEEP_G,), modes=(1, 2, 0), radii=RADII, flags=FLAGS8, sets=ALL_SETS),
    "k41-a-wave-leaves-beside-working-waves": dict(n=6, k=41, gs=(SWEEP_G,), modes=(1, 2, 0), radii=RADII, flags=FLAGS8, sets=ALL_SETS),
    "k57-last-chunk-of-one-item": dict(n=6, k=57, gs=(SWEEP_G,), modes=(1, 2, 0), radii=RADII, flags=FLAGS8, sets=ALL_SETS),
    "n171-k40-cap-binds-two-turns": dict(n=171, k=40, gs=(SWEEP_G,), modes=(1, 2, 0), radii=RADII[:1], flags=FLAGS2, sets=ALL_SETS),
    "n512-k19-one-chunk-three-turns": dict(n=512, k=19, gs=(SWEEP_G,), modes=(1, 2, 0), radii=RADII[:1], flags=FLAGS2, sets=ALL_SETS),
}
for _g in SWIZZLE_GS + (109, 128):
    SWEEP_CASES[f"swizzle-g{_g}"] = dict(n=2, k=24, gs=(_g,), modes=(2, 0) if _g > 109 else (1, 2, 0), radii=(SWIZZLE_RADIUS,),
                                         flags=((1, 0, 0), (0, 1, 1)), sets=SWEEP_SWIZZLE_SETS)


def check_sweep_case(cid):
    c = SWEEP_CASES[cid]
    n, k = c["n"], c["k"]
    info = {}
    for g in c["gs"]:
        for mode in c["modes"]:
            s = sweep_shape(n, k, mode, g)
            info[(g, mode)] = dict(chunks=s.chunks, chunk_items=s.chunk_items, turns=s.turns, last_items=s.last_items,
                                   cap=s.cap if s.lds else None, shift=s.shift, lds_bytes=s.lds_bytes)
            assert s.lds_bytes <= K_LDS_BYTES and s.lds == (mode == 1 or (mode == 0 and g <= map_lds_max_grid()))
            if "fewer-items-than-waves" in cid:
                assert k < K_WAVES and s.chunks == 1 and s.chunk_items == k
            if "one-item-per-wave" in cid:
                assert k == K_WAVES and s.chunks == 1 and s.chunk_items == K_WAVES
            if "a-wave-leaves-beside-working-waves" in cid:
                # in the last chunk a wave below chunk_items finds j >= K and leaves while other waves of the workgroup work on
                assert s.chunks >= 2 and 1 <= s.last_items < s.chunk_items <= K_WAVES
            if "last-chunk-of-one-item" in cid:
                assert s.chunks >= 2 and s.last_items == 1 and s.chunk_items == K_WAVES  # seven waves leave at once
                smaller = [sweep_shape(n, kk, mode, g) for kk in range(1, k)]
                assert not any(x.chunks >= 2 and x.last_items == 1 and x.chunk_items == K_WAVES for x in smaller)  # the least such K
            if "cap-binds-two-turns" in cid and s.lds:
                assert s.cap_binds and s.cap == 3 and s.chunk_items == 14 and s.turns == 2 and s.last_items == 12
            if "one-chunk-three-turns" in cid and s.lds:
                assert s.cap == 1 and s.chunks == 1 and s.turns == 3 and k % K_WAVES != 0  # a ragged last turn
            if ("cap-binds" in cid or "one-chunk" in cid) and not s.lds:
                assert s.chunks == s.uncapped and n * s.chunks > 512
    return info


# ---------------------------------------------------------------------------
# gnbv_frontier_viewpoints: the large lattice, fields that place the winner, cases
# ---------------------------------------------------------------------------
VIEW_DIMS = (13, 11, 9)   # 1287 nodes over the extent of tests/frontview_cases.py lattice(): three turns of 512 lanes
VIEW_G, VIEW_T = 12, 20
VIEW_R_MAX, VIEW_MAX_UNKNOWN = 10.0, 3
V_RANDOM, V_SPARSE, V_FREE, V_OCCUPIED, V_OPEN, V_UNKNOWN = range(D)  # the five of frontview_cases.py and an all-unknown grid
NO_ROUTE = FC.NO_ROUTE
LOW, MID, HIGH = 500, 1500, 2500  # a field of three costs


def view_lattice(dims):
    dims = tuple(int(d) for d in dims)
    lo = -0.5 * FC.EXTENT - 0.4
    h = np.array([(FC.EXTENT[a] + 0.8) / (dims[a] - 1) for a in range(3)])
    return dims, lo, h


def axis_window(q, r, lo, h, n):
    """csrc/frontview.hip axis_window in fp64: the nodes [i0, i1] of one axis the kernel visits for a target at q."""
    if n == 1:
        return 0, 0
    q, r, lo, h, top = f64(q), f64(r), f64(lo), f64(h), f64(n - 1)
    slack = f64(1.0) + ((abs(q) + r) + abs(lo)) / h * f64(2.0 ** -48)
    a, b = np.floor(((q - r) - lo) / h - slack), np.ceil(((q + r) - lo) / h + slack)
    return int(min(max(a, 0.0), top)), int(min(max(b, 0.0), top))


def view_window(range_gt, voxel_size, target, r_max, dims, lo, h):
    """(i0, i1, j0, j1, k0, k1) of one in-grid target of one env."""
    o, v = VO.voxel_frame(range_gt, voxel_size)
    q = o + (np.asarray(target, f64) + 0.5) * v
    return sum((axis_window(q[a], r_max, lo[a], h[a], dims[a]) for a in range(3)), ())


def slot_of(node, window, dims):
    """Where the kernel meets node c of a window: its slot s (i fastest), and from it the turn, the wave and the lane that hold it."""
    i0, i1, j0, j1, k0, k1 = window
    i, j, k = node % dims[0], (node // dims[0]) % dims[1], node // (dims[0] * dims[1])
    assert i0 <= i <= i1 and j0 <= j <= j1 and k0 <= k <= k1
    s = ((k - k0) * (j1 - j0 + 1) + (j - j0)) * (i1 - i0 + 1) + (i - i0)
    return SimpleNamespace(slot=s, turn=s // K_LANES, wave=(s % K_LANES) // K_WAVE, lane=s % K_WAVE, tid=s % K_LANES)


@functools.lru_cache(maxsize=None)
def view_sets(g=VIEW_G, dims=VIEW_DIMS, t=VIEW_T, placed=True):
    """The six distinct sets of the viewpoint cases: dict of tri int8 [6,G,G,G], range_gt, voxel_size, dims, lo, h, field uint32
    [6,M], targets int32 [6,T,3], r_min, r_max, max_unknown.  Fields of few costs, about 30 % of the nodes without a route.  With
    `placed` (the large lattice, whose window is the whole lattice, so that a node's slot is its id): the all-free set's cheapest
    cost stands on the nodes that wave 7 holds in every turn, all of them routed -- the winner is in wave 7 of the first turn and is
    tied with the same lane's later turns; the open set's cheapest cost stands on the nodes of the third turn alone."""
    tri5, rng5, vox5 = FC.grid_case(g)
    tri = np.concatenate([tri5, np.zeros((1, g, g, g), np.int8)])
    rng, vox = np.concatenate([rng5, rng5[:1]]), np.concatenate([vox5, vox5[:1]])
    dims, lo, h = view_lattice(dims)
    m = dims[0] * dims[1] * dims[2]
    rs = np.random.RandomState(500 + g + m)
    field = (rs.randint(0, 3, (D, m)) * 1000 + LOW).astype(np.uint32)
    unrouted = rs.rand(D, m) < 0.3
    if placed:
        c = np.arange(m)
        wave7 = (c % K_LANES) // K_WAVE == K_WAVES - 1
        field[V_FREE] = np.where(wave7, LOW, np.where(field[V_FREE] == LOW, MID, field[V_FREE]))
        unrouted[V_FREE] &= ~wave7
        field[V_OPEN] = np.where(c >= 2 * K_LANES, LOW, np.where(field[V_OPEN] == LOW, HIGH, field[V_OPEN]))
    field[unrouted] = NO_ROUTE
    targets = rs.randint(0, g, (D, t, 3)).astype(np.int32)
    if t >= 9:  # tests/frontview_cases.py's special targets
        targets[:, 5] = targets[:, 0]            # a duplicate target
        targets[:, 6, rs.randint(0, 3)] = -1     # outside: below
        targets[:, 7, rs.randint(0, 3)] = g      # outside: one past the end
        targets[:, 8] = (0, 0, g - 1)            # a corner
    out = dict(tri=tri, range_gt=rng, voxel_size=vox, dims=dims, lo=lo, h=h, field=field, targets=targets, r_min=0.0, r_max=VIEW_R_MAX,
               max_unknown=VIEW_MAX_UNKNOWN if placed else g)
    _frozen(tri, rng, vox, lo, h, field, targets)
    return out


@functools.lru_cache(maxsize=None)
def view_want(g=VIEW_G, dims=VIEW_DIMS, t=VIEW_T, placed=True):
    """The oracle's outputs for view_sets(...), read-only: node, cost, count, tied, in_range, each [6, T, ...].  A case of fewer
    targets takes the first of them: a target's outputs depend on nothing but the target."""
    c = view_sets(g, dims, t, placed)
    w = VO.viewpoints(c["tri"], c["range_gt"], c["voxel_size"], c["dims"], c["lo"], c["h"], c["field"], c["targets"], c["r_min"],
                      c["r_max"], c["max_unknown"])
    _frozen(*w.values())
    return w


VIEW_SWIZZLE_SETS = (V_SPARSE, V_OPEN)
VIEW_SWIZZLE_DIMS, VIEW_SWIZZLE_T = (7, 6, 5), 5  # frontview_cases.py's "box"
# id -> n, T, grid, [(mode, chunk)], the distinct sets; large: the 1287-node lattice with the placed fields
VIEW_CASES = {
    "t1-three-turns": dict(n=6, t=1, g=VIEW_G, runs=((1, 0), (1, 3), (2, 0), (2, 3), (0, 0)), sets=ALL_SETS, large=True),
    "t9-three-turns": dict(n=6, t=9, g=VIEW_G, runs=((1, 0), (1, 3), (2, 0), (2, 3), (0, 0)), sets=ALL_SETS, large=True),
    "t20-three-turns": dict(n=6, t=20, g=VIEW_G, runs=((1, 0), (1, 3), (2, 0), (2, 3), (0, 0)), sets=ALL_SETS, large=True),
    "n171-t20-m1-auto-chunk-7-ragged": dict(n=171, t=20, g=VIEW_G, runs=((1, 0),), sets=ALL_SETS, large=True),
    "n512-t20-m1-one-chunk": dict(n=512, t=20, g=VIEW_G, runs=((1, 0),), sets=ALL_SETS, large=True),
    "n171-t20-m2-one-target-per-workgroup": dict(n=171, t=20, g=VIEW_G, runs=((2, 0), (0, 0)), sets=ALL_SETS, large=True),
}
for _g in (44, 64, 86):
    VIEW_CASES[f"swizzle-g{_g}"] = dict(n=2, t=VIEW_SWIZZLE_T, g=_g, runs=((1, 0), (1, 2), (2, 0)), sets=VIEW_SWIZZLE_SETS, large=False)
VIEW_CASES["swizzle-g87-in-place-only"] = dict(n=2, t=VIEW_SWIZZLE_T, g=87, runs=((2, 0), (0, 0)), sets=VIEW_SWIZZLE_SETS, large=False)


def view_case_data(cid):
    """(the distinct sets' dict, the oracle's dict) of a case, both over all six sets and the pool's T targets."""
    c = VIEW_CASES[cid]
    key = (VIEW_G, VIEW_DIMS, VIEW_T, True) if c["large"] else (c["g"], VIEW_SWIZZLE_DIMS, VIEW_SWIZZLE_T, False)
    return view_sets(*key), view_want(*key)


def view_windows(cid):
    """{(set, target): window} of a case's in-grid targets."""
    c = VIEW_CASES[cid]
    s, _ = view_case_data(cid)
    g, out = c["g"], {}
    for d in c["sets"]:
        for j in range(c["t"]):
            tgt = s["targets"][d, j]
            if ((tgt >= 0) & (tgt < g)).all():
                out[(d, j)] = view_window(s["range_gt"][d], s["voxel_size"][d], tgt, s["r_max"], s["dims"], s["lo"], s["h"])
    return out


def window_nodes(w):
    return (w[1] - w[0] + 1) * (w[3] - w[2] + 1) * (w[5] - w[4] + 1)


def check_view_case(cid):
    c = VIEW_CASES[cid]
    s, w = view_case_data(cid)
    n, t, g = c["n"], c["t"], c["g"]
    m = int(np.prod(s["dims"]))
    windows = view_windows(cid)
    most = max(window_nodes(x) for x in windows.values())
    info = {}
    for mode, chunk in c["runs"]:
        v = view_shape(n, t, mode, g, chunk, most)
        info[(mode, chunk)] = dict(chunks=v.chunks, chunk_items=v.chunk_items, last_items=v.last_items, turns=v.turns, shift=v.shift,
                                   lds_bytes=v.lds_bytes)
        assert v.lds_bytes <= K_LDS_BYTES
        if c["large"]:
            # more than 1024 nodes lie inside r_max of a target: a lane takes three turns and all eight waves hold candidates
            assert int(w["in_range"][list(c["sets"]), :t].max()) > 2 * K_LANES and v.turns == 3
            assert all(x == (0, s["dims"][0] - 1, 0, s["dims"][1] - 1, 0, s["dims"][2] - 1) for x in windows.values())  # slot == node id
        if "auto-chunk-7-ragged" in cid:
            assert v.lds and v.cap == 3 and v.chunk_items == 7 and v.chunks == 3 and v.last_items == 6
        if "one-chunk" in cid:
            assert v.lds and v.cap == 1 and v.chunks == 1 and v.chunk_items == t
        if "one-target-per-workgroup" in cid:
            assert not v.lds and v.chunk_items == 1 and v.chunks == t and n * t > 512
        if "swizzle" in cid:
            assert v.lds == (mode == 1) and (mode != 1 or g <= view_lds_max_grid())
    if "in-place-only" in cid:
        assert g == view_lds_max_grid() + 1
    if c["n"] > len(c["sets"]):
        assert set(node_case_sets(c).tolist()) == set(c["sets"])
    return info

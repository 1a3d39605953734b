"""The inputs that tests/test_sweepmap_cpu.py (the robust share of the oracle) and tests/test_sweepmap_gpu.py (the kernel) share:
six envs with anisotropic voxel frames, their tri-class grids, K = 40 legs per env, and the oracle's distances computed once."""
import functools

import numpy as np

from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.flight import FlightLattice
from tests import sweepmap_oracle as SO

f32 = np.float32
N_ENVS, K = 6, 40
RADII = (0.23, 0.06)  # 0.06 is below every voxel edge of the 12^3 and 8^3 frames (>= 0.15 m; env 4: >= 0.033 m, above it)
FLAGS = [(u, o, gr) for u in (0, 1) for o in (0, 1) for gr in (0, 1)]
BIG_LO, BIG_HI = np.array([-1.4, 1.6, -0.3]), np.array([1.0, 4.2, 1.5])
SMALL_LO, SMALL_HI = np.array([-0.5, 2.5, 0.3]), np.array([0.1, 3.0, 0.7])


def lattice():
    """9 x 7 x 5, M = 315, unequal spacing: x in [-1, 0.6], y in [2, 3.8], z in [0.1, 1.1] (tests/test_flightmap_gpu.py's)."""
    cfg = TaskConfig(clip_pose_low=[-1.0, 2.0, 0.1, 0.0, 0.0, 0.0], clip_pose_idx_up=[8, 6, 4, 0, 12, 12],
                     action_unit=[0.2, 0.3, 0.25, 0.0, 0.1, 0.1])
    lat = FlightLattice(cfg, stride=1)
    assert lat.dims == (9, 7, 5) and lat.num_nodes == 315
    return lat


def frames(g):
    """range_gt [6,6] (max, min per axis: voxel centres) and voxel_size [6,3], anisotropic: envs 0-3 and 5 hold the lattice and most
    legs, env 4's grid is far smaller than the legs."""
    rng, vox = np.zeros((N_ENVS, 6), f32), np.zeros((N_ENVS, 3), f32)
    for e in range(N_ENVS):
        lo, hi = (SMALL_LO, SMALL_HI) if e == 4 else (BIG_LO - 0.01 * e, BIG_HI + 0.013 * e)
        v = (hi - lo) / g
        vox[e] = v
        rng[e, 1::2] = lo + 0.5 * v
        rng[e, 0::2] = hi - 0.5 * v
    return rng, vox


@functools.lru_cache(maxsize=None)
def case(g):
    """(tri int8 [6,G,G,G], range_gt, voxel_size): random thirds of -1 / 0 / 1 with the extremes -128 and 127, all free, all unknown,
    all occupied, the small grid (random thirds), a sparse grid (2.5 % occupied, 1.5 % unknown)."""
    rs = np.random.RandomState(100 + g)
    tri = rs.randint(-1, 2, (N_ENVS, g, g, g)).astype(np.int8)
    tri[1], tri[2], tri[3] = -1, 0, 1
    u = rs.rand(g, g, g)
    tri[5] = np.where(u < 0.025, 1, np.where(u < 0.04, 0, -1))
    ext = rs.rand(N_ENVS, g, g, g) < 0.3
    tri = np.where(ext & (tri < 0), -128, np.where(ext & (tri > 0), 127, tri)).astype(np.int8)
    assert (tri == -128).any() and (tri == 127).any() and (tri == 0).any()
    rng, vox = frames(g)
    for a in (tri, rng, vox):
        a.setflags(write=False)
    return tri, rng, vox


@functools.lru_cache(maxsize=None)
def legs(g):
    """(from f32 [6,40,6], to f32 [6,40,6], start f32 [6,6]): pose rows whose first three floats are the point.  Per env: 16 legs
    inside the large box, 6 crossing the whole grid, 6 with one end outside, 3 wholly outside, 6 axis-parallel, 2 of zero length
    (one inside, one outside), 1 with a NaN.  `start` is the one start per env of the broadcast form."""
    rs = np.random.RandomState(200 + g)
    frm, to = np.full((N_ENVS, K, 6), 7.0, f32), np.full((N_ENVS, K, 6), -7.0, f32)
    size = BIG_HI - BIG_LO
    for e in range(N_ENVS):
        inside = lambda m: BIG_LO + size * rs.rand(m, 3)  # noqa: E731
        a, b = inside(K), inside(K)
        for j in range(16, 22):  # across: from beyond one face to beyond the opposite one
            ax = j % 3
            a[j, ax], b[j, ax] = BIG_LO[ax] - 0.2 - 0.5 * rs.rand(), BIG_HI[ax] + 0.2 + 0.5 * rs.rand()
        for j in range(22, 28):  # one end outside
            ax, sign = j % 3, 1.0 if j < 25 else -1.0
            end = b if j % 2 else a
            end[j, ax] = (BIG_HI[ax] + 0.1 + rs.rand()) if sign > 0 else (BIG_LO[ax] - 0.1 - rs.rand())
        for j in range(28, 31):  # wholly outside, one of them passing close by a face
            ax = j % 3
            a[j, ax] = b[j, ax] = BIG_HI[ax] + (0.15 if j == 28 else 0.9) + 0.1 * rs.rand()
        for j in range(31, 37):  # axis-parallel: the two other coordinates equal
            ax = j % 3
            keep = a[j, ax]
            a[j] = b[j]
            a[j, ax] = keep
        b[37] = a[37]  # zero length, inside
        a[38] = b[38] = BIG_HI + np.array([0.05, -0.4, 0.05])  # zero length, just outside two faces
        b[39, 1] = np.nan
        frm[e, :, :3], to[e, :, :3] = a, b
    start = np.ascontiguousarray(frm[:, 3])
    for a in (frm, to, start):
        a.setflags(write=False)
    return frm, to, start


@functools.lru_cache(maxsize=None)
def dist(g, broadcast):
    """The oracle's least distances of the legs (tests/sweepmap_oracle.py min_dist), once per (grid, from-form)."""
    tri, rng, vox = case(g)
    frm, to, start = legs(g)
    return SO.min_dist(tri, rng, vox, start if broadcast else frm, to)


@functools.lru_cache(maxsize=None)
def want(g, broadcast, radius, flags):
    """(code uint8 [6,40], robust bool [6,40]) of the oracle."""
    tri, rng, vox = case(g)
    frm, to, start = legs(g)
    code, robust = SO.codes_from(dist(g, broadcast), g, rng, vox, start if broadcast else frm, to, radius, *[bool(f) for f in flags])
    code.setflags(write=False)
    robust.setflags(write=False)
    return code, robust


LIMIT_RADIUS = 0.12


@functools.lru_cache(maxsize=None)
def limit_case(g):
    """One env with a very sparse G^3 grid (a capsule holds thousands of voxels) and 8 random legs inside it, for the grids round the
    LDS limit and the largest one: (tri int8 [1,G,G,G], range_gt, voxel_size, from f32 [1,8,3], to f32 [1,8,3], code, robust) with
    unknown_blocks alone."""
    rs = np.random.RandomState(g)
    tri = rs.randint(-1, 2, (1, g, g, g)).astype(np.int8)
    tri[rs.rand(1, g, g, g) < 0.9999] = -1
    rng, vox = frames(g)
    rng, vox = rng[:1], vox[:1]
    frm = (BIG_LO + (BIG_HI - BIG_LO) * rs.rand(1, 8, 3)).astype(f32)
    to = (BIG_LO + (BIG_HI - BIG_LO) * rs.rand(1, 8, 3)).astype(f32)
    code, robust = SO.codes(tri, rng, vox, frm, to, LIMIT_RADIUS, True, False, False)
    return tri, rng, vox, frm, to, code, robust

"""The random cases of the frontier-viewpoint kernel tests (TEST INFRASTRUCTURE): built once per grid size, oracle results computed
once per (grid size, configuration) and shared read-only between tests/test_frontview_cpu.py -- which checks with the oracle alone
that the cases reach what they are there for -- and tests/test_frontview_gpu.py, which compares the kernel with them."""
import functools

import numpy as np

from tests import frontview_oracle as VO

GRIDS = (5, 20, 33, 87)  # 87: one above gnbv_frontview_lds_max_grid() (86), mode 2 only
RANDOM, SPARSE, FREE, OCCUPIED, OPEN = range(5)
N = 5
NO_ROUTE = 0xFFFFFFFF

# (lattice, T, r_min, r_max, max_unknown); max_unknown None = G.  Lattice "box" 7 x 6 x 5, "flat" 9 x 8 x 1 (a single-node axis),
# both sticking out of the grid on every side.  r_max 0.7 / 1.0 / 1.2: a window inside the lattice; 10: larger than the lattice.
CONFIGS = (
    ("box", 9, 0.0, 0.7, 0),
    ("box", 9, 0.5, 10.0, None),
    ("box", 3, 0.0, 10.0, 2),
    ("box", 1, 0.3, 1.2, 2),
    ("flat", 9, 0.0, 1.0, None),
    ("flat", 3, 0.4, 10.0, 0),
)
EXTENT = np.array([2.0, 2.4, 1.6])


@functools.lru_cache(maxsize=None)
def grid_case(g):
    """(tri int8 [N,G,G,G], range_gt f32 [N,6], voxel_size f32 [N,3]): random thirds of -1 / 0 / 1, sparse (5 % free, 3 % occupied in
    unknown space), all free, all occupied, open (90 % free, 5 % unknown, 5 % occupied); some values at the int8 extremes; a frame
    that differs per env and axis."""
    rs = np.random.RandomState(1000 + g)
    tri = rs.randint(-1, 2, (N, g, g, g)).astype(np.int8)
    u = rs.rand(g, g, g)
    tri[SPARSE] = np.where(u < 0.05, -1, np.where(u < 0.08, 1, 0))
    tri[FREE], tri[OCCUPIED] = -1, 1
    u = rs.rand(g, g, g)
    tri[OPEN] = np.where(u < 0.90, -1, np.where(u < 0.95, 0, 1))
    ext = rs.rand(*tri.shape) < 0.3
    tri = np.where(ext & (tri < 0), -128, np.where(ext & (tri > 0), 127, tri)).astype(np.int8)
    lo = -0.5 * EXTENT[None] + rs.uniform(-0.05, 0.05, (N, 3))
    hi = lo + EXTENT[None] * rs.uniform(0.95, 1.05, (N, 3))
    range_gt = np.empty((N, 6), np.float32)
    range_gt[:, 0::2], range_gt[:, 1::2] = hi, lo
    voxel_size = ((range_gt[:, 0::2] - range_gt[:, 1::2]) / np.float32(g)).astype(np.float32)
    for a in (tri, range_gt, voxel_size):
        a.setflags(write=False)
    return tri, range_gt, voxel_size


def lattice(name):
    """(dims, lo fp64 [3], h fp64 [3]): nodes from 0.4 m outside the nominal grid on every side (z of "flat": one node, h = 0)."""
    dims = (7, 6, 5) if name == "box" else (9, 8, 1)
    lo = -0.5 * EXTENT - 0.4
    h = np.array([(EXTENT[a] + 0.8) / (dims[a] - 1) if dims[a] > 1 else 0.0 for a in range(3)])
    if name == "flat":
        lo[2] = 0.1
    return dims, lo, h


@functools.lru_cache(maxsize=None)
def case(g, ci):
    """Everything one launch needs, host side: dict with tri, range_gt, voxel_size, dims, lo, h, field uint32 [N,M], targets int32
    [N,T,3], r_min, r_max, max_unknown."""
    name, t, r_min, r_max, mu = CONFIGS[ci]
    tri, range_gt, voxel_size = grid_case(g)
    dims, lo, h = lattice(name)
    m = dims[0] * dims[1] * dims[2]
    rs = np.random.RandomState(7 * g + ci)
    # about 30 % without a route, the rest from six values: many duplicates, so the tie rule decides winners
    field = (rs.randint(0, 6, (N, m)) * 1000 + 500).astype(np.uint32)
    field[rs.rand(N, m) < 0.3] = NO_ROUTE
    full = rs.randint(0, g, (N, 9, 3)).astype(np.int32)
    full[:, 5] = full[:, 0]             # a duplicate target
    full[:, 6, rs.randint(0, 3)] = -1   # outside: below
    full[:, 7, rs.randint(0, 3)] = g    # outside: one past the end
    full[:, 8] = (0, 0, g - 1)          # a corner
    if t == 9:
        targets = full
    elif t == 3:
        targets = full[:, [0, 6, 5]]
    else:
        targets = full[:, :1].copy()
        targets[OCCUPIED, 0] = (g, 0, 0)  # a whole env without a target
    out = dict(tri=tri, range_gt=range_gt, voxel_size=voxel_size, dims=dims, lo=lo, h=h, field=field,
               targets=np.ascontiguousarray(targets), r_min=r_min, r_max=r_max, max_unknown=g if mu is None else mu)
    for a in (field, out["targets"], lo, h):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(g, ci):
    """The oracle's outputs for case(g, ci), read-only."""
    c = case(g, ci)
    w = VO.viewpoints(c["tri"], c["range_gt"], c["voxel_size"], c["dims"], c["lo"], c["h"], c["field"], c["targets"], c["r_min"],
                      c["r_max"], c["max_unknown"])
    for a in w.values():
        a.setflags(write=False)
    return w

"""The blocked bits of gnbv_flight_blocked_tri (csrc/flightmap.hip) restated in plain numpy: fp64, the operation order of
include/gennbv_hip.h, one node at a time.  numpy never fuses a multiply with an add, so every intermediate is rounded as the
kernel's is and the comparison with the kernel is exact on every u32, padding bits included."""
import numpy as np

f32, f64 = np.float32, np.float64


def voxel_frame(range_gt, voxel_size):
    """(o [3], v [3]) fp64 of one env: o_a = (double)fp32(range_gt[2a+1] - fp32(0.5f * v_a)) as gnbv_pose_to_idx has it."""
    r, vs = np.asarray(range_gt, f32), np.asarray(voxel_size, f32)
    o = np.array([f32(r[2 * a + 1]) - f32(f32(0.5) * vs[a]) for a in range(3)], f32)
    return o.astype(f64), vs.astype(f64)


def axis_table(o, v, p, rho, g):
    """One axis, one node coordinate p: (i0, i1, empty, outside, gap^2 of the voxels i0..i1), all from fp64 scalars."""
    pm, pp = p - rho, p + rho
    f0, f1 = np.floor((pm - o) / v), np.floor((pp - o) / v)
    empty = bool(f1 < 0 or f0 > g - 1)
    i0, i1 = int(min(max(f0, 0.0), g - 1.0)), int(min(max(f1, 0.0), g - 1.0))
    outside = bool(pm < o or pp > o + f64(g) * v)
    i = np.arange(i0, i1 + 1).astype(f64)
    below = o + i * v - p
    above = p - (o + (i + 1.0) * v)
    gap = np.maximum(np.maximum(below, 0.0), above)
    return i0, i1, empty, outside, gap * gap


def node_blocked(tri, tx, ty, tz, pz, rho, unknown_blocks, outside_blocks, ground):
    """One node of one env's grid tri [G,G,G] (any signed dtype) from its three axis tables; pz its height."""
    if outside_blocks and (tx[3] or ty[3] or tz[3]):
        return True
    if ground and pz - rho <= 0.0:
        return True
    if tx[2] or ty[2] or tz[2]:
        return False
    touched = ((tx[4][:, None, None] + ty[4][None, :, None]) + tz[4][None, None, :]) <= rho * rho
    win = tri[tx[0]:tx[1] + 1, ty[0]:ty[1] + 1, tz[0]:tz[1] + 1]
    blocking = (win >= 0) if unknown_blocks else (win > 0)
    return bool((touched & blocking).any())


def blocked_bool(tri, range_gt, voxel_size, dims, lo, h, rho, unknown_blocks=False, outside_blocks=False, ground=False):
    """bool [N, M]: tri [N,G,G,G], range_gt [N,6], voxel_size [N,3]; the lattice dims / lo / h (fp64); node id (k ny + j) nx + i.
    A node's three axis tables depend on its index on that axis alone, so they are computed once per axis index."""
    tri = np.asarray(tri)
    n, g = tri.shape[0], tri.shape[1]
    nx, ny, nz = (int(d) for d in dims)
    lo, h, rho = np.asarray(lo, f64), np.asarray(h, f64), f64(rho)
    out = np.zeros((n, nx * ny * nz), bool)
    for e in range(n):
        o, v = voxel_frame(range_gt[e], voxel_size[e])
        pos = [[lo[a] + h[a] * f64(i) for i in range(d)] for a, d in enumerate((nx, ny, nz))]
        tab = [[axis_table(o[a], v[a], p, rho, g) for p in pos[a]] for a in range(3)]
        for c in range(nx * ny * nz):
            i, j, k = c % nx, (c // nx) % ny, c // (nx * ny)
            out[e, c] = node_blocked(tri[e], tab[0][i], tab[1][j], tab[2][k], pos[2][k], rho, unknown_blocks, outside_blocks, ground)
    return out


def pack_words(blocked):
    """bool [N, M] -> uint32 [N, ceil(M / 32)], bit c & 31 of word c >> 5, padding bits set."""
    n, m = blocked.shape
    words = (m + 31) // 32
    full = np.ones((n, words * 32), bool)
    full[:, :m] = blocked
    return (full.reshape(n, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def blocked_words(*args, **kw):
    return pack_words(blocked_bool(*args, **kw))

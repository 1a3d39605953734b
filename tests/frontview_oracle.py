"""CPU oracle of the frontier viewpoints (include/gennbv_hip.h gnbv_frontier_viewpoints), composed from the existing oracle only.

TEST INFRASTRUCTURE.  Per env and lattice node: `oracle.pose_to_idx` of the node's fp32 position gives the source voxel (saturated
at +-2^24 as the definition says), one `oracle.bresenham3d` call per node -- the node's voxel the source, the env's in-grid targets
the rays -- gives the in-grid voxels of every line in order, and numpy fp64 in the stated operation order gives the distance.  It
runs over ALL M nodes: no window, so a wrong window in the kernel shows.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

NO_ROUTE = 0xFFFFFFFF
CLAMP = 2 ** 24


def node_positions(dims, lo, h):
    """fp64 [M,3]: p_a = lo_a + h_a * idx_a of node c = (k ny + j) nx + i, in id order."""
    nx, ny, nz = (int(d) for d in dims)
    c = np.arange(nx * ny * nz, dtype=np.int64)
    idx = np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], -1).astype(np.float64)
    return np.asarray(lo, np.float64)[None] + np.asarray(h, np.float64)[None] * idx


def voxel_frame(range_gt, voxel_size):
    """(o [3], v [3]) fp64 of one env: v_a = (double)voxel_size[a], o_a = (double)fp32(range_gt[2a+1] - fp32(0.5f * voxel_size[a]))."""
    f32 = np.float32
    r, vs = np.asarray(range_gt, f32).reshape(6), np.asarray(voxel_size, f32).reshape(3)
    return (r[1::2] - f32(0.5) * vs).astype(f32).astype(np.float64), vs.astype(np.float64)


def viewpoints_env(tri, range_gt, voxel_size, dims, lo, h, field, targets, r_min, r_max, max_unknown):
    """One env: tri [g,g,g] (any signed dtype), field [M] uint32, targets [T,3] int -> (node int32 [T], cost uint32 [T],
    count int32 [T,2], tied bool [T]: another routed node that sees the target has the winner's field value -- the tie rule decided,
    in_range int64 [T]: the nodes in range, seen or not)."""
    tri = np.asarray(tri)
    g = tri.shape[0]
    cls = np.sign(tri.reshape(-1).astype(np.int64))
    field = np.asarray(field).astype(np.uint32).astype(np.int64)
    targets = np.asarray(targets, np.int64).reshape(-1, 3)
    t = targets.shape[0]
    pos = node_positions(dims, lo, h)
    m = pos.shape[0]
    o, v = voxel_frame(range_gt, voxel_size)
    rng = np.broadcast_to(np.asarray(range_gt, np.float32).reshape(1, 6), (m, 6))
    vox = np.broadcast_to(np.asarray(voxel_size, np.float32).reshape(1, 3), (m, 3))
    src = np.clip(O.pose_to_idx(pos.astype(np.float32), rng, vox), -CLAMP, CLAMP).astype(np.int32)
    is_target = ((targets >= 0) & (targets < g)).all(1)
    q = o[None] + (targets.astype(np.float64) + 0.5) * v[None]
    e = pos[:, None, :] - q[None, :, :]  # [M,T,3]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    in_range = (d2 >= float(r_min) * float(r_min)) & (d2 <= float(r_max) * float(r_max)) & is_target[None]
    sees = np.zeros((m, t), bool)
    for c in np.nonzero(in_range.any(1))[0]:
        js = np.nonzero(in_range[c])[0]
        traj, lens = O.bresenham3d(src[c], targets[js].astype(np.int32), g)
        for r, j in enumerate(js):
            line = traj[r, :lens[r]].astype(np.int64)
            assert lens[r] >= 1 and (line[-1] == targets[j]).all()  # w_L is the target
            w = cls[(line[:-1, 0] * g + line[:-1, 1]) * g + line[:-1, 2]]
            sees[c, j] = not (w > 0).any() and int((w == 0).sum()) <= int(max_unknown)
    routed = sees & (field != NO_ROUTE)[:, None]
    node = np.full(t, -1, np.int32)
    cost = np.full(t, NO_ROUTE, np.uint32)
    tied = np.zeros(t, bool)
    for j in range(t):
        cs = np.nonzero(routed[:, j])[0]
        if cs.size:
            best = cs[np.lexsort((cs, field[cs]))[0]]
            node[j], cost[j] = best, field[best]
            tied[j] = int((field[cs] == field[best]).sum()) > 1
    count = np.stack([sees.sum(0), routed.sum(0)], -1).astype(np.int32)
    return node, cost, count, tied, in_range.sum(0)


def viewpoints(tri, range_gt, voxel_size, dims, lo, h, field, targets, r_min, r_max, max_unknown):
    """tri [N,g,g,g], range_gt [N,6], voxel_size [N,3], field [N,M] uint32, targets [N,T,3] -> dict of node int32 [N,T], cost uint32
    [N,T], count int32 [N,T,2], tied bool [N,T], in_range int64 [N,T] (the nodes in range, seen or not)."""
    tri = np.asarray(tri)
    outs = [viewpoints_env(tri[e], np.asarray(range_gt)[e], np.asarray(voxel_size)[e], dims, lo, h, np.asarray(field)[e],
                           np.asarray(targets)[e], r_min, r_max, max_unknown) for e in range(tri.shape[0])]
    keys = ("node", "cost", "count", "tied", "in_range")
    return {k: np.stack([o[i] for o in outs]) for i, k in enumerate(keys)}

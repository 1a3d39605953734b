"""CPU oracle of the view gain (include/gennbv_hip.h gnbv_view_gain), composed from the existing oracle only.

TEST INFRASTRUCTURE.  Per env and candidate: `oracle.back_projection` of a constant-depth image (depth = range, seg 255 on
the lattice pixels) gives the ray ends, `oracle.pose_to_idx` the source and target voxels, `oracle.bresenham3d` the in-grid
voxels of every ray in order; numpy set operations give the three integers.  The camera matrices are an INPUT (the kernel's
`c2w_out`, or any other), so the oracle and the kernel start from the same bits.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O


def lattice(h: int, w: int, stride: int):
    """(us, vs): the pixel lattice u = stride // 2 + i * stride < w, v = stride // 2 + j * stride < h."""
    return np.arange(stride // 2, w, stride), np.arange(stride // 2, h, stride)


def lattice_count(h: int, w: int, stride: int) -> int:
    """Closed form of len(us) * len(vs)."""
    half = stride // 2
    nu = (w - half + stride - 1) // stride if half < w else 0
    nv = (h - half + stride - 1) // stride if half < h else 0
    return nu * nv


def ray_voxels(c2w, range_gt, voxel_size, inv_intri, h, w, stride, range_m, g):
    """One env, one candidate: c2w [4,4] -> (lin [R,3g] int64 linear voxel index of every visited in-grid voxel in order,
    valid [R,3g] bool).  R = lattice_count."""
    c2w = np.ascontiguousarray(c2w, np.float32).reshape(1, 4, 4)
    us, vs = lattice(h, w, stride)
    depth = np.full((1, h, w), np.float32(range_m), np.float32)
    seg = np.zeros((1, h, w), np.float32)
    seg[:, vs[:, None], us[None, :]] = 255.0
    world, fg = O.back_projection(depth, seg, c2w, inv_intri)
    rng = np.asarray(range_gt, np.float32).reshape(6)
    vox = np.asarray(voxel_size, np.float32).reshape(3)
    pts = world[0][fg[0]]  # row-major pixel order: v outer, u inner
    r = pts.shape[0]
    assert r == len(us) * len(vs)
    tgt = O.pose_to_idx(pts, np.broadcast_to(rng, (r, 6)), np.broadcast_to(vox, (r, 3)))
    src = O.pose_to_idx(c2w[0, :3, 3][None], rng[None], vox[None])[0]
    traj, lens = O.bresenham3d(src, tgt, g)  # [R,3g,3], [R]
    assert int(lens.max(initial=0)) <= g  # the 3g cap cannot trigger: one voxel per dominant-axis step
    t = traj.astype(np.int64)
    return (t[..., 0] * g + t[..., 1]) * g + t[..., 2], np.arange(3 * g)[None, :] < lens[:, None]


def view_gain_env(tri, c2w, range_gt, voxel_size, inv_intri, h, w, stride, range_m):
    """One env: tri [g,g,g] (any dtype; < 0 free, 0 unknown, > 0 occupied), c2w [K,4,4] -> gain [K,3] int32
    (unknown, unknown_hit, blocked)."""
    tri = np.asarray(tri)
    g = tri.shape[0]
    cls = np.sign(tri.reshape(-1).astype(np.int64))
    c2w = np.asarray(c2w, np.float32).reshape(-1, 4, 4)
    out = np.zeros((c2w.shape[0], 3), np.int32)
    if lattice_count(h, w, stride) == 0:
        return out
    steps = np.arange(3 * g)[None, :]
    for j in range(c2w.shape[0]):
        lin, valid = ray_voxels(c2w[j], range_gt, voxel_size, inv_intri, h, w, stride, range_m, g)
        c = cls[lin]
        occ = (c == 1) & valid
        blocked = occ.any(1)
        stop = np.where(blocked, occ.argmax(1), 3 * g)  # the first occupied voxel: not counted
        unk = valid & (steps < stop[:, None]) & (c == 0)
        out[j, 0] = np.unique(lin[unk]).size
        out[j, 1] = np.unique(lin[unk & blocked[:, None]]).size
        out[j, 2] = int(blocked.sum())
    return out


def view_gain(tri, c2w, range_gt, voxel_size, inv_intri, h, w, stride, range_m):
    """tri [N,g,g,g] or [N,g^3], c2w [N,K,4,4] (or [N,K,16]), range_gt [N,6], voxel_size [N,3] -> gain [N,K,3] int32."""
    tri = np.asarray(tri)
    n = tri.shape[0]
    g = round(tri[0].size ** (1.0 / 3.0))
    assert g ** 3 == tri[0].size
    c2w = np.asarray(c2w, np.float32).reshape(n, -1, 4, 4)
    return np.stack([view_gain_env(tri[e].reshape(g, g, g), c2w[e], np.asarray(range_gt)[e], np.asarray(voxel_size)[e],
                                   inv_intri, h, w, stride, range_m) for e in range(n)])

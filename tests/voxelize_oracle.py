"""fp64 brute-force surface voxelization oracle for gnbv_voxelize_surface (test infrastructure, CPU).

Voxel bounds as the updater bins points (csrc/voxel.hip k_pose_to_idx): per axis v = voxel_size[a] (fp32),
vmin = fp32(range_min[a] - fp32(0.5 * v)), voxel i = [vmin + i*v, vmin + (i+1)*v] in fp64.

`separation` returns, per voxel, the signed separation from the nearest triangle by the 13-axis separating-axis test
(3 box normals, the triangle normal, the 9 edge x box-axis cross products): max over the unit axes of the gap between
the two projections.  <= 0 means the closed box meets the closed triangle; > 0 is a lower bound of the Euclidean
distance.  Voxels farther than `reach` from every triangle's bounding box get +inf.
"""
from __future__ import annotations

import numpy as np
import torch


def voxel_bounds(range_gt_row, voxel_size_row, g: int):
    """(vmin [3] f32 as float64, v [3] as float64, face [3,g+1] float64 lower faces of voxels 0..g)."""
    v = np.asarray(voxel_size_row, dtype=np.float32)
    rmin = np.asarray(range_gt_row, dtype=np.float32)[[1, 3, 5]]
    vmin = (rmin - (np.float32(0.5) * v).astype(np.float32)).astype(np.float32)
    vmin64, v64 = vmin.astype(np.float64), v.astype(np.float64)
    face = vmin64[:, None] + np.arange(g + 1, dtype=np.float64)[None, :] * v64[:, None]
    return vmin64, v64, face


def _sat_gap(tri, c, h):
    """tri [P,3,3], c [P,3], h [P,3] float64 -> signed separation [P] (max over the 13 unit axes)."""
    v = tri - c[:, None, :]
    e = torch.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2]], 1)  # [P,3,3]
    eye = torch.eye(3, dtype=tri.dtype)
    axes = [eye[None, k].expand(tri.shape[0], 3) for k in range(3)]
    axes.append(torch.linalg.cross(e[:, 0], e[:, 1], dim=-1))
    for k in range(3):
        for j in range(3):
            axes.append(torch.linalg.cross(eye[None, k].expand(tri.shape[0], 3), e[:, j], dim=-1))
    best = torch.full((tri.shape[0],), -float("inf"), dtype=tri.dtype)
    for a in axes:
        norm = a.norm(dim=-1)
        p = (v * a[:, None, :]).sum(-1)  # [P,3]
        r = (h * a.abs()).sum(-1)
        gap = torch.maximum(p.amin(-1) - r, -r - p.amax(-1)) / norm
        gap = torch.where(norm > 0, gap, torch.full_like(gap, -float("inf")))
        best = torch.maximum(best, gap)
    return best


def separation(tris, range_gt_row, voxel_size_row, g: int, reach: float, chunk: int = 1 << 18) -> torch.Tensor:
    """[g,g,g] float64 signed separation of every voxel from the nearest of `tris` [T,3,3] (see the module docstring)."""
    tris = torch.as_tensor(tris).to(torch.float64).reshape(-1, 3, 3)
    _, v64, face = voxel_bounds(range_gt_row, voxel_size_row, g)
    face_t = torch.from_numpy(face)
    vmin = face_t[:, 0]
    v = torch.from_numpy(v64)
    out = torch.full((g * g * g,), float("inf"), dtype=torch.float64)
    if tris.shape[0] == 0:
        return out.reshape(g, g, g)
    tmin, tmax = tris.amin(1), tris.amax(1)
    i0 = torch.floor((tmin - reach - vmin) / v).to(torch.int64) - 1
    i1 = torch.floor((tmax + reach - vmin) / v).to(torch.int64) + 1
    i0, i1 = i0.clamp(0, g - 1), i1.clamp(-1, g - 1)
    span = (i1 - i0 + 1).clamp(min=0)
    per = span.prod(-1)
    tri_of = torch.repeat_interleave(torch.arange(tris.shape[0]), per)
    if tri_of.numel() == 0:
        return out.reshape(g, g, g)
    k = torch.arange(tri_of.numel()) - (torch.cumsum(per, 0) - per)[tri_of]
    sp = span[tri_of]
    ix = i0[tri_of, 0] + k % sp[:, 0]
    iy = i0[tri_of, 1] + (k // sp[:, 0]) % sp[:, 1]
    iz = i0[tri_of, 2] + k // (sp[:, 0] * sp[:, 1])
    for s in range(0, tri_of.numel(), chunk):
        sl = slice(s, s + chunk)
        ijk = torch.stack([ix[sl], iy[sl], iz[sl]], -1)
        lo = torch.stack([face_t[a][ijk[:, a]] for a in range(3)], -1)
        hi = torch.stack([face_t[a][ijk[:, a] + 1] for a in range(3)], -1)
        gap = _sat_gap(tris[tri_of[sl]], 0.5 * (lo + hi), 0.5 * (hi - lo))
        flat = (ijk[:, 0] * g + ijk[:, 1]) * g + ijk[:, 2]
        out.scatter_reduce_(0, flat, gap, "amin")
    return out.reshape(g, g, g)


def tau(range_gt_row) -> float:
    """The contract's false-positive allowance: 16 * 2^-23 * max |range_gt|."""
    return 16.0 * 2.0 ** -23 * float(np.abs(np.asarray(range_gt_row, dtype=np.float64)).max())


def check(grid, sep, t: float):
    """(false negatives, false positives beyond t, false positives within t) of a kernel grid [g,g,g] against the
    oracle's separation."""
    on = torch.as_tensor(grid).cpu() > 0.5
    fn = int((~on & (sep <= 0)).sum())
    fp_far = int((on & (sep > t)).sum())
    fp_near = int((on & (sep > 0) & (sep <= t)).sum())
    return fn, fp_far, fp_near

"""CPU oracle of the view gain of a measured frame (include/gennbv_hip.h GnbvViewGain depth_raw / carve_i8) and of
ops/carve.py CarvedMap, composed from the existing oracle and tests/view_gain_oracle.py.

TEST INFRASTRUCTURE.  Per env and candidate: the ray of lattice pixel (u, v) with raw depth r is SURFACE-ENDED iff r is finite,
r != 0, r > depth_sense_dist and |r| <= range, with length |r|; every other ray is RANGE-ENDED with length `range`.
`oracle.back_projection` of the image of those lengths (seg 255 on the lattice pixels) gives the ray ends, `oracle.pose_to_idx`
the source and target voxels, `oracle.bresenham3d` the in-grid voxels of every ray in order; the stop rule is
`view_gain_oracle.view_gain_env`'s, and on a surface-ended ray a visited voxel equal to the target voxel is left out.  numpy set
operations give the three integers, the two masks and the carve set.  The camera matrices are an INPUT (the kernel's `c2w_out`,
or any other), so the oracle and the kernel start from the same bits.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import oracle as O
from tests import gain_masks_oracle as MO
from tests import view_gain_oracle as VO


def ray_lengths(depth_raw, sense_dist, range_m):
    """depth_raw [...] f32 -> (length f32, surface bool): the rule of the header, elementwise."""
    r = np.asarray(depth_raw, np.float32)
    with np.errstate(invalid="ignore"):
        surface = np.isfinite(r) & (r != 0) & (r > np.float32(sense_dist)) & (np.abs(r) <= np.float32(range_m))
    return np.where(surface, np.abs(r), np.float32(range_m)).astype(np.float32), surface


@dataclass
class Rays:
    """One env, one candidate; R = lattice_count rays in row-major pixel order (v outer, u inner)."""
    lin: np.ndarray      # [R, 3g] int64 linear index of every visited in-grid voxel in order
    valid: np.ndarray    # [R, 3g] bool
    tgt_lin: np.ndarray  # [R] int64 linear index of the target voxel, -1 outside the grid
    surface: np.ndarray  # [R] bool
    us: np.ndarray       # [R] pixel column
    vs: np.ndarray       # [R] pixel row


def ray_voxels(c2w, depth_raw, range_gt, voxel_size, inv_intri, h, w, stride, range_m, sense_dist, g) -> Rays:
    """view_gain_oracle.ray_voxels with every pixel's own length; depth_raw [h, w]."""
    c2w = np.ascontiguousarray(c2w, np.float32).reshape(1, 4, 4)
    us, vs = VO.lattice(h, w, stride)
    length, surface = ray_lengths(np.asarray(depth_raw, np.float32).reshape(1, h, w), sense_dist, range_m)
    seg = np.zeros((1, h, w), np.float32)
    seg[:, vs[:, None], us[None, :]] = 255.0
    world, fg = O.back_projection(length, seg, c2w, inv_intri)
    rng = np.asarray(range_gt, np.float32).reshape(6)
    vox = np.asarray(voxel_size, np.float32).reshape(3)
    pts = world[0][fg[0]]
    r = pts.shape[0]
    assert r == len(us) * len(vs)
    tgt = O.pose_to_idx(pts, np.broadcast_to(rng, (r, 6)), np.broadcast_to(vox, (r, 3)))
    src = O.pose_to_idx(c2w[0, :3, 3][None], rng[None], vox[None])[0]
    traj, lens = O.bresenham3d(src, tgt, g)
    assert int(lens.max(initial=0)) <= g
    t = traj.astype(np.int64)
    inside = ((tgt >= 0) & (tgt < g)).all(1)
    tgt_lin = np.where(inside, (tgt[:, 0] * g + tgt[:, 1]) * g + tgt[:, 2], -1)
    vv, uu = np.meshgrid(vs, us, indexing="ij")
    return Rays((t[..., 0] * g + t[..., 1]) * g + t[..., 2], np.arange(3 * g)[None, :] < lens[:, None], tgt_lin,
                surface.reshape(h, w)[vv, uu].reshape(-1), uu.reshape(-1), vv.reshape(-1))


@dataclass
class RayFates:
    """What the stop rule makes of Rays against one grid."""
    blocked: np.ndarray   # [R] bool: met an occupied voxel
    unk: np.ndarray       # [R, 3g] bool: the unknown voxels the ray marks
    excluded: np.ndarray  # [R] bool: the target voxel was reached, is unknown, and was left out (surface-ended rays only)


def ray_fates(cls, rays: Rays) -> RayFates:
    """cls [g^3] int64 in {-1, 0, 1}."""
    g3 = rays.lin.shape[1]
    steps = np.arange(g3)[None, :]
    c = cls[rays.lin]
    occ = (c == 1) & rays.valid
    blocked = occ.any(1)
    stop = np.where(blocked, occ.argmax(1), g3)  # the first occupied voxel: not counted
    reached = rays.valid & (steps < stop[:, None])
    at_target = rays.surface[:, None] & (rays.lin == rays.tgt_lin[:, None]) & reached
    unk = reached & (c == 0) & ~at_target
    return RayFates(blocked, unk, (at_target & (c == 0)).any(1))


def measured_env(tri, c2w, depth_raw, range_gt, voxel_size, inv_intri, h, w, stride, range_m, sense_dist, words):
    """One env: tri [g^3] or [g,g,g], c2w [K,4,4], depth_raw [K,h,w] -> (gain [K,3] int32, unknown_bits, hit_bits uint32
    [K, words], carve bool [g^3]: the union of the candidates' unknown sets)."""
    tri = np.asarray(tri)
    g = round(tri.size ** (1.0 / 3.0))
    cls = np.sign(tri.reshape(-1).astype(np.int64))
    c2w = np.asarray(c2w, np.float32).reshape(-1, 4, 4)
    k = c2w.shape[0]
    gain = np.zeros((k, 3), np.int32)
    ub, hb = np.zeros((k, words), np.uint32), np.zeros((k, words), np.uint32)
    carve = np.zeros(g ** 3, bool)
    if VO.lattice_count(h, w, stride) == 0:
        return gain, ub, hb, carve
    depth_raw = np.asarray(depth_raw, np.float32).reshape(k, h, w)
    for j in range(k):
        rays = ray_voxels(c2w[j], depth_raw[j], range_gt, voxel_size, inv_intri, h, w, stride, range_m, sense_dist, g)
        f = ray_fates(cls, rays)
        u, hit = np.unique(rays.lin[f.unk]), np.unique(rays.lin[f.unk & f.blocked[:, None]])
        gain[j] = (u.size, hit.size, int(f.blocked.sum()))
        ub[j], hb[j] = MO.bits_of(u, words), MO.bits_of(hit, words)
        carve[u] = True
    return gain, ub, hb, carve


def measured(tri, c2w, depth_raw, range_gt, voxel_size, inv_intri, h, w, stride, range_m, sense_dist, words=None):
    """tri [N, g^3] (or [N,g,g,g]), c2w [N,K,4,4], depth_raw [N,K,h,w] -> (gain [N,K,3], unknown_bits, hit_bits [N,K,words],
    carve bool [N, g^3])."""
    tri = np.asarray(tri)
    n = tri.shape[0]
    g = round(tri[0].size ** (1.0 / 3.0))
    assert g ** 3 == tri[0].size
    words = MO.min_words(g) if words is None else int(words)
    c2w = np.asarray(c2w, np.float32).reshape(n, -1, 4, 4)
    depth_raw = np.asarray(depth_raw, np.float32).reshape(n, c2w.shape[1], h, w)
    out = [measured_env(tri[e], c2w[e], depth_raw[e], np.asarray(range_gt)[e], np.asarray(voxel_size)[e], inv_intri, h, w, stride,
                        range_m, sense_dist, words) for e in range(n)]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def merge(map_i8, tri, reset=None):
    """CarvedMap.update step 1 in numpy: map = where(reset | tri != 0, tri, map), tri taken by sign.  [N, g^3] int8."""
    map_i8 = np.asarray(map_i8, np.int8)
    t = np.sign(np.asarray(tri).reshape(map_i8.shape)).astype(np.int8)
    take = t != 0
    if reset is not None:
        take = take | np.asarray(reset).astype(bool).reshape(-1, 1)
    return np.where(take, t, map_i8)


def carved_update(map_i8, tri, depth_raw, c2w, range_gt, voxel_size, inv_intri, h, w, stride, range_m, sense_dist, reset=None):
    """One CarvedMap.update: the merge, then the measured frame of each env's own camera (k = 1) carved into the merged map.
    c2w [N,4,4], depth_raw [N,h,w] -> (map int8 [N, g^3], newly carved voxels [N] int32)."""
    m = merge(map_i8, tri, reset)
    n = m.shape[0]
    gain, _, _, carve = measured(m, np.asarray(c2w, np.float32).reshape(n, 1, 4, 4), np.asarray(depth_raw).reshape(n, 1, h, w), range_gt,
                                 voxel_size, inv_intri, h, w, stride, range_m, sense_dist)
    assert not (carve & (m != 0)).any()  # only unknown voxels are carved
    return np.where(carve, np.int8(-1), m), gain[:, 0, 0]

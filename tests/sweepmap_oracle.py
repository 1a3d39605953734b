"""CPU oracle of the swept sphere on the scanned map (csrc/sweepmap.hip, gnbv_sweep_tri) in fp64 numpy.  Test infrastructure.

The contract (include/gennbv_hip.h): the flight a -> b of a sphere of radius R touches the map (MAP = 1) when some blocking voxel
(occupied, or unknown with unknown_blocks) has dist(segment, closed box) <= R; it leaves the grid (OUTSIDE = 2) when
outside_blocks and on some axis min(a, b) - R < o or max(a, b) + R > o + G v; it reaches the ground (GROUND = 4) when ground and
min(a_z, b_z) - R <= 0.  An item with a non-finite coordinate has code 0.

Brute force over the env's blocking voxels: no windows, no pieces, and not the kernel's closed form.  s -> dist(a + s (b - a), box)
is convex on [0, 1] (the distance to a convex set along a line), so it is minimised by golden section, with the two ends added,
on top of the plain point-box distance.  45 iterations leave an interval of 0.618^45 ~ 4e-10 of the segment; the distance is
1-Lipschitz in the point, so the minimum is off by less than 4e-10 * |b - a|: far inside the band below.

The MAP predicate is monotone in R: an item is `robust` when the answers at R - d and R + d agree, d = 1e-6 m.  Robust items
must match the kernel bit for bit, the others may differ in bit 0 only; OUTSIDE and GROUND are closed forms in the kernel's own
operation order and are compared exactly on every item.

The minimum distance of a leg to the blocking voxels does not depend on R or on the two other flags, so it is computed once
(`min_dist`) and shared: `codes_from` turns it into codes for any radius and flag triple.
"""
from __future__ import annotations

import math

import numpy as np

from tests.flightmap_oracle import voxel_frame

f32, f64 = np.float32, np.float64
MAP, OUTSIDE, GROUND = 1, 2, 4
BAND = 1e-6
_GOLD = (math.sqrt(5.0) - 1.0) / 2.0


def point_box(p, lo, hi):
    """Distance of points p [..., 3] to the closed boxes [lo, hi] [..., 3]."""
    g = np.maximum(np.maximum(lo - p, 0.0), p - hi)
    return np.sqrt((g * g).sum(-1))


def segment_box(a, b, lo, hi, iters=45):
    """min over s in [0, 1] of point_box(a + s (b - a), box), broadcast over the leading dims: golden section plus the two ends."""
    if np.array_equal(a, b):  # zero length: the function of s is constant
        return point_box(a, lo, hi)
    d = b - a
    shape = np.broadcast(a[..., 0], lo[..., 0]).shape
    f = lambda s: point_box(a + d * s[..., None], lo, hi)  # noqa: E731
    s_lo, s_hi = np.zeros(shape), np.ones(shape)
    best = np.minimum(point_box(a, lo, hi), point_box(b, lo, hi))
    x1, x2 = s_hi - _GOLD * (s_hi - s_lo), s_lo + _GOLD * (s_hi - s_lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(iters):
        best = np.minimum(best, np.minimum(f1, f2))
        left = f1 <= f2  # the minimum lies in [s_lo, x2]; else in [x1, s_hi]
        s_lo, s_hi = np.where(left, s_lo, x1), np.where(left, x2, s_hi)
        n1, n2 = s_hi - _GOLD * (s_hi - s_lo), s_lo + _GOLD * (s_hi - s_lo)
        f1, f2 = f(n1), f(n2)
        x1, x2 = n1, n2
    return np.minimum(best, np.minimum(f1, f2))


def env_min_dist(tri, o, v, a, b, unknown_blocks):
    """[K] fp64: the least distance of each leg a[j] -> b[j] (fp64 [K,3], finite) to a blocking voxel of tri [G,G,G]; inf where the
    grid holds none."""
    blocking = np.argwhere((tri >= 0) if unknown_blocks else (tri > 0)).astype(f64)  # [V,3]
    k = a.shape[0]
    out = np.full(k, np.inf)
    if blocking.shape[0] == 0 or k == 0:
        return out
    lo, hi = o + blocking * v, o + (blocking + 1.0) * v
    step = max(1, 400000 // blocking.shape[0])
    for j0 in range(0, k, step):
        aa, bb = a[j0:j0 + step, None, :], b[j0:j0 + step, None, :]
        out[j0:j0 + step] = segment_box(aa, bb, lo[None], hi[None]).min(axis=1)
    return out


def _legs(frm, to, n, k):
    to = np.asarray(to, f32)[..., :3].astype(f64)
    frm = np.asarray(frm, f32)[..., :3].astype(f64)
    if frm.ndim == 2:
        frm = np.broadcast_to(frm[:, None, :], (n, k, 3))
    assert to.shape == (n, k, 3) and frm.shape == (n, k, 3)
    return frm, to


def min_dist(tri, range_gt, voxel_size, frm, to, unknown=(False, True)):
    """{unknown_blocks: fp64 [N,K]} for the values of the flag asked for: tri [N,G,G,G] (any signed dtype), frm [N,3] or [N,K,3],
    to [N,K,3] (fp32 values).  Items with a non-finite coordinate hold NaN."""
    tri = np.asarray(tri)
    n, k = tri.shape[0], np.asarray(to).shape[1]
    a, b = _legs(frm, to, n, k)
    finite = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    out = {bool(unk): np.full((n, k), np.nan) for unk in unknown}
    for e in range(n):
        o, v = voxel_frame(range_gt[e], voxel_size[e])
        idx = np.nonzero(finite[e])[0]
        for unk in out:
            out[unk][e, idx] = env_min_dist(tri[e], o, v, a[e, idx], b[e, idx], unk)
    return out


def codes_from(dist, g, range_gt, voxel_size, frm, to, radius, unknown_blocks=False, outside_blocks=False, ground=False):
    """(code uint8 [N,K], robust bool [N,K]) from min_dist's result."""
    d = dist[bool(unknown_blocks)]
    n, k = d.shape
    a, b = _legs(frm, to, n, k)
    finite = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    radius = f64(radius)
    with np.errstate(invalid="ignore"):
        hit, hit_lo, hit_hi = d <= radius, d <= radius - BAND, d <= radius + BAND
        code = np.where(hit, MAP, 0).astype(np.uint8)
        mn, mx = np.minimum(a, b), np.maximum(a, b)
        if outside_blocks:
            for e in range(n):
                o, v = voxel_frame(range_gt[e], voxel_size[e])
                out = ((mn[e] - radius < o) | (mx[e] + radius > o + f64(g) * v)).any(-1)
                code[e] |= np.where(out, OUTSIDE, 0).astype(np.uint8)
        if ground:
            code |= np.where(mn[..., 2] - radius <= 0.0, GROUND, 0).astype(np.uint8)
    code = np.where(finite, code, 0).astype(np.uint8)
    return code, (hit_lo == hit_hi) | ~finite


def codes(tri, range_gt, voxel_size, frm, to, radius, unknown_blocks=False, outside_blocks=False, ground=False):
    tri = np.asarray(tri)
    return codes_from(min_dist(tri, range_gt, voxel_size, frm, to, (unknown_blocks,)), tri.shape[1], range_gt, voxel_size, frm, to, radius,
                      unknown_blocks, outside_blocks, ground)


def agrees(got, want, robust):
    """The comparison rule: robust items bit for bit, the others in every bit but MAP."""
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.array_equal(got[robust], want[robust]) and np.array_equal(got & ~np.uint8(MAP), want & ~np.uint8(MAP)))

"""CPU oracle of the swept flight path (csrc/sweep.hip, gnbv_sweep_sphere) in fp64 numpy.  Test infrastructure.

The contract (include/gennbv_hip.h): the flight a -> b of a sphere of radius R is blocked (PATH = 8) when some closed triangle
of the env has dist(segment, T) <= R, and reaches the ground (PATH_GROUND = 16) when ground is on and min(a_z, b_z) - R <= 0.

Brute force over the env's triangles, no cells, and not the kernel's feature decomposition: s -> dist(a + s (b - a), T) is convex
on [0, 1] (the distance to a convex set along a line), so it is minimised by golden section, with the two ends added, on top
of a plain point-triangle distance.  45 iterations leave an interval of 0.618^45 ~ 4e-10 of the segment; the distance is
1-Lipschitz in the point, so the minimum is off by less than 4e-10 * |b - a|: 1e-8 m for a 25 m flight, a hundredth of the
band below.

The predicate is monotone in R: a case is `robust` when the answers at R - d and R + d agree, d = 1e-6 m.  Only robust cases
must match the kernel, and there bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
PATH, PATH_GROUND = 8, 16
BAND = 1e-6
_GOLD = (math.sqrt(5.0) - 1.0) / 2.0


def _dot(a, b):
    return np.einsum("...d,...d->...", a, b)


def _point_segment(p, a, b):
    d = b - a
    dd = _dot(d, d)
    t = np.clip(np.where(dd > 0, _dot(p - a, d) / np.where(dd > 0, dd, 1.0), 0.0), 0.0, 1.0)
    return np.linalg.norm(p - (a + d * t[..., None]), axis=-1)


def point_triangle(p, t):
    """Distance of points p [..., 3] to closed triangles t [..., 3, 3] (degenerate: its segment or point)."""
    v0, v1, v2 = t[..., 0, :], t[..., 1, :], t[..., 2, :]
    best = np.minimum(np.minimum(_point_segment(p, v0, v1), _point_segment(p, v1, v2)), _point_segment(p, v2, v0))
    n = np.cross(v1 - v0, v2 - v0)
    nn = _dot(n, n)
    ok = nn > 0
    inside = ok & (_dot(np.cross(v1 - v0, p - v0), n) >= 0) & (_dot(np.cross(v2 - v1, p - v1), n) >= 0) & (_dot(np.cross(v0 - v2, p - v2), n) >= 0)
    plane = np.abs(_dot(p - v0, n)) / np.sqrt(np.where(ok, nn, 1.0))
    return np.where(inside, np.minimum(best, plane), best)


def segment_triangle(a, b, t, iters=45):
    """min over s in [0, 1] of point_triangle(a + s (b - a), t): golden section plus the two ends."""
    d = b - a
    f = lambda s: point_triangle(a + d * s[..., None], t)  # noqa: E731
    lo, hi = np.zeros(a.shape[:-1]), np.ones(a.shape[:-1])
    best = np.minimum(f(lo), f(hi))
    x1, x2 = hi - _GOLD * (hi - lo), lo + _GOLD * (hi - lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(iters):
        left = f1 <= f2  # the minimum lies in [lo, x2]; else in [x1, hi]
        best = np.minimum(best, np.minimum(f1, f2))
        hi = np.where(left, x2, hi)
        lo = np.where(left, lo, x1)
        nx1, nx2 = hi - _GOLD * (hi - lo), lo + _GOLD * (hi - lo)
        x1, x2 = nx1, nx2
        f1, f2 = f(x1), f(x2)
    return np.minimum(best, np.minimum(f1, f2))


class SweepOracle:
    """tris: one [T_e,3,3] array per env (fp32 values)."""

    def __init__(self, tris):
        self.tris = [np.asarray(t, f32).astype(np.float64).reshape(-1, 3, 3) for t in tris]

    @staticmethod
    def from_mesh(mesh):
        return SweepOracle([mesh.env_triangles(e)[0].detach().cpu().numpy() for e in range(mesh.num_envs)])

    def distances(self, env, a, b, reach):
        """Smallest dist(segment, T) [M] over the triangles of env [M] (inf where there is none within `reach`: a triangle whose
        AABB misses the segment's AABB grown by `reach`, or whose bounding sphere stays further than `reach` from the segment,
        cannot matter to a radius <= reach and is left out)."""
        env = np.asarray(env, np.int64).reshape(-1)
        a = np.asarray(a, f32)[:, :3].astype(np.float64)
        b = np.asarray(b, f32)[:, :3].astype(np.float64)
        out = np.full(env.shape[0], np.inf)
        for e in np.unique(env):
            me = np.nonzero(env == e)[0]
            t = self.tris[e]
            if t.shape[0] == 0:
                continue
            tmin, tmax = t.min(1), t.max(1)
            centre = t.mean(1)
            rad = np.linalg.norm(t - centre[:, None], axis=-1).max(1)
            lo, hi = np.minimum(a[me], b[me]) - reach, np.maximum(a[me], b[me]) + reach
            with np.errstate(invalid="ignore"):
                ov = ((tmax[None] >= lo[:, None]) & (tmin[None] <= hi[:, None])).all(-1)  # [Me, T]
                ov &= _point_segment(centre[None], a[me][:, None], b[me][:, None]) - rad[None] <= reach + 1e-9
            pm, pt = np.nonzero(ov)
            if pm.size == 0:
                continue
            dist = segment_triangle(a[me][pm], b[me][pm], t[pt])
            np.minimum.at(out, me[pm], dist)
        return out

    def robust_codes(self, env, a, b, radius, ground=False, episode_length=None):
        """(codes [M] u8 at the kernel's fp32 radius, robust mask [M]) of the flights a -> b [M, >= 3] (fp32 values) in envs env [M];
        episode_length [M]: items with a value <= 1 get 0."""
        R = float(f32(radius))
        a32, b32 = np.asarray(a, f32)[:, :3], np.asarray(b, f32)[:, :3]
        dist = self.distances(env, a32, b32, R + 1e-3)
        zmin = np.minimum(a32[:, 2], b32[:, 2]).astype(np.float64)

        def at(r):
            return ((dist <= r).astype(np.uint8) * PATH) | ((bool(ground) & (zmin - r <= 0.0)).astype(np.uint8) * PATH_GROUND)
        keep = np.isfinite(a32).all(1) & np.isfinite(b32).all(1)
        if episode_length is not None:
            keep &= np.asarray(episode_length).reshape(-1) > 1
        code = np.where(keep, at(R), 0).astype(np.uint8)
        robust = ~keep | (at(R - BAND) == at(R + BAND))
        return code, robust

    def codes(self, env, a, b, radius, ground=False, episode_length=None):
        return self.robust_codes(env, a, b, radius, ground, episode_length)[0]


# ---------------------------------------------------------------------------
# hand cases with the answer known by construction: (name, triangles [T,3,3], a [3], b [3], radius, ground, expected code)
# ---------------------------------------------------------------------------
def hand_cases():
    from tests.collision_oracle import _box
    R, D = 0.1, 1e-3
    box = _box([-1, -1, 4], [1, 1, 6])
    none = np.zeros((0, 3, 3), f32)
    cases = []
    for sign, want in ((+1, 0), (-1, PATH)):
        g = R + sign * D
        tag = "free" if sign > 0 else "blocked"
        # parallel to the face x = 1
        cases.append((f"parallel_face_{tag}", box, [1 + g, -0.5, 5.0], [1 + g, 0.5, 5.5], R, False, want))
        # ending short of the face x = 1
        cases.append((f"short_of_face_{tag}", box, [3.0, 0.0, 5.0], [1 + g, 0.0, 5.0], R, False, want))
        # passing the edge x = 1, z = 6 (along y) at distance g: through the edge point + g (1, 0, 1) / sqrt 2, along (1, 0, -1)
        c = g / math.sqrt(2.0)
        cases.append((f"edge_{tag}", box, [1 + c - 1.5, 0.2, 6 + c + 1.5], [1 + c + 1.5, 0.2, 6 + c - 1.5], R, False, want))
        # passing the corner (1, 1, 6) at distance g: through corner + g (1, 1, 1) / sqrt 3, along (1, -1, 0)
        c = g / math.sqrt(3.0)
        cases.append((f"corner_{tag}", box, [1 + c - 1.5, 1 + c + 1.5, 6 + c], [1 + c + 1.5, 1 + c - 1.5, 6 + c], R, False, want))
        # a zero-length segment: the sphere test
        cases.append((f"zero_length_{tag}", box, [1 + g, 0.0, 5.0], [1 + g, 0.0, 5.0], R, False, want))
        # degenerate triangles: a segment and a point
        seg = np.array([[[-1, 0, 5], [1, 0, 5], [1, 0, 5]]], f32)
        cases.append((f"degenerate_segment_{tag}", seg, [0.0, g, 4.0], [0.0, g, 6.0], R, False, want))
        pt = np.array([[[0.5, 0.5, 5.0]] * 3], f32)
        cases.append((f"degenerate_point_{tag}", pt, [-1.0, 0.5, 5 + g], [2.0, 0.5, 5 + g], R, False, want))
        # the ground at min z = R +- D
        cases.append((f"ground_{tag}", none, [0.0, 0.0, 2.0], [1.0, 0.0, g], R, True, PATH_GROUND if sign < 0 else 0))
    cases.append(("ground_off", none, [0.0, 0.0, 2.0], [1.0, 0.0, 0.05], R, False, 0))
    # piercing a face of the box, and the interior of one large triangle (every edge and both ends far away)
    cases.append(("pierce_box_face", box, [2.0, 0.0, 5.0], [0.0, 0.0, 5.0], R, False, PATH))
    big = np.array([[[-3, -3, 5], [3, -3, 5], [0, 4, 5]]], f32)
    cases.append(("pierce_triangle", big, [0.2, 0.1, 6.0], [0.3, 0.0, 4.0], R, False, PATH))
    cases.append(("stop_above_triangle", big, [0.2, 0.1, 6.0], [0.3, 0.0, 5.0 + R + D], R, False, 0))
    cases.append(("stop_on_triangle", big, [0.2, 0.1, 6.0], [0.3, 0.0, 5.0 + R - D], R, False, PATH))
    # blocked and on the ground at once
    cases.append(("path_and_ground", box + np.array([0, 0, -4], f32), [3.0, 0.0, 0.05], [0.0, 0.0, 0.05], R, True, PATH | PATH_GROUND))
    return cases

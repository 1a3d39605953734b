"""CPU oracle of collision termination (csrc/collide.hip, gnbv_collide_cylinder) in fp64 numpy.

TEST INFRASTRUCTURE ONLY.  The same contract as the kernel, by a different algorithm:

  (S) every (body, triangle) pair whose AABBs overlap: Sutherland-Hodgman clip of the triangle to the slab
      |(x - c).a| <= h, projection of the clipped polygon onto the plane perpendicular to a, then the body is hit iff the
      centre lies inside the projected convex polygon (nonzero area) or within r of one of its edges (2-D);
  (I) (S) is false and, for some object whose closed AABB holds the centre, |sum of solid angles| / 4 pi >= 1/2;
  (G) ground and c_z - (r sqrt(1 - a_z^2) + h |a_z|) <= 0.

(S) is monotone in r and h, so a case is robust when the codes at (r - d, h - d) and (r + d, h + d) agree, d = 1e-9 x the
scene extent: only robust cases must match the kernel bit for bit (`robust_codes`).
"""
from __future__ import annotations

import math

import numpy as np

SURFACE, INSIDE, GROUND = 1, 2, 4
f32 = np.float32


def axes(poses: np.ndarray) -> np.ndarray:
    """a = Rz(yaw) Ry(pitch) Rx(roll) e_z in fp64 from the fp32 pose values [M, >= 6]."""
    p = np.asarray(poses, f32).astype(np.float64)
    cr, sr, cp, sp, cy, sy = np.cos(p[:, 3]), np.sin(p[:, 3]), np.cos(p[:, 4]), np.sin(p[:, 4]), np.cos(p[:, 5]), np.sin(p[:, 5])
    return np.stack([cy * sp * cr + sy * sr, sy * sp * cr - cy * sr, cp * cr], -1)


def _clip(poly, cnt, s, h):
    """Keep the part of each convex polygon [P,K,3] (cnt [P] vertices) where s * (x . a) <= h (a per row, in the caller's
    closure: s is [P,K] signed heights already multiplied by the sign)."""
    P, K = poly.shape[:2]
    out = np.zeros((P, K + 1, 3))
    oc = np.zeros(P, np.int64)
    ar = np.arange(P)
    f = s - h[:, None]
    for i in range(K):
        valid = i < cnt
        j = np.where(i + 1 < cnt, i + 1, 0)
        cur, nxt = poly[:, i], poly[ar, j]
        fc, fn = f[:, i], f[ar, j]
        cin, nin = fc <= 0, fn <= 0
        m = valid & cin
        out[ar[m], oc[m]] = cur[m]
        oc[m] += 1
        m = valid & (cin != nin)
        t = fc[m] / (fc[m] - fn[m])
        out[ar[m], oc[m]] = cur[m] + t[:, None] * (nxt[m] - cur[m])
        oc[m] += 1
    return out, oc


def _surface_pairs(v, a, r, h):
    """v [P,3,3] triangle vertices relative to the body's centre, a [P,3] unit axes: (S) per pair."""
    P = v.shape[0]
    if P == 0:
        return np.zeros(0, bool)
    hh = np.full(P, h)
    poly, cnt = v, np.full(P, 3)
    s = np.einsum("pkd,pd->pk", poly, a)
    poly, cnt = _clip(poly, cnt, s, hh)
    s = -np.einsum("pkd,pd->pk", poly, a)
    poly, cnt = _clip(poly, cnt, s, hh)
    # an orthonormal basis (u, w) of the plane perpendicular to a
    k = np.argmin(np.abs(a), 1)
    e = np.zeros_like(a)
    e[np.arange(P), k] = 1.0
    u = np.cross(a, e)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = np.cross(a, u)
    X, Y = np.einsum("pkd,pd->pk", poly, u), np.einsum("pkd,pd->pk", poly, w)
    K = poly.shape[1]
    ar = np.arange(P)
    best = np.full(P, np.inf)
    pos = np.ones(P, bool)
    neg = np.ones(P, bool)
    area = np.zeros(P)
    for i in range(K):
        valid = i < cnt
        j = np.where(i + 1 < cnt, i + 1, 0)
        px, py, qx, qy = X[:, i], Y[:, i], X[ar, j], Y[ar, j]
        dx, dy = qx - px, qy - py
        dd = dx * dx + dy * dy
        t = np.clip(np.where(dd > 0, -(px * dx + py * dy) / np.where(dd > 0, dd, 1.0), 0.0), 0.0, 1.0)
        ex, ey = px + t * dx, py + t * dy
        best = np.where(valid, np.minimum(best, ex * ex + ey * ey), best)
        cr = dx * (-py) - dy * (-px)  # edge x (origin - p)
        pos &= ~valid | (cr >= 0)
        neg &= ~valid | (cr <= 0)
        area += np.where(valid, px * qy - qx * py, 0.0)
    inside = (pos | neg) & (area != 0.0)
    return (cnt >= 1) & (inside | (best <= r * r))


def _solid_angles(v):
    """v [...,3,3] vertices relative to the query point -> solid angle per triangle (Van Oosterom & Strackee)."""
    A, B, C = v[..., 0, :], v[..., 1, :], v[..., 2, :]
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (A, B, C))
    num = np.einsum("...d,...d->...", A, np.cross(B, C))
    den = la * lb * lc + np.einsum("...d,...d->...", A, B) * lc + np.einsum("...d,...d->...", A, C) * lb + \
        np.einsum("...d,...d->...", B, C) * la
    return 2.0 * np.arctan2(num, den)


class CollisionOracle:
    """tris: one [T_e,3,3] array per env (fp32 values), ids: one [T_e] int array per env (object ids)."""

    def __init__(self, tris, ids):
        self.tris = [np.asarray(t, f32).astype(np.float64).reshape(-1, 3, 3) for t in tris]
        self.ids = [np.asarray(i).reshape(-1) for i in ids]
        self.objs = []
        for t, i in zip(self.tris, self.ids):
            objs = []
            for o in np.unique(i):
                tt = t[i == o]
                objs.append((tt, tt.reshape(-1, 3).min(0), tt.reshape(-1, 3).max(0)))
            self.objs.append(objs)
        allv = np.concatenate([t.reshape(-1, 3) for t in self.tris] + [np.zeros((1, 3))])
        self.extent = float(np.abs(allv).max()) + 1.0

    @staticmethod
    def from_mesh(mesh):
        return CollisionOracle(*zip(*[tuple(x.detach().cpu().numpy() for x in mesh.env_triangles(e)) for e in range(mesh.num_envs)]))

    def codes(self, env, poses, r, h, ground=False):
        """Contact codes [M] u8 of bodies (r, h in fp64) at poses [M, >= 6] (fp32 values) in envs env [M]."""
        env = np.asarray(env, np.int64).reshape(-1)
        poses = np.asarray(poses, f32)
        M = env.shape[0]
        c = poses[:, :3].astype(np.float64)
        a = axes(poses)
        ext = r * np.sqrt(np.maximum(0.0, 1.0 - a * a)) + h * np.abs(a)  # the body's AABB half-extents
        surf = np.zeros(M, bool)
        for e in np.unique(env):
            me = np.nonzero(env == e)[0]
            t = self.tris[e]
            if t.shape[0] == 0:
                continue
            tmin, tmax = t.min(1), t.max(1)
            lo, hi = c[me] - ext[me] - 1e-9, c[me] + ext[me] + 1e-9
            ov = ((tmax[None] >= lo[:, None]) & (tmin[None] <= hi[:, None])).all(-1)  # [Me, T]
            pm, pt = np.nonzero(ov)
            if pm.size == 0:
                continue
            m = me[pm]
            hitp = _surface_pairs(t[pt] - c[m][:, None, :], a[m], r, h)
            surf[m[hitp]] = True
        inside = np.zeros(M, bool)
        for e in np.unique(env):
            me = np.nonzero((env == e) & ~surf)[0]
            for tt, lo, hi in self.objs[e]:
                mm = me[((c[me] >= lo) & (c[me] <= hi)).all(-1) & ~inside[me]]
                if mm.size == 0:
                    continue
                w = _solid_angles(tt[None] - c[mm][:, None, None, :]).sum(1) / (4.0 * math.pi)
                inside[mm[np.abs(w) >= 0.5]] = True
        grd = np.zeros(M, bool)
        if ground:
            grd = c[:, 2] - ext[:, 2] <= 0.0
        fin = np.isfinite(poses[:, :6]).all(1)
        code = (surf.astype(np.uint8) * SURFACE) | (inside.astype(np.uint8) * INSIDE) | (grd.astype(np.uint8) * GROUND)
        return np.where(fin, code, 0).astype(np.uint8)

    def robust_codes(self, env, poses, radius, half_length, ground=False):
        """(codes at the kernel's fp32 radius / half-length, robust mask [M])."""
        r, h = float(f32(radius)), float(f32(half_length))
        d = 1e-9 * self.extent
        lo = self.codes(env, poses, r - d, max(h - d, 0.0) if h > 0 else h, ground)
        hi = self.codes(env, poses, r + d, h + d, ground)
        return self.codes(env, poses, r, h, ground), lo == hi


# ---------------------------------------------------------------------------
# hand cases with known answers: (name, triangles [T,3,3], ids [T], pose [6], radius, half_length, ground, expected code)
# ---------------------------------------------------------------------------
def _wall(x=0.0):
    """A 10 x 10 m square in the plane x = `x`, centred at (x, 0, 5)."""
    p = np.array([[x, -5, 0], [x, 5, 0], [x, 5, 10], [x, -5, 10]], f32)
    return np.stack([p[[0, 1, 2]], p[[0, 2, 3]]])


def _box(lo, hi):
    import torch
    from gennbv_amd.env.mesh_scene import box_triangles
    return box_triangles(torch.tensor([lo], dtype=torch.float32), torch.tensor([hi], dtype=torch.float32)).numpy()


def _sphere(centre, radius):
    from gennbv_amd.env.mesh_scene import sphere_triangles
    return sphere_triangles(centre, radius).numpy()


def hand_cases():
    R, H = 0.1, 0.02
    half_pi = float(f32(math.pi / 2))
    deg = lambda x: float(f32(math.radians(x)))  # noqa: E731
    z01 = float(f32(0.1))
    cases = []
    wall = _wall()
    ones = lambda t: np.ones(t.shape[0], np.int32)  # noqa: E731
    # disk face-on to the wall (axis along +x: pitch 90 deg), at distance h -+ 1e-4
    cases.append(("face_on_touch", wall, ones(wall), [H - 1e-4, 0, 5, 0, half_pi, 0], R, H, False, SURFACE))
    cases.append(("face_on_free", wall, ones(wall), [H + 1e-4, 0, 5, 0, half_pi, 0], R, H, False, 0))
    cases.append(("face_on_touch_back", wall, ones(wall), [-(H - 1e-4), 0, 5, 0, half_pi, 0], R, H, False, SURFACE))
    # edge-on (axis along z), at distance r -+ 1e-4
    cases.append(("edge_on_touch", wall, ones(wall), [R - 1e-4, 0, 5, 0, 0, 0], R, H, False, SURFACE))
    cases.append(("edge_on_free", wall, ones(wall), [R + 1e-4, 0, 5, 0, 0, 0], R, H, False, 0))
    # tilted 45 deg about y: extent along x = (r + h) / sqrt(2)
    e45 = (R + H) / math.sqrt(2.0)
    cases.append(("tilt45_touch", wall, ones(wall), [e45 - 1e-4, 0, 5, 0, deg(45), 0], R, H, False, SURFACE))
    cases.append(("tilt45_free", wall, ones(wall), [e45 + 1e-4, 0, 5, 0, deg(45), 0], R, H, False, 0))
    # yaw turns the tilted axis away from x: the extent along x grows back towards r
    cases.append(("tilt45_yaw90_free", wall, ones(wall), [R + 1e-4, 0, 5, 0, deg(45), half_pi], R, H, False, 0))
    cases.append(("tilt45_yaw90_touch", wall, ones(wall), [R - 1e-3, 0, 5, 0, deg(45), half_pi], R, H, False, SURFACE))
    # a small triangle entirely inside the cylinder
    small = np.array([[[0.03, 0.0, 5.0], [-0.02, 0.03, 5.005], [-0.02, -0.03, 4.995]]], f32)
    cases.append(("triangle_inside", small, ones(small), [0, 0, 5, 0, 0, 0], R, H, False, SURFACE))
    # a triangle whose interior (not its boundary) the axis pierces: a large triangle in the plane z = 5
    big = np.array([[[-3, -3, 5], [3, -3, 5], [0, 4, 5]]], f32)
    cases.append(("axis_pierces", big, ones(big), [0.2, 0.1, 5.01, 0, 0, 0], R, H, False, SURFACE))
    cases.append(("axis_misses_above", big, ones(big), [0.2, 0.1, 5.03, 0, 0, 0], R, H, False, 0))
    # a body inside a box, and inside a sphere mesh
    box = _box([-1, -1, 4], [1, 1, 6])
    cases.append(("inside_box", box, ones(box), [0.1, -0.2, 5.3, 0, deg(30), deg(60)], R, H, False, INSIDE))
    sph = _sphere((0.0, 0.0, 5.0), 1.0)
    cases.append(("inside_sphere", sph, ones(sph), [0.2, 0.1, 4.8, 0, deg(-45), 0], R, H, False, INSIDE))
    # inside the sphere's AABB but outside the sphere
    cases.append(("sphere_aabb_corner", sph, ones(sph), [0.8, 0.8, 5.8, 0, 0, 0], R, H, False, 0))
    # degenerate triangles: a segment through the body, a segment beside it, a point inside, a point outside
    seg = np.array([[[-1, 0, 5], [1, 0, 5], [1, 0, 5]]], f32)
    cases.append(("segment_through", seg, ones(seg), [0, 0.05, 5, 0, 0, 0], R, H, False, SURFACE))
    cases.append(("segment_beside", seg, ones(seg), [0, R + 1e-4, 5, 0, 0, 0], R, H, False, 0))
    pt = np.array([[[0.05, 0.05, 5.01]] * 3], f32)
    cases.append(("point_inside", pt, ones(pt), [0, 0, 5, 0, 0, 0], R, H, False, SURFACE))
    cases.append(("point_outside", pt, ones(pt), [0, 0, 4.95, 0, 0, 0], R, H, False, 0))
    # the ground at the lowest lattice z = fp32(0.1) with r = fp32(0.1)
    none = np.zeros((0, 3, 3), f32)
    nid = np.zeros(0, np.int32)
    cases.append(("ground_pitch60", none, nid, [0, 0, z01, 0, deg(60), 0], z01, H, True, 0))
    cases.append(("ground_pitch75", none, nid, [0, 0, z01, 0, deg(75), 0], z01, H, True, GROUND))
    cases.append(("ground_pitch90", none, nid, [0, 0, z01, 0, half_pi, 0], z01, H, True, GROUND))
    cases.append(("ground_pitch90_off", none, nid, [0, 0, z01, 0, half_pi, 0], z01, H, False, 0))
    cases.append(("ground_level", none, nid, [0, 0, z01, 0, 0, 0], z01, H, True, 0))
    return cases


def lowest_point(pose, r, h):
    """c_z - (r sqrt(1 - a_z^2) + h |a_z|) in fp64."""
    a = axes(np.asarray([pose], f32))[0]
    return float(f32(pose[2])) - (r * math.sqrt(max(0.0, 1.0 - a[2] * a[2])) + h * abs(a[2]))

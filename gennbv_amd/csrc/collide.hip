// collide.hip -- collision termination of closed-loop envs on MI355X: does the drone body meet its env's scene?
//
// Replaces collision_buf of the reference's check_termination (gennbv/env/env_train_gennbv.py:438-457, the contact forces on
// the cf2x body).  The body is a closed solid cylinder of radius r and half-length h centred at the pose's (x, y, z), axis
// a = R e_z with R = Rz(yaw) Ry(pitch) Rx(roll) (Isaac Gym's quat_from_euler_xyz, which set_state uses), a in fp64 from the fp32
// pose values.  Every object of an env (a MeshScene object id) is a closed solid: its triangles plus the points x of its
// closed AABB where |w(x)| >= 1/2, w = the generalized winding number of its triangles.  contact_out[e]:
//
//   bit 0 (S)  a triangle of env e meets the solid cylinder (a triangle entirely inside it included)
//   bit 1 (I)  (S) is false and the centre lies in the solid of some object of env e
//   bit 2 (G)  the ground is enabled and the body's lowest point c_z - (r sqrt(1 - a_z^2) + h |a_z|) is <= 0
//
//   k_collide_cylinder   one wave per env, kWavesPerBlock envs per workgroup:
//     1. (S) candidates: the body's AABB (half-extents e_k = r sqrt(1 - a_k^2) + h |a_k|, grown) -> the range of cells it
//        overlaps, clamped to the env's grid, and the wave's walk over those cells' triangle lists (scene_cells.h cell_range,
//        wave_any_listed_tri);
//     2. (S) exact test, fp64, per triangle: P = triangle n slab |(x - c).a| <= h meets the infinite cylinder iff the axis
//        line pierces P or P's boundary comes within r of the axis.  That boundary is the three edges clipped to the slab
//        and the triangle's chords on the two cap planes; the piercing test is the axis segment against the triangle
//        (Moller-Trumbore).  No per-lane arrays;
//     3. (I), only when (S) is false: lane j tests object j's closed AABB; the objects that contain the centre are walked in
//        order, w = sum of the triangles' solid angles (Van Oosterom-Strackee) / 4 pi with a fixed lane-to-triangle
//        assignment and a fixed-order wave reduction.  Without (S) every triangle is >= min(r, h) from the centre, so w is
//        well conditioned;
//     4. lane 0 stores the code: no atomics, deterministic.
#include <cmath>

#include "common.h"
#include "scene_cells.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr double kPi = 3.14159265358979323846;

// squared distance between the axis line (through the origin, unit direction a) and the segment p + u d, u in [u0, u1]
__device__ __forceinline__ double seg_axis_dist2(V3 p, V3 d, V3 a, double u0, double u1)
{
    const V3 pw = p - a * dot(p, a);  // the parts perpendicular to the axis
    const V3 dw = d - a * dot(d, a);
    const double dd = dot(dw, dw);
    const double u = fmin(fmax(dd > 0.0 ? -dot(pw, dw) / dd : u0, u0), u1);
    const V3 q = pw + dw * u;
    return dot(q, q);
}

// edge p -> p + d clipped to the slab |x.a| <= h (s0, s1: the endpoints' heights), then within r of the axis?
__device__ __forceinline__ bool edge_hits(V3 p, V3 d, double s0, double s1, V3 a, double h, double r2)
{
    double u0 = 0.0, u1 = 1.0;
    const double ds = s1 - s0;
    if (ds == 0.0) {
        if (fabs(s0) > h) return false;
    } else {
        const double ua = (-h - s0) / ds, ub = (h - s0) / ds;
        u0 = fmax(u0, fmin(ua, ub));
        u1 = fmin(u1, fmax(ua, ub));
        if (u0 > u1) return false;
    }
    return seg_axis_dist2(p, d, a, u0, u1) <= r2;
}

// where edge p -> q crosses the cap plane (t: the endpoints' signed heights above it); false if it does not
__device__ __forceinline__ bool plane_point(V3 p, V3 q, double tp, double tq, V3 &out)
{
    if (!((tp <= 0.0 && tq >= 0.0) || (tp >= 0.0 && tq <= 0.0)) || tp == tq) return false;
    out = p + (q - p) * (tp / (tp - tq));
    return true;
}

// the triangle's chord on the cap plane x.a = hc within r of the axis?  The crossing points are collinear and come in
// pairs (>= 2 or none; a vertex on the plane is found by both its edges): the union of the pair segments is the chord.
// An edge inside the plane gives no crossing of its own; the edge test covers it.
__device__ __forceinline__ bool chord_hits(V3 v0, V3 v1, V3 v2, double s0, double s1, double s2, double hc, V3 a, double r2)
{
    const double t0 = s0 - hc, t1 = s1 - hc, t2 = s2 - hc;
    V3 p01 = v0, p12 = v0, p20 = v0;
    const bool k01 = plane_point(v0, v1, t0, t1, p01);
    const bool k12 = plane_point(v1, v2, t1, t2, p12);
    const bool k20 = plane_point(v2, v0, t2, t0, p20);
    bool hit = false;
    if (k01 && k12) hit = hit || seg_axis_dist2(p01, p12 - p01, a, 0.0, 1.0) <= r2;
    if (k12 && k20) hit = hit || seg_axis_dist2(p12, p20 - p12, a, 0.0, 1.0) <= r2;
    if (k20 && k01) hit = hit || seg_axis_dist2(p20, p01 - p20, a, 0.0, 1.0) <= r2;
    return hit;
}

// closed triangle q (9 floats, world) vs the closed solid cylinder centred at c, unit axis a, radius^2 r2, half-length h
__device__ bool tri_cylinder(const float *q, V3 c, V3 a, double r2, double h)
{
    const V3 v0 = v3((double)q[0], (double)q[1], (double)q[2]) - c;
    const V3 v1 = v3((double)q[3], (double)q[4], (double)q[5]) - c;
    const V3 v2 = v3((double)q[6], (double)q[7], (double)q[8]) - c;
    const double s0 = dot(v0, a), s1 = dot(v1, a), s2 = dot(v2, a);
    if (fmin(s0, fmin(s1, s2)) > h || fmax(s0, fmax(s1, s2)) < -h) return false;  // outside the slab
    const V3 e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2;
    if (edge_hits(v0, e0, s0, s1, a, h, r2) || edge_hits(v1, e1, s1, s2, a, h, r2) || edge_hits(v2, e2, s2, s0, a, h, r2)) return true;
    if (chord_hits(v0, v1, v2, s0, s1, s2, h, a, r2) || chord_hits(v0, v1, v2, s0, s1, s2, -h, a, r2)) return true;
    // the axis segment (origin + t a, |t| <= h) pierces the triangle (a zero determinant: parallel or degenerate, the
    // boundary tests above decide)
    const V3 f2 = v2 - v0;
    const V3 pv = cross(a, f2);
    const double det = dot(e0, pv);
    if (det == 0.0) return false;
    const double inv = 1.0 / det;
    const V3 tv = v3(-v0.x, -v0.y, -v0.z);
    const double u = dot(tv, pv) * inv;
    const V3 qv = cross(tv, e0);
    const double v = dot(a, qv) * inv;
    const double t = dot(f2, qv) * inv;
    return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && fabs(t) <= h;
}

// solid angle of triangle q (9 floats) seen from c (Van Oosterom & Strackee 1983)
__device__ __forceinline__ double solid_angle(const float *q, V3 c)
{
    const V3 A = v3((double)q[0], (double)q[1], (double)q[2]) - c;
    const V3 B = v3((double)q[3], (double)q[4], (double)q[5]) - c;
    const V3 C = v3((double)q[6], (double)q[7], (double)q[8]) - c;
    const double la = sqrt(dot(A, A)), lb = sqrt(dot(B, B)), lc = sqrt(dot(C, C));
    const double num = dot(A, cross(B, C));
    const double den = la * lb * lc + dot(A, B) * lc + dot(A, C) * lb + dot(B, C) * la;
    return 2.0 * atan2(num, den);
}

// the contact code of env e's scene at pose p (one wave; the same value in every lane)
__device__ __forceinline__ uint8_t collide_code(const GnbvMeshScene &sc, const GnbvMeshObjects &ob, int e, const float *__restrict__ p,
                                                float radius, float half_length, int ground)
{
    const int lane = threadIdx.x & (kWave - 1);
    const V3 c = v3((double)p[0], (double)p[1], (double)p[2]);
    const double roll = (double)p[3], pitch = (double)p[4], yaw = (double)p[5];
    const double cr = cos(roll), sr = sin(roll), cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
    const V3 a = v3(cy * sp * cr + sy * sr, sy * sp * cr - cy * sr, cp * cr);  // R e_z, R = Rz(yaw) Ry(pitch) Rx(roll)
    const double r = (double)radius, h = (double)half_length, r2 = r * r;
    const double ex = r * sqrt(fmax(0.0, 1.0 - a.x * a.x)) + h * fabs(a.x);
    const double ey = r * sqrt(fmax(0.0, 1.0 - a.y * a.y)) + h * fabs(a.y);
    const double ez = r * sqrt(fmax(0.0, 1.0 - a.z * a.z)) + h * fabs(a.z);
    const bool finite = isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(a.x) && isfinite(a.y) && isfinite(a.z);

    // ---- (S): candidates from the cells the body's AABB overlaps
    bool s_hit = false;
    if (finite) {
        const double grow = 1e-12 * (fmax(fabs(c.x), fmax(fabs(c.y), fabs(c.z))) + r + h);  // rounding of a and of e_k
        const double blo[3] = {c.x - ex - grow, c.y - ey - grow, c.z - ez - grow};
        const double bhi[3] = {c.x + ex + grow, c.y + ey + grow, c.z + ez + grow};
        const EnvCells cells = load_env_cells(sc, e);
        CellRange range;
        if (cell_range(cells, blo, bhi, range))
            s_hit = wave_any_listed_tri(sc, cells, range, no_cells(),
                                        [&](const float *q) { return tri_aabb_meets(q, blo, bhi) && tri_cylinder(q, c, a, r2, h); });
    }

    // ---- (I): the centre inside an object's solid (only without (S))
    bool inside = false;
    if (finite && !s_hit) {
        const int o0 = ob.env_obj_start[e], o1 = ob.env_obj_start[e + 1];
        for (int k0 = o0; k0 < o1 && !inside; k0 += kWave) {
            const int k = k0 + lane;
            bool in_box = false;
            if (k < o1) {
                const float *bb = ob.obj_aabb + (size_t)k * 6;
                in_box = c.x >= (double)bb[0] && c.y >= (double)bb[1] && c.z >= (double)bb[2] && c.x <= (double)bb[3] &&
                         c.y <= (double)bb[4] && c.z <= (double)bb[5];
            }
            uint64_t m = __ballot(in_box);
            while (m != 0 && !inside) {
                const int obj = k0 + __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const int t0 = ob.obj_tri_start[obj], t1 = ob.obj_tri_start[obj + 1];
                double sum = 0.0;
                for (int t = t0 + lane; t < t1; t += kWave) sum += solid_angle(sc.tris + (size_t)ob.obj_tris[t] * 9, c);
                const double w = wave_sum_all(sum) / (4.0 * kPi);
                inside = fabs(w) >= 0.5;
            }
        }
    }

    // ---- (G): closed form
    const bool g_hit = finite && ground != 0 && c.z - ez <= 0.0;
    return (uint8_t)((s_hit ? 1 : 0) | (inside ? 2 : 0) | (g_hit ? 4 : 0));
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_collide_cylinder(GnbvMeshScene sc, GnbvMeshObjects ob,
                                                                              const float *__restrict__ poses, int64_t poses_row_stride,
                                                                              float radius, float half_length, int ground,
                                                                              uint8_t *__restrict__ contact_out)
{
    const int e = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x / kWave);
    if (e >= sc.n) return;  // whole wave
    const uint8_t code = collide_code(sc, ob, e, poses + (size_t)e * poses_row_stride, radius, half_length, ground);
    if ((threadIdx.x & (kWave - 1)) == 0) contact_out[e] = code;
}

// one wave per (env, candidate): item = e k + j, row item of poses
__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_collide_cylinder_batch(GnbvMeshScene sc, GnbvMeshObjects ob,
                                                                                    const float *__restrict__ poses, int k,
                                                                                    int64_t poses_row_stride, float radius,
                                                                                    float half_length, int ground,
                                                                                    uint8_t *__restrict__ contact_out)
{
    const int item = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x / kWave);
    if (item >= sc.n * k) return;  // whole wave
    const uint8_t code = collide_code(sc, ob, item / k, poses + (size_t)item * poses_row_stride, radius, half_length, ground);
    if ((threadIdx.x & (kWave - 1)) == 0) contact_out[item] = code;
}

}  // namespace

static bool collide_args_ok(const GnbvMeshScene *scene, const GnbvMeshObjects *objects, const float *poses, int64_t poses_row_stride,
                            float radius, float half_length, const uint8_t *contact_out)
{
    if (scene == nullptr || objects == nullptr || poses == nullptr || contact_out == nullptr) return false;
    const GnbvMeshScene &sc = *scene;
    const GnbvMeshObjects &ob = *objects;
    return scene_ok(sc) && ob.n == sc.n && ob.num_objects >= 0 && poses_row_stride >= 6 && std::isfinite(radius) && radius > 0.0f &&
           std::isfinite(half_length) && half_length >= 0.0f && ob.env_obj_start != nullptr && ob.obj_tri_start != nullptr &&
           // obj_aabb / obj_tris (and the scene's tris) may be NULL when no env has an object
           (ob.num_objects == 0 || (ob.obj_aabb != nullptr && ob.obj_tris != nullptr && sc.tris != nullptr));
}

GNBV_API int gnbv_collide_cylinder(const GnbvMeshScene *scene, const GnbvMeshObjects *objects, const float *poses, int64_t poses_row_stride,
                                   float radius, float half_length, int ground, uint8_t *contact_out, void *stream)
{
    GNBV_CHECK_ARG(collide_args_ok(scene, objects, poses, poses_row_stride, radius, half_length, contact_out));
    const GnbvMeshScene sc = *scene;
    const GnbvMeshObjects ob = *objects;
    const int blocks = (sc.n + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(k_collide_cylinder, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, gnbv_stream(stream), sc, ob, poses,
                       poses_row_stride, radius, half_length, ground, contact_out);
    return gnbv_launch_status();
}

GNBV_API int gnbv_collide_cylinder_batch(const GnbvMeshScene *scene, const GnbvMeshObjects *objects, const float *poses, int k,
                                         int64_t poses_row_stride, float radius, float half_length, int ground, uint8_t *contact_out,
                                         void *stream)
{
    GNBV_CHECK_ARG(collide_args_ok(scene, objects, poses, poses_row_stride, radius, half_length, contact_out));
    const GnbvMeshScene sc = *scene;
    const GnbvMeshObjects ob = *objects;
    GNBV_CHECK_ARG(k >= 1 && (int64_t)sc.n * k <= 0x7fffffff);
    const int blocks = (int)(((int64_t)sc.n * k + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(k_collide_cylinder_batch, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, gnbv_stream(stream), sc, ob, poses, k,
                       poses_row_stride, radius, half_length, ground, contact_out);
    return gnbv_launch_status();
}

// sweep.hip -- swept flight path on MI355X: does the drone, flown straight from one pose to the next, meet its env's scene?
//
// collide.hip tests the body where it stops; this file tests the way there.  Item (e, j) is the segment a -> b (the xyz of
// `from` and `to`, fp32 taken to fp64) and the swept solid is the sphere of radius R moved along it (a capsule): the body's
// orientation changes in flight, and the sphere that bounds the cylinder (R = sqrt(r^2 + h^2)) is the orientation-independent
// choice -- conservative: it never passes a path the cylinder could not fly.  contact_out[e, j]:
//
//   bit 3 (8,  PATH)         some closed triangle T of env e has dist(segment, T) <= R (a degenerate triangle counts as its
//                            segment or point; a zero-length segment is the sphere test)
//   bit 4 (16, PATH_GROUND)  the ground is enabled and min(a_z, b_z) - R <= 0
//
// There is no "inside" bit: a path whose start is free cannot enter a closed solid without coming within R of one of its
// triangles, and whether the start is free is collide.hip's question.
//
//   k_sweep_sphere   one wave per item, kWavesPerBlock items per workgroup; the work follows the segment, not its bounding box:
//     1. the segment is clipped to the env's cell grid grown by R (every triangle lies inside the grid), and the clipped part is
//        cut into pieces no longer than about the shortest cell edge (at most kMaxPieces: longer pieces list more cells, never
//        fewer);
//     2. per piece: the cell range of its R-grown AABB, minus the cells the previous piece's range held (along a straight
//        line the ranges move monotonically, so a cell is listed once per run of pieces), walked by the wave as collide_code
//        walks its range (scene_cells.h cell_range, wave_any_listed_tri).  A triangle listed in several cells is tested more
//        than once: the results are ORed;
//     3. per triangle, fp64: an AABB reject against the whole segment's R-grown box, then the exact predicate against the WHOLE
//        segment: dist = 0 if the segment pierces the triangle, else the minimum of the plane distance of either endpoint
//        whose projection falls inside the triangle and the three segment-edge distances (which hold every
//        endpoint-to-boundary distance);
//     4. the whole wave leaves at the first hit (__any); lane 0 stores the code, or ORs it into contact_out[e, j]
//        (`accumulate`; the item's own wave does the read-modify-write of its own byte): no atomics, deterministic.
#include <cmath>

#include "common.h"
#include "scene_cells.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kMaxPieces = 4096;

__device__ __forceinline__ double clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }

// squared distance between the segments p1 + s d1 and p2 + t d2, s, t in [0, 1] (either may have zero length)
__device__ __forceinline__ double seg_seg_dist2(V3 p1, V3 d1, V3 p2, V3 d2)
{
    const V3 r = p1 - p2;
    const double a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r);
    double s = 0.0, t = 0.0;
    if (a > 0.0 || e > 0.0) {
        if (!(a > 0.0)) {
            t = clamp01(f / e);
        } else {
            const double c = dot(d1, r);
            if (!(e > 0.0)) {
                s = clamp01(-c / a);
            } else {
                const double b = dot(d1, d2);
                const double den = a * e - b * b;
                s = den > 0.0 ? clamp01((b * f - c * e) / den) : 0.0;
                t = (b * s + f) / e;
                if (t < 0.0) {
                    t = 0.0;
                    s = clamp01(-c / a);
                } else if (t > 1.0) {
                    t = 1.0;
                    s = clamp01((b - c) / a);
                }
            }
        }
    }
    const V3 q = r + d1 * s - d2 * t;
    return dot(q, q);
}

// x (relative to v0) inside the closed triangle's prism: on the inner side of all three edge planes (n = e0 x f2, not zero)
__device__ __forceinline__ bool in_prism(V3 x, V3 e0, V3 f2, V3 n)
{
    const V3 e1 = f2 - e0;
    return dot(cross(e0, x), n) >= 0.0 && dot(cross(e1, x - e0), n) >= 0.0 && dot(cross(x - f2, f2), n) >= 0.0;
}

// closed triangle q (9 floats, world) within R (r2 = R^2) of the segment a -> a + d?
__device__ bool tri_capsule(const float *q, V3 a, V3 d, double r2)
{
    const V3 v0 = v3((double)q[0], (double)q[1], (double)q[2]);
    const V3 v1 = v3((double)q[3], (double)q[4], (double)q[5]);
    const V3 v2 = v3((double)q[6], (double)q[7], (double)q[8]);
    const V3 e0 = v1 - v0, e1 = v2 - v1, f2 = v2 - v0;
    if (seg_seg_dist2(a, d, v0, e0) <= r2 || seg_seg_dist2(a, d, v1, e1) <= r2 || seg_seg_dist2(a, d, v0, f2) <= r2) return true;
    const V3 n = cross(e0, f2);
    const double nn = dot(n, n);
    if (!(nn > 0.0)) return false;  // degenerate: its segment or point, which the edges are
    const V3 pa = a - v0, pb = pa + d;
    const double da = dot(pa, n), db = dot(pb, n);
    if (da * da <= r2 * nn && in_prism(pa, e0, f2, n)) return true;  // an endpoint above the face, within R of its plane
    if (db * db <= r2 * nn && in_prism(pb, e0, f2, n)) return true;
    if (((da <= 0.0 && db >= 0.0) || (da >= 0.0 && db <= 0.0)) && da != db)  // the segment pierces the face
        return in_prism(pa + d * (da / (da - db)), e0, f2, n);
    return false;
}

// the path code of the flight a -> b in env e (one wave; the same value in every lane)
__device__ __forceinline__ uint8_t sweep_code(const GnbvMeshScene &sc, int e, const float *__restrict__ pf, const float *__restrict__ pt,
                                              float radius, int ground)
{
    const V3 a = v3((double)pf[0], (double)pf[1], (double)pf[2]);
    const V3 b = v3((double)pt[0], (double)pt[1], (double)pt[2]);
    if (!(isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z))) return 0;
    const double R = (double)radius, r2 = R * R;
    const V3 d = b - a;
    const uint8_t g_bit = (ground != 0 && fmin(a.z, b.z) - R <= 0.0) ? 16 : 0;

    const EnvCells cells = load_env_cells(sc, e);
    if (cells.res[0] <= 0) return g_bit;  // an env without triangles
    const double av[3] = {a.x, a.y, a.z}, dv[3] = {d.x, d.y, d.z};
    const double amax = fmax(fmax(fabs(a.x), fabs(b.x)), fmax(fmax(fabs(a.y), fabs(b.y)), fmax(fabs(a.z), fabs(b.z))));
    const double grow = R + 1e-12 * (amax + R);  // R, and the rounding of the piece ends
    double blo[3], bhi[3];
    // ---- 1. the part s in [s0, s1] of the segment inside the grid grown by R
    double s0 = 0.0, s1 = 1.0, cmin = 0.0;
    bool any = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double clo = cells.lo[k], csz = cells.size[k];
        cmin = k == 0 ? csz : fmin(cmin, csz);
        blo[k] = fmin(av[k], av[k] + dv[k]) - grow;
        bhi[k] = fmax(av[k], av[k] + dv[k]) + grow;
        const double pad = grow + 1e-6 * csz;
        const double glo = clo - pad, ghi = clo + csz * (double)cells.res[k] + pad;
        if (dv[k] == 0.0) {
            any = any && av[k] >= glo && av[k] <= ghi;
        } else {
            const double u0 = (glo - av[k]) / dv[k], u1 = (ghi - av[k]) / dv[k];
            s0 = fmax(s0, fmin(u0, u1) - 1e-9);
            s1 = fmin(s1, fmax(u0, u1) + 1e-9);
        }
    }
    if (!any || s0 > s1) return g_bit;
    const double len = sqrt(dot(d, d)) * (s1 - s0);
    const int np = (int)fmin(fmax(ceil(len / cmin), 1.0), (double)kMaxPieces);

    // ---- 2./3. the pieces (np is wave-uniform)
    CellRange prev = no_cells();  // the previous piece's cell range
    for (int p = 0; p < np; ++p) {
        const double sa = s0 + (s1 - s0) * ((double)p / (double)np), sb = s0 + (s1 - s0) * ((double)(p + 1) / (double)np);
        double plo[3], phi[3];  // the piece's R-grown AABB
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double xa = av[k] + dv[k] * sa, xb = av[k] + dv[k] * sb;
            plo[k] = fmin(xa, xb) - grow;
            phi[k] = fmax(xa, xb) + grow;
        }
        CellRange range;
        if (!cell_range(cells, plo, phi, range)) {
            prev = no_cells();
            continue;
        }
        if (wave_any_listed_tri(sc, cells, range, prev,
                                [&](const float *q) { return tri_aabb_meets(q, blo, bhi) && tri_capsule(q, a, d, r2); }))
            return (uint8_t)(8 | g_bit);
        prev = range;
    }
    return g_bit;
}

// one wave per (env, item): item = e k + j
__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_sweep_sphere(GnbvMeshScene sc, const float *__restrict__ from,
                                                                          int64_t from_env_stride, int64_t from_item_stride,
                                                                          const float *__restrict__ to, int k, int64_t to_row_stride,
                                                                          float radius, int ground,
                                                                          const int64_t *__restrict__ episode_length, int accumulate,
                                                                          uint8_t *contact_out)
{
    const int item = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x / kWave);
    if (item >= sc.n * k) return;  // whole wave
    const int e = item / k, j = item - e * k;
    uint8_t code = 0;
    if (episode_length == nullptr || episode_length[e] > 1)  // the first pose of an episode is set, not flown to
        code = sweep_code(sc, e, from + (size_t)e * from_env_stride + (size_t)j * from_item_stride, to + (size_t)item * to_row_stride,
                          radius, ground);
    if ((threadIdx.x & (kWave - 1)) == 0) contact_out[item] = accumulate ? (uint8_t)(contact_out[item] | code) : code;
}

}  // namespace

GNBV_API int gnbv_sweep_sphere(const GnbvMeshScene *scene, const float *from, int64_t from_env_stride, int64_t from_item_stride,
                               const float *to, int k, int64_t to_row_stride, float radius, int ground, const int64_t *episode_length,
                               int accumulate, uint8_t *contact_out, void *stream)
{
    GNBV_CHECK_ARG(scene != nullptr && from != nullptr && to != nullptr && contact_out != nullptr);
    const GnbvMeshScene sc = *scene;
    GNBV_CHECK_ARG(scene_ok(sc));
    GNBV_CHECK_ARG(k >= 1 && (int64_t)sc.n * k <= 0x7fffffff);
    GNBV_CHECK_ARG(to_row_stride >= 3 && from_env_stride >= 3 && (from_item_stride == 0 || from_item_stride >= 3));
    GNBV_CHECK_ARG(std::isfinite(radius) && radius > 0.0f && (accumulate == 0 || accumulate == 1));
    const int blocks = (int)(((int64_t)sc.n * k + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(k_sweep_sphere, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, gnbv_stream(stream), sc, from, from_env_stride,
                       from_item_stride, to, k, to_row_stride, radius, ground, episode_length, accumulate, contact_out);
    return gnbv_launch_status();
}

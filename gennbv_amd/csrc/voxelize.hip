// voxelize.hip -- surface voxelization of a MeshScene on MI355X: the ground-truth grid of a closed-loop env.
//
// The reference loads a grid_gt.pt per scene that an offline tool made (gennbv/env/env_train_gennbv.py:21-96).  Here
// the grid is computed from the same triangles the renderer draws, under the updater's own voxel bounds
// (k_pose_to_idx in voxel.hip, gennbv/utils.py:230-270):
//
//   per axis a:  v = voxel_size[a],  vmin = fp32(range_min[a] - fp32(0.5 * v))
//   voxel i   =  the closed interval [vmin + i*v, vmin + (i+1)*v], evaluated in fp64 from those fp32 values
//   grid_out[e,x,y,z] = 1 iff the closed box of (x,y,z) meets a closed triangle of env e, else 0
//
//   k_voxelize_surface   one 512-lane workgroup per (env, 8^3 brick of voxels), one lane per voxel:
//     1. the brick's box -> the range of MeshScene cells it overlaps (the cell lists are a conservative superset:
//        a triangle that touches the brick is listed in one of them);
//     2. the lanes stride over those cells' entries and keep a triangle if its AABB meets the brick's box and this
//        is the first of the brick's cells that lists it (neighbour lookups in the sorted cell lists: no duplicates);
//        survivors go to an LDS list;
//     3. every lane runs the separating-axis triangle / box test (Akenine-Moller: 3 box normals, the triangle
//        normal, 9 edge cross products) for its voxel against the list, in fp64;
//     4. every lane stores its voxel, once: no atomics on global memory, no zero fill, deterministic.
//
// Conservative rounding: the box of the test is grown by delta = 2^-40 * (|coordinates| involved).  A separating
// axis found for the computed (rounded) axis vector is a proof of separation whatever the rounding of that vector, so
// only the evaluation of the projections can err, and it errs by < 2^-50 * |coordinates|: no false negative, and a
// false positive only within delta of the voxel, far below the 16 * 2^-23 * max|range| the contract allows.
#include "common.h"
#include "scene_cells.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kBrick = 8;
constexpr int kBlock = kBrick * kBrick * kBrick;  // one lane per voxel of the brick
constexpr int kCap = 2 * kBlock;                 // LDS candidates; flushed when one more chunk might not fit
constexpr int kTriStride = 10;                   // 9 vertex floats + max |coordinate|
constexpr double kGrow = 0x1p-40;                // box growth per unit of coordinate magnitude (header comment)

__device__ __forceinline__ double min3(double a, double b, double c) { return fmin(a, fmin(b, c)); }
__device__ __forceinline__ double max3(double a, double b, double c) { return fmax(a, fmax(b, c)); }

// the three vertices (relative to the box centre) project onto (ax, ay, az) outside the box's projection radius
__device__ __forceinline__ bool separated(double ax, double ay, double az, const double *v, double hx, double hy, double hz)
{
    const double p0 = ax * v[0] + ay * v[1] + az * v[2];
    const double p1 = ax * v[3] + ay * v[4] + az * v[5];
    const double p2 = ax * v[6] + ay * v[7] + az * v[8];
    const double r = hx * fabs(ax) + hy * fabs(ay) + hz * fabs(az);
    return min3(p0, p1, p2) > r || max3(p0, p1, p2) < -r;
}

// closed triangle q (9 floats) vs the closed box centre c, half extent h (already grown).  A zero-length edge or a
// zero normal gives a zero axis, which separates nothing: a degenerate triangle is tested as its segment or point.
__device__ bool tri_box_overlap(const float *q, double cx, double cy, double cz, double hx, double hy, double hz)
{
    double v[9];
    v[0] = (double)q[0] - cx; v[1] = (double)q[1] - cy; v[2] = (double)q[2] - cz;
    v[3] = (double)q[3] - cx; v[4] = (double)q[4] - cy; v[5] = (double)q[5] - cz;
    v[6] = (double)q[6] - cx; v[7] = (double)q[7] - cy; v[8] = (double)q[8] - cz;
    // box normals
    if (min3(v[0], v[3], v[6]) > hx || max3(v[0], v[3], v[6]) < -hx) return false;
    if (min3(v[1], v[4], v[7]) > hy || max3(v[1], v[4], v[7]) < -hy) return false;
    if (min3(v[2], v[5], v[8]) > hz || max3(v[2], v[5], v[8]) < -hz) return false;
    // edges e_j = v_{j+1} - v_j from the exact fp32 vertices (the differences round; see the header comment)
    const double e0x = (double)q[3] - (double)q[0], e0y = (double)q[4] - (double)q[1], e0z = (double)q[5] - (double)q[2];
    const double e1x = (double)q[6] - (double)q[3], e1y = (double)q[7] - (double)q[4], e1z = (double)q[8] - (double)q[5];
    const double e2x = (double)q[0] - (double)q[6], e2y = (double)q[1] - (double)q[7], e2z = (double)q[2] - (double)q[8];
    // triangle normal
    const double nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
    if (separated(nx, ny, nz, v, hx, hy, hz)) return false;
    // box axis x edge
    if (separated(0.0, -e0z, e0y, v, hx, hy, hz)) return false;
    if (separated(0.0, -e1z, e1y, v, hx, hy, hz)) return false;
    if (separated(0.0, -e2z, e2y, v, hx, hy, hz)) return false;
    if (separated(e0z, 0.0, -e0x, v, hx, hy, hz)) return false;
    if (separated(e1z, 0.0, -e1x, v, hx, hy, hz)) return false;
    if (separated(e2z, 0.0, -e2x, v, hx, hy, hz)) return false;
    if (separated(-e0y, e0x, 0.0, v, hx, hy, hz)) return false;
    if (separated(-e1y, e1x, 0.0, v, hx, hy, hz)) return false;
    if (separated(-e2y, e2x, 0.0, v, hx, hy, hz)) return false;
    return true;
}

// is triangle t in the sorted list of cell `cell`?
__device__ __forceinline__ bool cell_lists(const GnbvMeshScene &sc, int cell, int t)
{
    int lo = sc.cell_start[cell], hi = sc.cell_start[cell + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int x = sc.cell_tris[mid];
        if (x == t) return true;
        if (x < t) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// the voxel bounds of the updater (header comment): lower face of voxel i on one axis
__device__ __forceinline__ double voxel_face(float vmin, float v, int i) { return (double)vmin + (double)i * (double)v; }

__global__ __launch_bounds__(kBlock) void k_voxelize_surface(GnbvMeshScene sc, const float *__restrict__ range_gt,
                                                             const float *__restrict__ voxel_size, int g, int nb,
                                                             float *__restrict__ grid_out)
{
    __shared__ float s_tri[kCap * kTriStride];
    __shared__ int s_n;

    const int e = blockIdx.y;
    const int brick = blockIdx.x;
    const int tid = threadIdx.x;
    const int i0x = (brick / (nb * nb)) * kBrick, i0y = ((brick / nb) % nb) * kBrick, i0z = (brick % nb) * kBrick;
    const int x = i0x + (tid >> 6), y = i0y + ((tid >> 3) & 7), z = i0z + (tid & 7);
    const bool active = x < g && y < g && z < g;
    const size_t out = (((size_t)e * g + x) * g + y) * g + z;

    float vs[3], vmin[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        vs[a] = voxel_size[e * 3 + a];
        vmin[a] = __fsub_rn(range_gt[e * 6 + 2 * a + 1], __fmul_rn(0.5f, vs[a]));
        ok = ok && vs[a] > 0.f && isfinite(vs[a]) && isfinite(vmin[a]) && isfinite(vmin[a] + (float)g * vs[a]);
    }
    if (!ok) {  // not a grid (the host cannot check device values without a sync): mark the whole env, loudly
        if (active) grid_out[out] = __builtin_nanf("");
        return;
    }

    // the brick's box [blo, bhi] (voxel_face of its first and one past its last voxel: the same numbers as the voxels')
    const double blo[3] = {voxel_face(vmin[0], vs[0], i0x), voxel_face(vmin[1], vs[1], i0y), voxel_face(vmin[2], vs[2], i0z)};
    const double bhi[3] = {voxel_face(vmin[0], vs[0], min(i0x + kBrick, g)), voxel_face(vmin[1], vs[1], min(i0y + kBrick, g)),
                           voxel_face(vmin[2], vs[2], min(i0z + kBrick, g))};
    const double bmag = fmax(fmax(fmax(fabs(blo[0]), fabs(bhi[0])), fmax(fabs(blo[1]), fabs(bhi[1]))), fmax(fabs(blo[2]), fabs(bhi[2])));

    // this lane's voxel: centre and half extent
    const double lx = voxel_face(vmin[0], vs[0], x), hx_ = voxel_face(vmin[0], vs[0], x + 1);
    const double ly = voxel_face(vmin[1], vs[1], y), hy_ = voxel_face(vmin[1], vs[1], y + 1);
    const double lz = voxel_face(vmin[2], vs[2], z), hz_ = voxel_face(vmin[2], vs[2], z + 1);
    const double cx = 0.5 * (lx + hx_), cy = 0.5 * (ly + hy_), cz = 0.5 * (lz + hz_);
    const double hx = 0.5 * (hx_ - lx), hy = 0.5 * (hy_ - ly), hz = 0.5 * (hz_ - lz);
    const double cmag = fmax(fmax(fabs(cx), fabs(cy)), fabs(cz)) + fmax(fmax(hx, hy), hz);
    bool hit = false;

    // the brick's range of mesh cells: scene_cells.h cell_range, kept in this kernel's own one-sided form (equal when `any`
    // holds).  The shared form measured 0.5 % slower on box scenes, where most workgroups run little but this prologue.
    const int rx = sc.cell_res[e * 3 + 0], ry = sc.cell_res[e * 3 + 1], rz = sc.cell_res[e * 3 + 2];
    const int res[3] = {rx, ry, rz};
    int c0[3], c1[3];
    bool any = rx > 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double clo = (double)sc.cell_lo[e * 3 + a], csz = (double)sc.cell_size[e * 3 + a];
        const double f0 = floor((blo[a] - clo) / csz - 1e-6), f1 = floor((bhi[a] - clo) / csz + 1e-6);
        any = any && f1 >= 0.0 && f0 <= (double)(res[a] - 1);
        c0[a] = (int)fmax(f0, 0.0);
        c1[a] = (int)fmin(f1, (double)(res[a] - 1));
    }

    if (tid == 0) s_n = 0;
    __syncthreads();
    if (any) {
        const int base = sc.cell_base[e];
        for (int kz = c0[2]; kz <= c1[2]; ++kz)
            for (int ky = c0[1]; ky <= c1[1]; ++ky)
                for (int kx = c0[0]; kx <= c1[0]; ++kx) {
                    const int cell = base + kx + rx * (ky + ry * kz);
                    const int b = sc.cell_start[cell], end = sc.cell_start[cell + 1];
                    for (int k0 = b; k0 < end; k0 += kBlock) {
                        // ---- gather: brick-level AABB rejection and first-listing-cell dedup
                        const int k = k0 + tid;
                        if (k < end) {
                            const int t = sc.cell_tris[k];
                            const float *q = sc.tris + (size_t)t * 9;
                            float qv[9];
#pragma unroll
                            for (int j = 0; j < 9; ++j) qv[j] = q[j];
                            float m = 0.f;
#pragma unroll
                            for (int j = 0; j < 9; ++j) m = fmaxf(m, fabsf(qv[j]));
                            const double grow = 4.0 * kGrow * ((double)m + bmag);  // >= every voxel's growth below
                            bool keep = true;
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                const double tmin = fmin(fmin((double)qv[a], (double)qv[3 + a]), (double)qv[6 + a]);
                                const double tmax = fmax(fmax((double)qv[a], (double)qv[3 + a]), (double)qv[6 + a]);
                                keep = keep && tmax >= blo[a] - grow && tmin <= bhi[a] + grow;
                            }
                            // a triangle lists in a box of cells: keep it in the lowest of them inside the brick's range
                            keep = keep && !(kx > c0[0] && cell_lists(sc, cell - 1, t));
                            keep = keep && !(ky > c0[1] && cell_lists(sc, cell - rx, t));
                            keep = keep && !(kz > c0[2] && cell_lists(sc, cell - rx * ry, t));
                            if (keep) {
                                const int slot = atomicAdd(&s_n, 1);  // LDS; the order of the list does not change the OR
                                float *d = s_tri + slot * kTriStride;
#pragma unroll
                                for (int j = 0; j < 9; ++j) d[j] = qv[j];
                                d[9] = m;
                            }
                        }
                        __syncthreads();
                        const int n = s_n;
                        __syncthreads();  // every lane has read n before the next chunk appends to s_n
                        if (n > kCap - kBlock) {  // ---- flush: the next chunk might not fit
                            for (int i = 0; i < n && active && !hit; ++i) {
                                const float *d = s_tri + i * kTriStride;
                                const double grow = kGrow * ((double)d[9] + cmag);
                                hit = tri_box_overlap(d, cx, cy, cz, hx + grow, hy + grow, hz + grow);
                            }
                            __syncthreads();
                            if (tid == 0) s_n = 0;
                            __syncthreads();
                        }
                    }
                }
    }
    const int n = s_n;  // (every lane passed a barrier since the last write of s_n)
    for (int i = 0; i < n && active && !hit; ++i) {
        const float *d = s_tri + i * kTriStride;
        const double grow = kGrow * ((double)d[9] + cmag);
        hit = tri_box_overlap(d, cx, cy, cz, hx + grow, hy + grow, hz + grow);
    }
    if (active) grid_out[out] = hit ? 1.0f : 0.0f;
}

}  // namespace

GNBV_API int gnbv_voxelize_surface(const GnbvMeshScene *scene, const float *range_gt, const float *voxel_size, int g,
                                   float *grid_out, void *stream)
{
    GNBV_CHECK_ARG(scene != nullptr && range_gt != nullptr && voxel_size != nullptr && grid_out != nullptr);
    const GnbvMeshScene sc = *scene;
    GNBV_CHECK_ARG(scene_ok(sc) && sc.n <= 65535 && g > 1 && g <= 1024);
    const int nb = (g + kBrick - 1) / kBrick;
    dim3 grid(nb * nb * nb, sc.n);
    hipLaunchKernelGGL(k_voxelize_surface, grid, dim3(kBlock), 0, gnbv_stream(stream), sc, range_gt, voxel_size, g, nb, grid_out);
    return gnbv_launch_status();
}

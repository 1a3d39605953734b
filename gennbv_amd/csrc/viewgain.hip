// viewgain.hip -- view gain of candidate camera poses against the tri-class grid an env holds now, on MI355X.
//
// "How much would the map change if the camera went to pose p?"  For env e, candidate j (DESIGN.md "View gain and baseline
// policies"; include/gennbv_hip.h gnbv_view_gain has the exact definition): the rays of the pixel lattice u = s/2 + i s,
// v = s/2 + j s end at the world point the voxel update would compute for that pixel at depth `range` (pixel_to_world of
// backproject.h, the canonical fp32 chain); source and target voxel are the unclamped pose_to_idx; each ray visits the in-grid
// voxels of the reference's integer Bresenham (voxel.hip bresenham_walk) in order and stops in front of the first occupied one.
// Three int32 per candidate: DISTINCT unknown voxels visited by any ray, the same over the rays that were stopped, stopped rays.
//
//   k_view_gain   workgroup (env, chunk of candidates):
//     1. the env's grid is packed to 2 bits per voxel into LDS once (unknown 0, occupied 1, free 3: 64 KiB at 64^3) and
//        serves every candidate of the chunk;
//     2. per candidate: 16 lanes build the camera matrices of the next 16 candidates (k_render_camera's arithmetic: fp64
//        trig rounded to fp32, roll ignored); one ray per lane, sequential integer walk.  The walk does not start at the
//        source: the range of steps i in [0, da] whose voxel lies in the grid comes from the closed form of the Bresenham
//        minors, nb(i) = floor((2 db i + da) / (2 da)) (exact on the dominant axis, widened by one step on the minors and
//        guarded by a bounds test in the loop), so a target 1 000 voxels away costs at most G steps;
//     3. distinct counts from two visited bitmasks in LDS (all rays / stopped rays, 32 KiB each at 64^3): atomicOr returns
//        the old word and the lane counts the bits it was first to set.  Only unknown voxels are marked.  A ray marks mask
//        A on its way; a stopped ray walks again into mask B;
//     4. wave reductions -> per-wave partials in LDS -> lane 0 sums them in wave order and stores the three integers.  No
//        global atomics, every output is written once by one lane: deterministic;
//     5. the workgroup clears both masks (16-byte stores) before the next candidate.
#include <cmath>

#include "common.h"
#include "backproject.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kMaxThreads = 1024;
constexpr int kMaxGrid = 64;          // LDS: G^3 / 4 (grid) + 2 * G^3 / 8 (masks) bytes = 128 KiB at 64^3
constexpr int kCamBatch = 16;         // camera matrices built at a time
constexpr float kCoordClamp = 16777216.0f;  // voxel coordinates saturate at +-2^24: the 64-bit closed form stays exact

struct VgParams {
    int n, k, g, chunk, chunks;
    const int8_t *tri;
    int64_t tri_row_stride;
    int tri_aligned;
    const float *poses, *range_gt, *voxel_size;
    Intrinsics kinv;
    int h, w, stride, nu, nrays;
    float range;
    int32_t *gain;
    float *c2w_out;
    int grid_words, mask_words, ablate;
};

// unclamped pose_to_idx of one axis (k_pose_to_idx): floor((p - (range_min - 0.5 v)) / v), IEEE division
__device__ __forceinline__ int axis_to_idx(float p, float range_min, float v)
{
    const float vmin = __fsub_rn(range_min, __fmul_rn(0.5f, v));
    const float fl = floorf(__fdiv_rn(__fsub_rn(p, vmin), v));
    if (!(fl == fl)) return 0;
    return (int)fminf(fmaxf(fl, -kCoordClamp), kCoordClamp);
}

// floor(num / den), den > 0, |num| < 2^52: fp64 quotient + remainder fix-up
__device__ __forceinline__ long long floor_div(long long num, long long den)
{
    long long q = (long long)floor((double)num / (double)den);
    const long long r = num - q * den;
    if (r < 0) --q;
    else if (r >= den) ++q;
    return q;
}

// steps [lo, hi] of a minor axis (start p0, direction s, extent d; the dominant extent is da > 0) whose coordinate
// p0 + s nb(i) may lie in [0, g): one step wider than the exact range on both sides
__device__ __forceinline__ void minor_range(int p0, int s, int d, int da, int g, long long &lo, long long &hi)
{
    const long long mlo = s > 0 ? -(long long)p0 : (long long)p0 - (g - 1);  // nb(i) must reach mlo ...
    const long long mhi = s > 0 ? (long long)(g - 1) - p0 : (long long)p0;    // ... and not pass mhi
    if (mhi < 0 || (mlo > 0 && d == 0)) {
        hi = -1;
        return;
    }
    if (d == 0) return;
    // first i with nb(i) >= m (m >= 1): ceil((2 da m - da) / (2 d))
    if (mlo > 0) lo = max(lo, floor_div(2LL * da * mlo - da + 2LL * d - 1, 2LL * d) - 1);
    hi = min(hi, floor_div(2LL * da * (mhi + 1) - da + 2LL * d - 1, 2LL * d));
}

struct RayWalk {  // the walk of one ray restricted to the steps [ilo, ihi]
    int n;        // steps to take (0: the ray never meets the grid)
    int pb, pc, p1, p2, lin;
    int sb, sc, two_da, two_db, two_dc, la, lb, lc;  // la, lb, lc: signed linear-index strides of the three axes
};

__device__ __forceinline__ RayWalk make_walk(int x0, int y0, int z0, int x1, int y1, int z1, int g)
{
    RayWalk r;
    r.n = 0;
    const int dx = abs(x1 - x0), dy = abs(y1 - y0), dz = abs(z1 - z0);
    const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1, sz = z0 < z1 ? 1 : -1;
    const int dm = max(max(dx, dy), dz);
    // dominant axis a, minors (b, c) in the reference's order (voxel.hip bresenham_walk); st*: linear stride of the axis
    int pa, pb, pc, da, db, dc, sa, sb, sc, sta, stb, stc;
    const int gg = g * g;
    if (dm == dx)      { pa = x0; pb = y0; pc = z0; da = dx; db = dy; dc = dz; sa = sx; sb = sy; sc = sz; sta = gg; stb = g; stc = 1; }
    else if (dm == dy) { pa = y0; pb = x0; pc = z0; da = dy; db = dx; dc = dz; sa = sy; sb = sx; sc = sz; sta = g; stb = gg; stc = 1; }
    else               { pa = z0; pb = x0; pc = y0; da = dz; db = dx; dc = dy; sa = sz; sb = sx; sc = sy; sta = 1; stb = gg; stc = g; }
    // dominant axis: pa + sa i in [0, g), i in [0, da] -- exact
    long long lo = sa > 0 ? -(long long)pa : (long long)pa - (g - 1);
    long long hi = sa > 0 ? (long long)(g - 1) - pa : (long long)pa;
    lo = max(lo, 0LL);
    hi = min(hi, (long long)da);
    if (da > 0) {
        minor_range(pb, sb, db, da, g, lo, hi);
        if (hi >= lo) minor_range(pc, sc, dc, da, g, lo, hi);
    }
    if (hi < lo) return r;
    long long nb = 0, nc = 0;
    if (da > 0 && lo > 0) {
        nb = floor_div(2LL * db * lo + da, 2LL * da);
        nc = floor_div(2LL * dc * lo + da, 2LL * da);
    }
    r.n = (int)(hi - lo + 1);  // <= g + 2
    pa += sa * (int)lo;
    r.pb = pb + sb * (int)nb;
    r.pc = pc + sc * (int)nc;
    // the decision variables in front of step lo -> lo + 1
    r.p1 = (int)(2LL * db * (lo + 1) - da - 2LL * da * nb);
    r.p2 = (int)(2LL * dc * (lo + 1) - da - 2LL * da * nc);
    r.lin = pa * sta + r.pb * stb + r.pc * stc;
    r.sb = sb; r.sc = sc;
    r.two_da = 2 * da; r.two_db = 2 * db; r.two_dc = 2 * dc;
    r.la = sa * sta; r.lb = sb * stb; r.lc = sc * stc;
    return r;
}

// visit(lin) for every in-grid voxel of the walk, in order; visit returns true to stop.  Returns whether it stopped.
template <typename Visit>
__device__ __forceinline__ bool run_walk(RayWalk r, int g, Visit &&visit)
{
    const unsigned ug = (unsigned)g;
    for (int i = 0; i < r.n; ++i) {
        if ((unsigned)r.pb < ug && (unsigned)r.pc < ug) {
            if (visit(r.lin)) return true;
        }
        if (r.p1 >= 0) { r.pb += r.sb; r.lin += r.lb; r.p1 -= r.two_da; }
        if (r.p2 >= 0) { r.pc += r.sc; r.lin += r.lc; r.p2 -= r.two_da; }
        r.lin += r.la;
        r.p1 += r.two_db;
        r.p2 += r.two_dc;
    }
    return false;
}

__device__ __forceinline__ uint32_t pack_codes4(uint32_t bytes4)
{
    uint32_t code = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int t = (int)(int8_t)(bytes4 >> (8 * b));
        code |= (t > 0 ? 1u : (t < 0 ? 3u : 0u)) << (2 * b);
    }
    return code;
}

__global__ __launch_bounds__(kMaxThreads) void k_view_gain(VgParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    __shared__ float s_cam[kCamBatch][16];
    __shared__ int s_src[kCamBatch][3];
    __shared__ int s_part[kMaxThreads / kWave][3];

    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int e = blockIdx.x / p.chunks, ch = blockIdx.x - e * p.chunks;
    const int j0 = ch * p.chunk, j1 = min(p.k, j0 + p.chunk);
    const int g = p.g, g3 = g * g * g;
    uint32_t *s_grid = s_mem, *s_a = s_mem + p.grid_words, *s_b = s_a + p.mask_words;

    // ---- 1. the env's grid, 2 bits per voxel
    const int8_t *row = p.tri + (size_t)e * p.tri_row_stride;
    for (int w = tid; w < p.grid_words; w += nthreads) {
        const int base = w * 16;
        uint32_t code = 0;
        if (p.tri_aligned && base + 16 <= g3) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + base);
            code = pack_codes4(v.x) | (pack_codes4(v.y) << 8) | (pack_codes4(v.z) << 16) | (pack_codes4(v.w) << 24);
        } else {
            for (int b = 0; b < 16 && base + b < g3; ++b) {
                const int t = (int)row[base + b];
                code |= (t > 0 ? 1u : (t < 0 ? 3u : 0u)) << (2 * b);
            }
        }
        s_grid[w] = code;
    }
    uint4 *s_masks4 = reinterpret_cast<uint4 *>(s_a);
    const int mask_quads = p.mask_words / 2;  // both masks, 4 words at a time (mask_words is a multiple of 4)
    for (int w = tid; w < mask_quads; w += nthreads) s_masks4[w] = make_uint4(0u, 0u, 0u, 0u);

    const float rmin_x = p.range_gt[e * 6 + 1], rmin_y = p.range_gt[e * 6 + 3], rmin_z = p.range_gt[e * 6 + 5];
    const float vx = p.voxel_size[e * 3 + 0], vy = p.voxel_size[e * 3 + 1], vz = p.voxel_size[e * 3 + 2];
    const bool mark = (p.ablate & 1) == 0, second = (p.ablate & 2) == 0;

    for (int j = j0; j < j1; ++j) {
        const int slot = (j - j0) % kCamBatch;
        if (slot == 0) {
            // ---- 2a. cameras of the next kCamBatch candidates (k_render_camera's arithmetic; -ffp-contract=off)
            if (tid < kCamBatch && j + tid < j1) {
                const float *q = p.poses + ((size_t)e * p.k + j + tid) * 6;
                const double pitch = (double)q[4], yaw = (double)q[5];
                const double cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
                const double fx = cp * cy, fy = cp * sy, fz = -sp;
                const double rx = sy, ry = -cy, rz = 0.0;
                const double dx = fy * rz - fz * ry, dy = fz * rx - fx * rz, dz = fx * ry - fy * rx;
                float *m = s_cam[tid];
                m[0] = (float)rx; m[1] = (float)dx; m[2] = (float)fx; m[3] = q[0];
                m[4] = (float)ry; m[5] = (float)dy; m[6] = (float)fy; m[7] = q[1];
                m[8] = (float)rz; m[9] = (float)dz; m[10] = (float)fz; m[11] = q[2];
                m[12] = 0.f; m[13] = 0.f; m[14] = 0.f; m[15] = 1.f;
                if (p.c2w_out != nullptr) {
                    float *o = p.c2w_out + ((size_t)e * p.k + j + tid) * 16;
#pragma unroll
                    for (int i = 0; i < 16; ++i) o[i] = m[i];
                }
                s_src[tid][0] = axis_to_idx(q[0], rmin_x, vx);
                s_src[tid][1] = axis_to_idx(q[1], rmin_y, vy);
                s_src[tid][2] = axis_to_idx(q[2], rmin_z, vz);
            }
        }
        __syncthreads();  // cameras ready; masks clear

        // ---- 2b / 3. one ray per lane
        const float *M = s_cam[slot];
        const int x0 = s_src[slot][0], y0 = s_src[slot][1], z0 = s_src[slot][2];
        int n_unknown = 0, n_unknown_hit = 0, n_blocked = 0;
        for (int r = tid; r < p.nrays; r += nthreads) {
            const int iv = r / p.nu, iu = r - iv * p.nu;
            const int u = p.stride / 2 + iu * p.stride, v = p.stride / 2 + iv * p.stride;
            float wp[3];
            pixel_to_world(p.range, (float)u, (float)v, p.kinv, M, wp);
            const int x1 = axis_to_idx(wp[0], rmin_x, vx), y1 = axis_to_idx(wp[1], rmin_y, vy), z1 = axis_to_idx(wp[2], rmin_z, vz);
            const RayWalk rw = make_walk(x0, y0, z0, x1, y1, z1, g);
            if (rw.n == 0) continue;
            const bool blocked = run_walk(rw, g, [&](int lin) {
                const uint32_t cls = (s_grid[lin >> 4] >> ((lin & 15) * 2)) & 3u;
                if (cls == 1u) return true;
                if (cls == 0u && mark) {
                    const uint32_t bit = 1u << (lin & 31);
                    n_unknown += (atomicOr(&s_a[lin >> 5], bit) & bit) == 0u;
                }
                return false;
            });
            if (blocked) {
                ++n_blocked;
                if (mark && second)
                    run_walk(rw, g, [&](int lin) {
                        const uint32_t cls = (s_grid[lin >> 4] >> ((lin & 15) * 2)) & 3u;
                        if (cls == 1u) return true;
                        if (cls == 0u) {
                            const uint32_t bit = 1u << (lin & 31);
                            n_unknown_hit += (atomicOr(&s_b[lin >> 5], bit) & bit) == 0u;
                        }
                        return false;
                    });
            }
        }

        // ---- 4. the three sums, in wave order
        n_unknown = wave_reduce_sum(n_unknown);
        n_unknown_hit = wave_reduce_sum(n_unknown_hit);
        n_blocked = wave_reduce_sum(n_blocked);
        if ((tid & (kWave - 1)) == 0) {
            s_part[tid / kWave][0] = n_unknown;
            s_part[tid / kWave][1] = n_unknown_hit;
            s_part[tid / kWave][2] = n_blocked;
        }
        __syncthreads();  // every ray of candidate j is done: partials complete, masks and camera slot free
        if (tid == 0) {
            int a = 0, b = 0, c = 0;
            for (int w = 0; w < nthreads / kWave; ++w) {
                a += s_part[w][0];
                b += s_part[w][1];
                c += s_part[w][2];
            }
            int32_t *o = p.gain + ((size_t)e * p.k + j) * 3;
            o[0] = a; o[1] = b; o[2] = c;
        }
        // ---- 5. clear the masks for the next candidate (ordered in front of its rays by the barrier at the loop's head;
        //         lane 0 reads s_part before it arrives there, the waves write it after)
        if (j + 1 < j1 && mark)
            for (int w = tid; w < mask_quads; w += nthreads) s_masks4[w] = make_uint4(0u, 0u, 0u, 0u);
    }
}

}  // namespace

GNBV_API int gnbv_view_gain(const GnbvViewGain *args, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvViewGain a = *args;
    GNBV_CHECK_ARG(a.n > 0 && a.k > 0 && a.g >= 2 && a.g <= kMaxGrid && a.h > 0 && a.w > 0 && a.stride >= 1);
    GNBV_CHECK_ARG(a.h <= 32768 && a.w <= 32768);
    GNBV_CHECK_ARG(std::isfinite(a.range) && a.range > 0.0f && a.chunk >= 0 && a.ablate >= 0 && a.ablate <= 3);
    GNBV_CHECK_ARG(a.tri_i8 != nullptr && a.poses != nullptr && a.range_gt != nullptr && a.voxel_size != nullptr);
    GNBV_CHECK_ARG(a.inv_intri != nullptr && a.gain != nullptr);
    const int g3 = a.g * a.g * a.g;
    GNBV_CHECK_ARG(a.tri_row_stride >= g3);
    VgParams p;
    p.n = a.n; p.k = a.k; p.g = a.g;
    // candidates per workgroup: enough workgroups for two per compute unit, but the grid is packed once per workgroup
    int chunk = a.chunk;
    if (chunk == 0) {
        const int want = (512 + a.n - 1) / a.n;  // chunks per env
        chunk = (a.k + want - 1) / want;
    }
    chunk = chunk < 1 ? 1 : (chunk > a.k ? a.k : chunk);
    p.chunk = chunk;
    p.chunks = (a.k + chunk - 1) / chunk;
    GNBV_CHECK_ARG((int64_t)a.n * p.chunks <= 0x7fffffff);
    p.tri = a.tri_i8;
    p.tri_row_stride = a.tri_row_stride;
    p.tri_aligned = (((uintptr_t)a.tri_i8 | (uintptr_t)a.tri_row_stride) & 15) == 0;
    p.poses = a.poses; p.range_gt = a.range_gt; p.voxel_size = a.voxel_size;
    for (int i = 0; i < 9; ++i) p.kinv.k[i] = a.inv_intri[i];
    p.h = a.h; p.w = a.w; p.stride = a.stride;
    const int half = a.stride / 2;
    p.nu = half < a.w ? (a.w - half + a.stride - 1) / a.stride : 0;
    const int nv = half < a.h ? (a.h - half + a.stride - 1) / a.stride : 0;
    p.nrays = p.nu * nv;
    p.range = a.range;
    p.gain = a.gain;
    p.c2w_out = a.c2w_out;
    p.grid_words = (((g3 + 15) / 16) + 3) & ~3;
    p.mask_words = (((g3 + 31) / 32) + 3) & ~3;
    p.ablate = a.ablate;
    const size_t lds = (size_t)(p.grid_words + 2 * p.mask_words) * sizeof(uint32_t);
    // one ray per lane; a workgroup whose LDS leaves room for several per compute unit stays at 256 lanes
    int threads = ((p.nrays > 0 ? p.nrays : 1) + kWave - 1) / kWave * kWave;
    const int cap = lds > 32 * 1024 ? kMaxThreads : 256;
    threads = threads > cap ? cap : threads;
    // (per call: the attribute belongs to the current device's copy of the kernel)
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)k_view_gain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return (int)hipGetLastError();
    hipLaunchKernelGGL(k_view_gain, dim3((unsigned)(a.n * p.chunks)), dim3(threads), lds, gnbv_stream(stream), p);
    return gnbv_launch_status();
}

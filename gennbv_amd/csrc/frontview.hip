// frontview.hip -- frontier viewpoints (gnbv_frontier_viewpoints): for T target voxels per env, which node of the flight lattice has
// a clear line of sight to the target on the scanned map, and which of those is cheapest to fly to.  The classical nearest-frontier
// question, joined from pieces that exist: the route costs of the belief field (flight.hip: field [N, M] u32), the voxel frame of
// gnbv_flight_blocked_tri, the ray rule of the view gain (ray_walk.h: unclamped pose_to_idx source, the in-grid voxels of the
// reference's Bresenham).  include/gennbv_hip.h has the exact definition; integers and fp64 in a stated order, tests compare ==.
//
//   k_frontview<kLds, kF32>   workgroup (env, chunk of the env's T targets), 512 lanes.
//     1. kLds (mode 1): the env's grid goes into two LDS bit planes, occupied and unknown (map_bits.h: map_pack_planes, coalesced
//        reads of either grid form, the bank swizzle), once per workgroup, and serves every target of the chunk.  !kLds (mode 2):
//        the voxels are read in place.
//     2. per target: the index window of the lattice that |p_a - q_a| <= r_max admits (padded: the header has the rule; clamped in
//        fp64 before conversion, so the loops are bounded by the lattice whatever the device arrays hold), one node per lane and
//        turn, i fastest -- consecutive lanes read consecutive field words.  The distance test comes first, the field word is
//        loaded next (it is in flight during the walk), then the walk: make_walk enters the grid by the closed form, so a node far
//        outside costs at most G steps; the line ends at the target, which is in the grid, so the last in-grid step is the target
//        itself and is dropped: its class is not looked at.  The walk stops at the first occupied voxel or at unknown voxel
//        number max_unknown + 1.
//     3. per target a 64-bit key (field << 32 | node) reduced by minimum and the two counts by integer sum: across the wave by
//        shuffles, then across the waves through LDS in wave order; lane 0 stores the four words.  Minimum and integer sums do not
//        depend on the order; no global atomics, one writer per output element.
//   The grid forms, the pack, the swizzle, the LDS limit, the (lds, f32) dispatch, the workgroups per env and the lattice check are
//   map_bits.h's, shared with the other kernels on the map; the voxel frame is voxel_frame.h's, the all-lanes minimum common.h's.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "map_bits.h"
#include "ray_walk.h"
#include "voxel_frame.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kViewLanes = 512;
constexpr int kViewWaves = kViewLanes / kWave;
constexpr int kViewScratchBytes = kViewWaves * 16;  // per wave: the key (8 bytes) and the two counts; in front of the bit planes
constexpr unsigned long long kNoKey = ~0ull;
constexpr uint32_t kNoRoute = 0xFFFFFFFFu;

constexpr int view_lds_max_grid() { return map_lds_max_grid(2, kViewScratchBytes); }

struct ViewArgs {
    int g, t, nx, ny, nz;
    int chunks, chunk_items;  // workgroups per env; targets per workgroup
    int shift, plane_words;   // the LDS swizzle; words of one bit plane
    int max_unknown;
    double lo[3], h[3];
    double r_max, r2_min, r2_max;
};

// the nodes [i0, i1] of one axis that may lie within r of q: the exact range of |lo + h i - q| <= r is widened by one node and by
// 2^-48 of the magnitudes over h (the rounding of lo + h i, of r * r against d2, and of this arithmetic), clamped in fp64 (a NaN
// clamps to 0: the loops stay inside the lattice)
__device__ __forceinline__ void axis_window(double q, double r, double lo, double h, int n, int &i0, int &i1)
{
    i0 = 0;
    i1 = 0;
    if (n == 1) return;
    const double top = (double)(n - 1);
    const double slack = 1.0 + ((fabs(q) + r) + fabs(lo)) / h * 0x1p-48;
    const double a = floor(((q - r) - lo) / h - slack), b = ceil(((q + r) - lo) / h + slack);
    i0 = (int)fmin(fmax(a, 0.0), top);
    i1 = (int)fmin(fmax(b, 0.0), top);
}

template <bool kLds, bool kF32>
__global__ __launch_bounds__(kViewLanes) void k_frontview(const void *__restrict__ tri_base, int64_t row_bytes,
                                                          const float *__restrict__ range_gt, const float *__restrict__ voxel_size,
                                                          const uint32_t *__restrict__ field, const int32_t *__restrict__ targets,
                                                          ViewArgs A, int32_t *__restrict__ node_out, uint32_t *__restrict__ cost_out,
                                                          int32_t *__restrict__ count_out)
{
    extern __shared__ __attribute__((aligned(16))) char view_lds[];
    unsigned long long *s_key = reinterpret_cast<unsigned long long *>(view_lds);  // [kViewWaves]
    int *s_cnt = reinterpret_cast<int *>(view_lds + kViewWaves * 8);               // [kViewWaves][2]
    uint32_t *occ = reinterpret_cast<uint32_t *>(view_lds + kViewScratchBytes), *unk = occ + A.plane_words;
    const int e = blockIdx.x / A.chunks, chunk = blockIdx.x - e * A.chunks;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const void *tri = static_cast<const char *>(tri_base) + (size_t)e * row_bytes;
    const int g = A.g;

    if (kLds) {
        map_pack_planes<kF32, kViewWaves>(tri, g, A.shift, occ, unk);
        __syncthreads();
    }

    double o[3], v[3];
    voxel_frame_f64(range_gt, voxel_size, e, o, v);
    float rmin[3], vf[3];  // what axis_to_idx takes
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        rmin[ax] = range_gt[e * 6 + 2 * ax + 1];
        vf[ax] = voxel_size[e * 3 + ax];
    }
    const size_t m = (size_t)A.nx * A.ny * A.nz;
    const uint32_t *fld = field + (size_t)e * m;

    for (int t = 0; t < A.chunk_items; ++t) {  // (every bound below is the same in all lanes: the barriers are uniform)
        const int j = chunk * A.chunk_items + t;
        if (j >= A.t) break;
        const size_t item = (size_t)e * A.t + j;
        const int tx = targets[item * 3 + 0], ty = targets[item * 3 + 1], tz = targets[item * 3 + 2];
        const bool is_target = (unsigned)tx < (unsigned)g && (unsigned)ty < (unsigned)g && (unsigned)tz < (unsigned)g;
        unsigned long long key = kNoKey;
        int n_see = 0, n_route = 0;
        if (is_target) {
            const double q[3] = {o[0] + ((double)tx + 0.5) * v[0], o[1] + ((double)ty + 0.5) * v[1], o[2] + ((double)tz + 0.5) * v[2]};
            int i0, i1, j0, j1, k0, k1;
            axis_window(q[0], A.r_max, A.lo[0], A.h[0], A.nx, i0, i1);
            axis_window(q[1], A.r_max, A.lo[1], A.h[1], A.ny, j0, j1);
            axis_window(q[2], A.r_max, A.lo[2], A.h[2], A.nz, k0, k1);
            const int wx = i1 - i0 + 1, wy = j1 - j0 + 1, wz = k1 - k0 + 1;  // >= 1 each, <= the lattice
            const int wxy = wx * wy, total = wxy * wz;                       // <= 2^30
            for (int s = tid; s < total; s += kViewLanes) {
                const int kk = s / wxy, rem = s - kk * wxy, jj = rem / wx;
                const int ix = i0 + (rem - jj * wx), iy = j0 + jj, iz = k0 + kk;
                const double px = A.lo[0] + A.h[0] * (double)ix, py = A.lo[1] + A.h[1] * (double)iy, pz = A.lo[2] + A.h[2] * (double)iz;
                const double ex = px - q[0], ey = py - q[1], ez = pz - q[2];
                const double d2 = (ex * ex + ey * ey) + ez * ez;
                if (!(d2 >= A.r2_min && d2 <= A.r2_max)) continue;  // (a NaN: not in range)
                const int c = (iz * A.ny + iy) * A.nx + ix;
                const uint32_t cost = fld[c];
                const int x0 = axis_to_idx((float)px, rmin[0], vf[0]), y0 = axis_to_idx((float)py, rmin[1], vf[1]),
                          z0 = axis_to_idx((float)pz, rmin[2], vf[2]);
                RayWalk rw = make_walk(x0, y0, z0, tx, ty, tz, g);
                // the target is in the grid and the line ends there: the last step of the range is the target's (the dominant
                // range is exact and ends at da, the minors' only widen it); dropped -- its class is not looked at
                if (rw.n > 0) --rw.n;
                int unknown = 0;
                const bool lost = run_walk(rw, g, [&](int lin, int) {
                    int cls;
                    if (kLds) {
                        const int w = map_swizzle(lin >> 5, A.shift);
                        const uint32_t bit = 1u << (lin & 31);
                        cls = (occ[w] & bit) ? 1 : ((unk[w] & bit) ? 0 : -1);
                    } else {
                        cls = voxel_class<kF32>(tri, lin);
                    }
                    if (cls > 0) return true;
                    if (cls == 0 && ++unknown > A.max_unknown) return true;
                    return false;
                });
                if (lost) continue;
                ++n_see;
                if (cost != kNoRoute) {
                    ++n_route;
                    const unsigned long long mine = ((unsigned long long)cost << 32) | (unsigned)c;
                    key = mine < key ? mine : key;
                }
            }
        }
        // ---- 3. across the wave, then across the waves in wave order
        key = wave_min_all(key);
        n_see = wave_reduce_sum(n_see);
        n_route = wave_reduce_sum(n_route);
        if (lane == 0) {
            s_key[wave] = key;
            s_cnt[2 * wave] = n_see;
            s_cnt[2 * wave + 1] = n_route;
        }
        __syncthreads();
        if (tid == 0) {
            unsigned long long best = kNoKey;
            int a = 0, b = 0;
            for (int w = 0; w < kViewWaves; ++w) {
                best = s_key[w] < best ? s_key[w] : best;
                a += s_cnt[2 * w];
                b += s_cnt[2 * w + 1];
            }
            node_out[item] = best == kNoKey ? -1 : (int32_t)(uint32_t)best;
            cost_out[item] = best == kNoKey ? kNoRoute : (uint32_t)(best >> 32);
            count_out[item * 2] = a;
            count_out[item * 2 + 1] = b;
        }
        __syncthreads();  // lane 0 has read the partials: the next target may write them
    }
}

template <bool kLds, bool kF32>
int launch_view(const MapGrid &grid, const GnbvFrontView &a, const ViewArgs &A, size_t lds, hipStream_t stream)
{
    const int bad = gnbv_raise_lds<k_frontview<kLds, kF32>>(lds, kMapLdsBytes);
    if (bad != 0) return bad;
    hipLaunchKernelGGL((k_frontview<kLds, kF32>), dim3((unsigned)(a.n * A.chunks)), dim3(kViewLanes), lds, stream, grid.base, grid.row_bytes,
                       a.range_gt, a.voxel_size, a.field, a.targets, A, a.node_out, a.cost_out, a.count_out);
    return gnbv_launch_status();
}

}  // namespace

GNBV_API int gnbv_frontview_lds_max_grid(void) { return view_lds_max_grid(); }

GNBV_API int gnbv_frontier_viewpoints(const GnbvFrontView *args, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvFrontView a = *args;
    MapGrid grid;
    const int bad = map_grid(a.tri_i8, a.tri_i8_row_stride, a.tri_f32, a.tri_f32_row_stride, a.g, &grid);
    if (bad != 0) return bad;
    GNBV_CHECK_ARG(a.range_gt != nullptr && a.voxel_size != nullptr && a.field != nullptr && a.targets != nullptr);
    GNBV_CHECK_ARG(a.node_out != nullptr && a.cost_out != nullptr && a.count_out != nullptr);
    GNBV_CHECK_ARG(a.n >= 1 && a.t >= 1 && (int64_t)a.n * a.t <= 0x7fffffff);
    GNBV_CHECK_ARG(a.mode >= 0 && a.mode <= 2 && a.chunk >= 0 && a.max_unknown >= 0);
    GNBV_CHECK_ARG(lattice_ok(a.nx, a.ny, a.nz, a.lo, a.h));
    GNBV_CHECK_ARG(std::isfinite(a.r_min) && std::isfinite(a.r_max) && a.r_min >= 0.0 && a.r_max > 0.0 && a.r_min <= a.r_max);
    const bool fits = a.g <= view_lds_max_grid();
    GNBV_CHECK_ARG(a.mode != 1 || fits);
    // auto is the grid in place: measured faster at every size and radius tried (DESIGN.md "Frontier viewpoints": a workgroup's
    // share of T = 8 targets does not pay for packing the whole grid, and the walks' byte reads stay in L2)
    const bool lds = a.mode == 1;
    ViewArgs A;
    A.g = a.g;
    A.t = a.t;
    A.nx = a.nx; A.ny = a.ny; A.nz = a.nz;
    MapChunks ch = map_chunks(a.t, 1, a.n, lds);  // the items: targets, one per workgroup and turn
    if (a.chunk > 0) {                            // the caller's targets per workgroup
        ch.per = std::min(a.chunk, a.t);
        ch.chunks = (a.t + ch.per - 1) / ch.per;
    }
    A.chunk_items = ch.per;
    A.chunks = ch.chunks;
    GNBV_CHECK_ARG((int64_t)a.n * A.chunks <= 0x7fffffff);
    A.shift = map_swizzle_shift(a.g);
    A.plane_words = lds ? (int)(map_lds_bytes(a.g) / 4) : 0;
    A.max_unknown = a.max_unknown;
    for (int ax = 0; ax < 3; ++ax) {
        A.lo[ax] = a.lo[ax];
        A.h[ax] = a.h[ax];
    }
    A.r_max = a.r_max;
    A.r2_min = a.r_min * a.r_min;
    A.r2_max = a.r_max * a.r_max;
    const size_t bytes = kViewScratchBytes + (lds ? 2 * map_lds_bytes(a.g) : 0);
    return map_dispatch(lds, grid.f32, [&](auto kLds, auto kF32) {
        return launch_view<decltype(kLds)::value, decltype(kF32)::value>(grid, a, A, bytes, gnbv_stream(stream));
    });
}

// sweepmap.hip -- a straight flight judged on the scanned map (gnbv_sweep_tri): the sphere of radius R moved along N x K straight
// legs, tested against each env's tri-class grid (< 0 free, 0 unknown, > 0 occupied: gnbv_flight_blocked_tri's forms and signs).
//
// sweep.hip asks the ground-truth mesh whether a leg is flyable, flightmap.hip asks the map about balls at lattice nodes; this file
// asks the map about a leg.  Item (e, j) is the segment a -> b (the xyz of `from` and `to`, fp32 taken to fp64; the item layout of
// gnbv_sweep_sphere), code_out[e, j]:
//
//   bit 0 (1, MAP)      some voxel that blocks (occupied, or unknown with unknown_blocks) is touched: its closed box lies within R
//                       of the segment (seg_box.h has the predicate: fp64, closed form)
//   bit 1 (2, OUTSIDE)  outside_blocks and on some axis min(a, b) - R < o or max(a, b) + R > o + (double)G v
//   bit 2 (4, GROUND)   ground and min(a_z, b_z) - R <= 0
//
// An item with a non-finite coordinate gets 0.  The voxel frame is gnbv_pose_to_idx's (voxel_frame.h: voxel_frame_f64).  The grid
// forms, the LDS pack and swizzle, the span of a word, the LDS limit, the (lds, f32) dispatch and the workgroups per env are
// map_bits.h's, shared with the other kernels on the map.
//
//   k_sweep_tri<kLds, kF32>   workgroup (env, chunk of the env's K items), 512 lanes, a wave owns an item at a time; the work
//     follows the segment, as in sweep.hip:
//     1. the segment is clipped to the grid grown by R and the clipped part is cut into pieces of about the shortest voxel edge
//        (at most kMaxPieces: longer pieces have larger windows, never dropped voxels);
//     2. per piece: the voxel window of its R-grown box (clamped to the grid in fp64 before conversion, so every loop runs at most
//        G times per axis whatever the device arrays hold).  All pieces have the same extent, so one bound wx x wy holds every
//        window's columns, and the (piece, column) pairs are dealt to the lanes 64 at a time: a leg of many small windows and a
//        short leg with one large window both fill the wave, and a wave waits for memory once per 64 pairs, not once per piece.
//        Of each column the lane walks the z-run minus what the previous piece's window held -- that voxel is tested by the
//        previous piece's lanes, against the WHOLE segment;
//     3. the bit first, then the geometry: only a voxel that blocks gets the fp64 predicate, free space costs no arithmetic;
//     4. the whole wave leaves at the first hit (__any, once per 64 pairs); lane 0 stores the byte.  No atomics, no workspace.
//     kLds (mode 1): the workgroup first packs "this voxel blocks" into one bit per voxel in LDS (map_bits.h: the pack and the bank
//       swizzle) and amortises that over its items; a z-run is read as whole words and a zero word is skipped.
//     !kLds (mode 2): the same decisions with the voxels read from global memory (up to 128^3).
#include <cmath>

#include "common.h"
#include "map_bits.h"
#include "seg_box.h"
#include "voxel_frame.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kSweepLanes = 512;
constexpr int kSweepWaves = kSweepLanes / kWave;
constexpr int kMaxPieces = 1024;

struct SweepMapArgs {
    int g, k;
    int chunks, chunk_items;  // workgroups per env; items per workgroup
    int shift;                // the LDS swizzle
    int unknown_blocks, outside_blocks, ground;
    int64_t from_env_stride, from_item_stride, to_row_stride;
    double radius, r2;
};

struct Window {  // inclusive voxel ranges; valid = not empty
    int lo[3], hi[3];
    bool valid;
};

// the clipped segment cut into np pieces: piece p is s in [s0 + (s1 - s0) p / np, s0 + (s1 - s0) (p + 1) / np]
struct Pieces {
    double s0, s1, grow;
    int np;
};

// the voxel window of piece p's R-grown box, clamped to the grid in fp64 before conversion
__device__ __forceinline__ Window piece_window(const Pieces &pc, int p, const double *o, const double *v, int g, const double *a,
                                               const double *d)
{
    Window w;
    const double top = (double)(g - 1);
    const double sa = pc.s0 + (pc.s1 - pc.s0) * ((double)p / (double)pc.np), sb = pc.s0 + (pc.s1 - pc.s0) * ((double)(p + 1) / (double)pc.np);
    bool empty = false;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double xa = a[ax] + d[ax] * sa, xb = a[ax] + d[ax] * sb;
        const double f0 = floor(((fmin(xa, xb) - pc.grow) - o[ax]) / v[ax]), f1 = floor(((fmax(xa, xb) + pc.grow) - o[ax]) / v[ax]);
        empty = empty || !(f1 >= 0.0) || !(f0 <= top);  // (a NaN: empty)
        w.lo[ax] = (int)fmin(fmax(f0, 0.0), top);       // (a NaN clamps to 0: the loops stay inside the grid)
        w.hi[ax] = (int)fmin(fmax(f1, 0.0), top);
    }
    w.valid = !empty;
    return w;
}

// does the sphere moved along a -> b touch a blocking voxel of the env's grid?  One wave; the same answer in every lane.
template <bool kLds, bool kF32>
__device__ __forceinline__ bool leg_touches_map(const SweepMapArgs &A, const double *o, const double *v, const double *a, const double *b,
                                                const void *__restrict__ tri, const uint32_t *bits, int lane)
{
    const int g = A.g;
    const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double amax = fmax(fmax(fmax(fabs(a[0]), fabs(b[0])), fmax(fabs(a[1]), fabs(b[1]))), fmax(fabs(a[2]), fabs(b[2])));
    Pieces pc;
    pc.grow = A.radius + 1e-12 * (amax + A.radius);  // R, and the rounding of the piece ends
    // ---- 1. the part s in [s0, s1] of the segment inside the grid grown by R
    pc.s0 = 0.0;
    pc.s1 = 1.0;
    double vmin = 0.0;
    bool any = true;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        vmin = ax == 0 ? v[ax] : fmin(vmin, v[ax]);
        const double pad = pc.grow + 1e-6 * v[ax];
        const double glo = o[ax] - pad, ghi = o[ax] + (double)g * v[ax] + pad;
        if (d[ax] == 0.0) {
            any = any && a[ax] >= glo && a[ax] <= ghi;
        } else {
            const double u0 = (glo - a[ax]) / d[ax], u1 = (ghi - a[ax]) / d[ax];
            pc.s0 = fmax(pc.s0, fmin(u0, u1) - 1e-9);
            pc.s1 = fmin(pc.s1, fmax(u0, u1) + 1e-9);
        }
    }
    if (!any || !(pc.s0 <= pc.s1)) return false;
    const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * (pc.s1 - pc.s0);
    pc.np = (int)fmin(fmax(ceil(len / vmin), 1.0), (double)kMaxPieces);  // (a NaN gives 1)
    // every piece's window has at most wx x wy columns: a box of extent L meets at most floor(L / v) + 2 voxels of an axis (L with a
    // relative 1e-9 on top: the pieces' own ends are rounded)
    int wxy[2];
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
        const double ext = fabs(d[ax]) * (pc.s1 - pc.s0) / (double)pc.np + 2.0 * pc.grow;
        wxy[ax] = (int)fmin(fmax(floor(ext / v[ax] * (1.0 + 1e-9)) + 2.0, 1.0), (double)g);  // (a NaN gives 1)
    }
    const int wy = wxy[1], cols = wxy[0] * wy;  // <= G^2
    const int total = pc.np * cols;             // <= kMaxPieces G^2 < 2^31
    const bool unk = A.unknown_blocks != 0;

    // ---- 2./3. the (piece, column) pairs dealt to the lanes, 64 at a time (np, cols and total are wave-uniform)
    for (int t0 = 0; t0 < total; t0 += kWave) {
        const int t = t0 + lane;
        bool hit = false;
        if (t < total) {
            const int p = t / cols, c = t - p * cols;
            const Window w = piece_window(pc, p, o, v, g, a, d);
            const int x = w.lo[0] + c / wy, y = w.lo[1] + c % wy;
            if (w.valid && x <= w.hi[0] && y <= w.hi[1]) {
                int z0 = w.lo[2], z1 = w.hi[2];
                if (p > 0) {
                    // minus what the previous piece's window held: that voxel is tested, against the WHOLE segment, by that piece's
                    // lanes (along a straight line the z-runs move one way: what is left is one run)
                    const Window q = piece_window(pc, p - 1, o, v, g, a, d);
                    if (q.valid && x >= q.lo[0] && x <= q.hi[0] && y >= q.lo[1] && y <= q.hi[1]) {
                        if (q.lo[2] <= z0 && q.hi[2] >= z0) z0 = q.hi[2] + 1;
                        else if (q.hi[2] >= z1 && q.lo[2] <= z1) z1 = q.lo[2] - 1;
                    }
                }
                if (z0 <= z1) {
                    double lo[3], hi[3];
                    lo[0] = o[0] + (double)x * v[0];
                    hi[0] = o[0] + (double)(x + 1) * v[0];
                    lo[1] = o[1] + (double)y * v[1];
                    hi[1] = o[1] + (double)(y + 1) * v[1];
                    const int base = (x * g + y) * g;
                    if (kLds) {
                        const int b0 = base + z0, b1 = base + z1;
                        for (int wd = b0 >> 5; wd <= (b1 >> 5) && !hit; ++wd) {
                            uint32_t word = bits[map_swizzle(wd, A.shift)] & map_span(wd, b0, b1);
                            while (word != 0u) {
                                const int z = (wd << 5) + __builtin_ctz(word) - base;
                                word &= word - 1u;
                                lo[2] = o[2] + (double)z * v[2];
                                hi[2] = o[2] + (double)(z + 1) * v[2];
                                if (seg_box_within(a, b, d, lo, hi, A.r2)) {
                                    hit = true;
                                    break;
                                }
                            }
                        }
                    } else {
                        for (int z = z0; z <= z1; ++z) {
                            if (!voxel_blocks<kF32>(tri, base + z, unk)) continue;
                            lo[2] = o[2] + (double)z * v[2];
                            hi[2] = o[2] + (double)(z + 1) * v[2];
                            if (seg_box_within(a, b, d, lo, hi, A.r2)) {
                                hit = true;
                                break;
                            }
                        }
                    }
                }
            }
        }
        if (__any(hit)) return true;
    }
    return false;
}

template <bool kLds, bool kF32>
__global__ __launch_bounds__(kSweepLanes) void k_sweep_tri(const void *__restrict__ tri_base, int64_t row_bytes,
                                                           const float *__restrict__ range_gt, const float *__restrict__ voxel_size,
                                                           const float *__restrict__ from, const float *__restrict__ to, SweepMapArgs A,
                                                           uint8_t *__restrict__ code_out)
{
    extern __shared__ __attribute__((aligned(16))) char sweepmap_lds[];
    uint32_t *bits = reinterpret_cast<uint32_t *>(sweepmap_lds);
    const int e = blockIdx.x / A.chunks, chunk = blockIdx.x - e * A.chunks;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const void *tri = static_cast<const char *>(tri_base) + (size_t)e * row_bytes;

    if (kLds) {
        map_pack_bits<kF32, kSweepWaves>(tri, A.g, A.unknown_blocks != 0, A.shift, bits);
        __syncthreads();
    }

    double o[3], v[3];
    voxel_frame_f64(range_gt, voxel_size, e, o, v);

    for (int t = wave; t < A.chunk_items; t += kSweepWaves) {  // (no barrier below: a wave may leave alone)
        const int j = chunk * A.chunk_items + t;
        if (j >= A.k) break;
        const size_t item = (size_t)e * A.k + j;
        const float *pf = from + (size_t)e * A.from_env_stride + (size_t)j * A.from_item_stride;
        const float *pt = to + item * A.to_row_stride;
        const double a[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        const double b[3] = {(double)pt[0], (double)pt[1], (double)pt[2]};
        uint8_t code = 0;
        if (isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]) && isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2])) {
            bool outside = false;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
                outside = outside || fmin(a[ax], b[ax]) - A.radius < o[ax] || fmax(a[ax], b[ax]) + A.radius > o[ax] + (double)A.g * v[ax];
            if (A.outside_blocks && outside) code |= 2;
            if (A.ground && fmin(a[2], b[2]) - A.radius <= 0.0) code |= 4;
            if (leg_touches_map<kLds, kF32>(A, o, v, a, b, tri, bits, lane)) code |= 1;
        }
        if (lane == 0) code_out[item] = code;
    }
}

template <bool kLds, bool kF32>
int launch_sweep(const MapGrid &grid, const float *range_gt, const float *voxel_size, const float *from, const float *to, const SweepMapArgs &A,
                 int n, size_t lds, uint8_t *code_out, hipStream_t stream)
{
    const int bad = gnbv_raise_lds<k_sweep_tri<kLds, kF32>>(lds, kMapLdsBytes);
    if (bad != 0) return bad;
    hipLaunchKernelGGL((k_sweep_tri<kLds, kF32>), dim3((unsigned)(n * A.chunks)), dim3(kSweepLanes), lds, stream, grid.base, grid.row_bytes,
                       range_gt, voxel_size, from, to, A, code_out);
    return gnbv_launch_status();
}

}  // namespace

GNBV_API int gnbv_sweepmap_lds_max_grid(void) { return map_lds_max_grid(); }

GNBV_API int gnbv_sweep_tri(const int8_t *tri_i8, int64_t tri_i8_row_stride, const float *tri_f32, int64_t tri_f32_row_stride, int g,
                            const float *range_gt, const float *voxel_size, int n, const float *from, int64_t from_env_stride,
                            int64_t from_item_stride, const float *to, int k, int64_t to_row_stride, double radius, int unknown_blocks,
                            int outside_blocks, int ground, uint8_t *code_out, int mode, void *stream)
{
    MapGrid grid;
    const int bad = map_grid(tri_i8, tri_i8_row_stride, tri_f32, tri_f32_row_stride, g, &grid);
    if (bad != 0) return bad;
    GNBV_CHECK_ARG(range_gt != nullptr && voxel_size != nullptr && from != nullptr && to != nullptr && code_out != nullptr);
    GNBV_CHECK_ARG(n >= 1 && k >= 1 && mode >= 0 && mode <= 2);
    GNBV_CHECK_ARG(std::isfinite(radius) && radius > 0.0);
    GNBV_CHECK_ARG(to_row_stride >= 3 && from_env_stride >= 3 && (from_item_stride == 0 || from_item_stride >= 3));
    const bool fits = g <= map_lds_max_grid();
    GNBV_CHECK_ARG(mode != 1 || fits);
    const bool lds = mode == 1 || (mode == 0 && fits);
    SweepMapArgs A;
    A.g = g;
    A.k = k;
    const MapChunks ch = map_chunks(k, kSweepWaves, n, lds);  // the items: legs, one per wave and turn
    A.chunks = ch.chunks;
    A.chunk_items = ch.per;
    GNBV_CHECK_ARG((int64_t)n * A.chunks <= 0x7fffffff && (int64_t)n * k <= 0x7fffffff);
    A.shift = map_swizzle_shift(g);
    A.unknown_blocks = unknown_blocks != 0;
    A.outside_blocks = outside_blocks != 0;
    A.ground = ground != 0;
    A.from_env_stride = from_env_stride;
    A.from_item_stride = from_item_stride;
    A.to_row_stride = to_row_stride;
    A.radius = radius;
    A.r2 = radius * radius;
    const size_t bytes = lds ? map_lds_bytes(g) : 0;
    return map_dispatch(lds, grid.f32, [&](auto kLds, auto kF32) {
        return launch_sweep<decltype(kLds)::value, decltype(kF32)::value>(grid, range_gt, voxel_size, from, to, A, n, bytes, code_out,
                                                                          gnbv_stream(stream));
    });
}

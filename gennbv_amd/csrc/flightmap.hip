// flightmap.hip -- the free set of the flight lattice from the map the agent has scanned so far (gnbv_flight_blocked_tri,
// gnbv_flight_classify_tri).
//
// flight.hip routes over blocked bits; MeshScene.flight_blocked takes them from the ground-truth mesh.  This file takes them from
// an env's own tri-class grid (< 0 free, 0 unknown, > 0 occupied: gnbv_view_gain's signs), once per env step: node c of env e is
// blocked iff the closed ball of radius rho round the node touches an occupied voxel (or, by flag, an unknown one, the outside of
// the grid, the ground).  The predicate is exact -- fp64, one fixed operation order, no FMA (include/gennbv_hip.h states it; the
// library is built with -ffp-contract=off) -- so tests compare every u32 of the output with a numpy restatement.
//
// Shared with the other kernels on the map: the grid forms, the LDS pack and swizzle, the span of a word, the LDS limit, the
// (lds, f32) dispatch, the workgroups per env and the lattice check are map_bits.h's; the voxel frame is voxel_frame.h's.
//
//   k_flight_tri<kLds, kF32, kTell>   workgroup (env, chunk of nodes), 512 lanes; a wave owns 64 consecutive nodes at a time and
//     stores their ballot as two whole words of blocked_out: one writer per word, no atomics.  Nodes at or past M (padding) count
//     as blocked.  Per node: the per-axis voxel window [i0, i1] of the ball (clamped to the grid in fp64 before conversion, so every
//     loop below runs at most G times whatever the device arrays hold), then x, y, z over the window with gx^2 and gx^2 + gy^2
//     hoisted; a partial sum already above rho^2 skips the rest (adding a square >= 0 never lowers a rounded sum).  The walk ends at
//     the first touched blocking voxel.
//     kLds (mode 1): the workgroup first packs "this voxel blocks" into one bit per voxel in LDS (64 voxels per wave ballot,
//       coalesced reads of either grid form; G^3 / 8 bytes, 32 KiB at 64^3) and a node reads the z-run of a (x, y) column as whole
//       words: a word with no blocking bit inside the window costs no arithmetic.  Lanes of a wave are x-neighbours, their words lie
//       G^2 / 32 apart -- at G = 64 all on one bank -- so the words are swizzled.
//     !kLds (mode 2): the same decisions with the voxels read from global memory, for grids whose bits do not fit (up to 128^3).
//     kF32: the grid is the fp32 slice of an observation row, else int8 rows.
//     kTell (gnbv_flight_classify_tri): unknown space is told apart.  Two outputs: "blocked" as with unknown_blocks = 0, and "costly"
//       = not blocked, but the ball touches an unknown voxel -- what two launches without kTell (unknown_blocks = 0 and 1) and an
//       AND-NOT would give, from one pass over the window.  The walk still ends at the first touched occupied voxel; a touched
//       unknown voxel only sets a flag, and from then on unknown voxels are skipped.
//       kLds: two bit planes, occupied then unknown (every voxel read once), G^3 / 4 bytes, so the limit is lower
//       (map_planes_max_grid, 86); a word of the window is occ | unk until the flag is set, occ alone afterwards.
#include <cmath>

#include "common.h"
#include "map_bits.h"
#include "voxel_frame.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kMapLanes = 512;
constexpr int kMapWaves = kMapLanes / kWave;

struct MapArgs {
    int g, nx, ny, nz, m, words;
    int chunks, chunk_waves;  // workgroups per env; 64-node groups per workgroup
    int shift, plane_words;   // the LDS swizzle; words of one bit plane
    int unknown_blocks, outside_blocks, ground;
    double lo[3], h[3], rho, rho2;
};

// the squared gap on one axis between node coordinate p and voxel i = [o + i v, o + (i + 1) v]
__device__ __forceinline__ double gap2(double o, double v, int i, double p)
{
    const double below = o + (double)i * v - p;
    const double above = p - (o + (double)(i + 1) * v);
    const double gap = fmax(fmax(below, 0.0), above);
    return gap * gap;
}

// the ball of node c: its centre, its per-axis voxel window [i0, i1] (clamped to the grid in fp64 before conversion), whether it
// leaves the grid and whether the window is empty
struct NodeWindow {
    double p[3];
    int i0[3], i1[3];
    bool outside, empty;
};

__device__ __forceinline__ NodeWindow node_window(const MapArgs &a, int c, const double *o, const double *v)
{
    const int g = a.g;
    const int idx[3] = {c % a.nx, (c / a.nx) % a.ny, c / (a.nx * a.ny)};
    const double top = (double)(g - 1);
    NodeWindow n;
    n.outside = false;
    n.empty = false;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        n.p[ax] = a.lo[ax] + a.h[ax] * (double)idx[ax];
        const double pm = n.p[ax] - a.rho, pp = n.p[ax] + a.rho;
        const double f0 = floor((pm - o[ax]) / v[ax]), f1 = floor((pp - o[ax]) / v[ax]);
        n.empty = n.empty || f1 < 0.0 || f0 > top;
        n.i0[ax] = (int)fmin(fmax(f0, 0.0), top);  // (a NaN clamps to 0: the loops stay inside the grid)
        n.i1[ax] = (int)fmin(fmax(f1, 0.0), top);
        n.outside = n.outside || pm < o[ax] || pp > o[ax] + (double)g * v[ax];
    }
    return n;
}

// The class of node c.  kBlocked where the ball touches a voxel that blocks (or the outside / the ground, by flag): the walk ends
// there.  !kTell: a voxel blocks where it is occupied, or unknown with a.unknown_blocks; `blk` is that one plane and the answer is
// kBlocked or kClear.  kTell: only an occupied voxel blocks (`blk`), and a touched unknown one (`unk`) makes the node kCostly unless
// it turns out blocked: a flag, the walk goes on, looking for occupied voxels only.
enum { kClear = 0, kBlocked = 1, kCostly = 2 };

template <bool kLds, bool kF32, bool kTell>
__device__ __forceinline__ int node_class(const MapArgs &a, int c, const double *o, const double *v, const void *__restrict__ tri,
                                          const uint32_t *blk, const uint32_t *unk)
{
    const int g = a.g;
    const NodeWindow n = node_window(a, c, o, v);
    const double *p = n.p;
    const int *i0 = n.i0, *i1 = n.i1;
    if (a.outside_blocks && n.outside) return kBlocked;
    if (a.ground && p[2] - a.rho <= 0.0) return kBlocked;
    if (n.empty) return kClear;
    const bool unknown_blocks = !kTell && a.unknown_blocks != 0;
    bool costly = false;
    for (int x = i0[0]; x <= i1[0]; ++x) {
        const double gx2 = gap2(o[0], v[0], x, p[0]);
        if (gx2 > a.rho2) continue;
        for (int y = i0[1]; y <= i1[1]; ++y) {
            const double s = gx2 + gap2(o[1], v[1], y, p[1]);
            if (s > a.rho2) continue;
            const int base = (x * g + y) * g;
            if (kLds) {
                const int b0 = base + i0[2], b1 = base + i1[2];
                for (int w = b0 >> 5; w <= (b1 >> 5); ++w) {
                    const uint32_t span = map_span(w, b0, b1);
                    const int at = map_swizzle(w, a.shift);
                    const uint32_t wb = blk[at] & span;
                    uint32_t word = wb;
                    if (kTell && !costly) word |= unk[at] & span;  // (once costly, unknown voxels decide nothing)
                    while (word != 0u) {
                        const int bit = __builtin_ctz(word);
                        word &= word - 1u;
                        if (s + gap2(o[2], v[2], (w << 5) + bit - base, p[2]) > a.rho2) continue;
                        if (!kTell || ((wb >> bit) & 1u)) return kBlocked;
                        costly = true;
                    }
                }
            } else {
                for (int z = i0[2]; z <= i1[2]; ++z) {
                    const int cls = voxel_class<kF32>(tri, base + z);
                    const bool blocks = cls > 0 || (unknown_blocks && cls == 0);
                    if (!blocks && !(kTell && cls == 0 && !costly)) continue;
                    if (s + gap2(o[2], v[2], z, p[2]) > a.rho2) continue;
                    if (blocks) return kBlocked;
                    costly = true;
                }
            }
        }
    }
    return costly ? kCostly : kClear;
}

// the ballot of kBlocked (padding set) into blocked_out and, with kTell, the ballot of kCostly (padding clear) into costly_out
template <bool kLds, bool kF32, bool kTell>
__global__ __launch_bounds__(kMapLanes) void k_flight_tri(const void *__restrict__ tri_base, int64_t row_bytes,
                                                          const float *__restrict__ range_gt, const float *__restrict__ voxel_size, MapArgs a,
                                                          uint32_t *__restrict__ blocked_out, uint32_t *__restrict__ costly_out)
{
    extern __shared__ __attribute__((aligned(16))) char map_lds[];
    uint32_t *blk = reinterpret_cast<uint32_t *>(map_lds), *unk = blk + a.plane_words;
    const int e = blockIdx.x / a.chunks, chunk = blockIdx.x - e * a.chunks;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const void *tri = static_cast<const char *>(tri_base) + (size_t)e * row_bytes;

    if (kLds) {
        if (kTell) map_pack_planes<kF32, kMapWaves>(tri, a.g, a.shift, blk, unk);
        else map_pack_bits<kF32, kMapWaves>(tri, a.g, a.unknown_blocks != 0, a.shift, blk);
        __syncthreads();
    }

    double o[3], v[3];
    voxel_frame_f64(range_gt, voxel_size, e, o, v);

    uint32_t *out_b = blocked_out + (size_t)e * a.words, *out_c = kTell ? costly_out + (size_t)e * a.words : nullptr;
    for (int t = wave; t < a.chunk_waves; t += kMapWaves) {
        const int c0 = (chunk * a.chunk_waves + t) * kWave, c = c0 + lane;
        int cls = kBlocked;  // padding
        if (c < a.m) cls = node_class<kLds, kF32, kTell>(a, c, o, v, tri, blk, unk);
        const unsigned long long mb = __ballot(cls == kBlocked), mc = __ballot(cls == kCostly);
        const int w = c0 >> 5;
        if (lane == 0 && w < a.words) {
            out_b[w] = (uint32_t)mb;
            if (kTell) out_c[w] = (uint32_t)mc;
        }
        if (lane == 0 && w + 1 < a.words) {
            out_b[w + 1] = (uint32_t)(mb >> 32);
            if (kTell) out_c[w + 1] = (uint32_t)(mc >> 32);
        }
    }
}

template <bool kLds, bool kF32, bool kTell>
int launch_map(const MapGrid &grid, const float *range_gt, const float *voxel_size, const MapArgs &a, int n, size_t lds,
               uint32_t *blocked_out, uint32_t *costly_out, hipStream_t stream)
{
    const int bad = gnbv_raise_lds<k_flight_tri<kLds, kF32, kTell>>(lds, kMapLdsBytes);
    if (bad != 0) return bad;
    hipLaunchKernelGGL((k_flight_tri<kLds, kF32, kTell>), dim3((unsigned)(n * a.chunks)), dim3(kMapLanes), lds, stream, grid.base,
                       grid.row_bytes, range_gt, voxel_size, a, blocked_out, costly_out);
    return gnbv_launch_status();
}

// the body of the two entry points: the argument checks, the launch shape, the launch.  kTell: costly_out is written too and
// unknown_blocks is 0; mode 1 holds two planes, so its limit is lower.
template <bool kTell>
int flight_tri(const int8_t *tri_i8, int64_t tri_i8_row_stride, const float *tri_f32, int64_t tri_f32_row_stride, int g, const float *range_gt,
               const float *voxel_size, int n, int nx, int ny, int nz, const double *lo, const double *h, double rho, int unknown_blocks,
               int outside_blocks, int ground, uint32_t *blocked_out, uint32_t *costly_out, int mode, void *stream)
{
    MapGrid grid;
    const int bad = map_grid(tri_i8, tri_i8_row_stride, tri_f32, tri_f32_row_stride, g, &grid);
    if (bad != 0) return bad;
    GNBV_CHECK_ARG(range_gt != nullptr && voxel_size != nullptr && blocked_out != nullptr && lo != nullptr && h != nullptr);
    GNBV_CHECK_ARG(!kTell || costly_out != nullptr);
    GNBV_CHECK_ARG(n >= 1 && mode >= 0 && mode <= 2);
    GNBV_CHECK_ARG(std::isfinite(rho) && rho > 0.0);
    GNBV_CHECK_ARG(lattice_ok(nx, ny, nz, lo, h));
    constexpr int kPlanes = kTell ? 2 : 1;
    const bool fits = g <= map_lds_max_grid(kPlanes);
    GNBV_CHECK_ARG(mode != 1 || fits);
    const bool lds = mode == 1 || (mode == 0 && fits);
    MapArgs a;
    for (int ax = 0; ax < 3; ++ax) {
        a.lo[ax] = lo[ax];
        a.h[ax] = h[ax];
    }
    const int64_t m = (int64_t)nx * ny * nz;
    a.g = g;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.m = (int)m;
    a.words = (int)((m + 31) / 32);
    const MapChunks ch = map_chunks((m + kWave - 1) / kWave, kMapWaves, n, lds);  // the items: 64-node groups, one per wave and turn
    a.chunks = ch.chunks;
    a.chunk_waves = ch.per;
    GNBV_CHECK_ARG((int64_t)n * a.chunks <= 0x7fffffff);
    a.shift = map_swizzle_shift(g);
    a.plane_words = lds ? (int)(map_lds_bytes(g) / 4) : 0;
    a.unknown_blocks = unknown_blocks != 0;
    a.outside_blocks = outside_blocks != 0;
    a.ground = ground != 0;
    a.rho = rho;
    a.rho2 = rho * rho;
    const size_t bytes = lds ? kPlanes * map_lds_bytes(g) : 0;
    return map_dispatch(lds, grid.f32, [&](auto kLds, auto kF32) {
        return launch_map<decltype(kLds)::value, decltype(kF32)::value, kTell>(grid, range_gt, voxel_size, a, n, bytes, blocked_out, costly_out,
                                                                              gnbv_stream(stream));
    });
}

}  // namespace

GNBV_API int gnbv_flightmap_lds_max_grid(void) { return map_lds_max_grid(); }

GNBV_API int gnbv_flight_blocked_tri(const int8_t *tri_i8, int64_t tri_i8_row_stride, const float *tri_f32, int64_t tri_f32_row_stride,
                                     int g, const float *range_gt, const float *voxel_size, int n, int nx, int ny, int nz, const double *lo,
                                     const double *h, double rho, int unknown_blocks, int outside_blocks, int ground,
                                     uint32_t *blocked_out, int mode, void *stream)
{
    return flight_tri<false>(tri_i8, tri_i8_row_stride, tri_f32, tri_f32_row_stride, g, range_gt, voxel_size, n, nx, ny, nz, lo, h, rho,
                             unknown_blocks, outside_blocks, ground, blocked_out, nullptr, mode, stream);
}

GNBV_API int gnbv_flightmap_classify_lds_max_grid(void) { return map_planes_max_grid(); }

GNBV_API int gnbv_flight_classify_tri(const int8_t *tri_i8, int64_t tri_i8_row_stride, const float *tri_f32, int64_t tri_f32_row_stride,
                                      int g, const float *range_gt, const float *voxel_size, int n, int nx, int ny, int nz, const double *lo,
                                      const double *h, double rho, int outside_blocks, int ground, uint32_t *blocked_out,
                                      uint32_t *costly_out, int mode, void *stream)
{
    return flight_tri<true>(tri_i8, tri_i8_row_stride, tri_f32, tri_f32_row_stride, g, range_gt, voxel_size, n, nx, ny, nz, lo, h, rho, 0,
                            outside_blocks, ground, blocked_out, costly_out, mode, stream);
}

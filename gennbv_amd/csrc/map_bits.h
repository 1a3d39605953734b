// map_bits.h -- what every kernel that reads an env's tri-class grid (< 0 free, 0 unknown, > 0 occupied) shares: flightmap.hip,
// sweepmap.hip, frontier.hip, frontview.hip.  Nothing here may be restated elsewhere.
//
//   device  a voxel read in place (voxel_class, voxel_blocks); the grid packed into LDS bit planes, one bit per voxel
//           (map_pack_bits: one plane; map_pack: the two-plane loop, with map_pack_planes and map_pack_window its callers); the
//           swizzle; the bits of a word inside a run (map_span).
//   host    the front end of the entry points: the grid forms resolved and checked (map_grid), the dynamic-LDS limit raised once
//           per kernel (gnbv_raise_lds, common.h), (lds, f32) turned into template arguments (map_dispatch), the workgroups of an env
//           (map_chunks), the geometry of a flight lattice (lattice_ok: flight.hip uses it too).
//   The fp64 voxel frame these kernels place the grid with is voxel_frame.h's (voxel_frame_f64).
//
// The packed form: voxel (x G + y) G + z is bit (vox & 31) of word vox >> 5, 64 voxels per wave ballot.  Lanes of a wave that read
// x-neighbours touch words G^2 / 32 apart -- at G = 64 all on one bank -- so word w is kept at w ^ ((w >> shift) & 31),
// shift ~ log2(G^2 / 32), >= 5: a permutation inside each aligned group of 32 words that spreads x-neighbours over the banks.
#pragma once

#include <stddef.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.h"

constexpr int kMapLdsBytes = 160 * 1024;
constexpr int kMapMaxGrid = 128;

// LDS of the packed form: one bit per voxel in whole 64-voxel ballots, rounded up to a group of 32 words (the swizzle stays inside
// a group)
constexpr size_t map_lds_bytes(int g)
{
    const size_t words = 2 * (((size_t)g * g * g + 63) / 64);
    return 4 * ((words + 31) / 32 * 32);
}

// the largest grid whose `planes` bit planes, each map_lds_bytes(g) long (whole groups of 32 words: the swizzle of a plane stays
// inside it), fit LDS beside `extra` bytes
constexpr int map_lds_max_grid(int planes = 1, size_t extra = 0)
{
    int g = 1;
    while (g < kMapMaxGrid && planes * map_lds_bytes(g + 1) + extra <= (size_t)kMapLdsBytes) ++g;
    return g;
}

// two planes, "occupied" then "unknown" (gnbv_flight_classify_tri)
constexpr int map_planes_max_grid() { return map_lds_max_grid(2); }

// the swizzle's shift for a G^3 grid: ~ round(log2(G^2 / 32)), at least 5
static inline int map_swizzle_shift(int g)
{
    int shift = 5;
    while (shift < 20 && (2 << shift) * 3 <= (g * g / 32) * 4) ++shift;
    return shift;
}

// the class of a voxel: 1 occupied, 0 unknown, -1 free
template <bool kF32>
__device__ __forceinline__ int voxel_class(const void *__restrict__ tri, int idx)
{
    if (kF32) {
        const float t = static_cast<const float *>(tri)[idx];
        return t > 0.0f ? 1 : (t == 0.0f ? 0 : -1);
    }
    const int t = static_cast<const int8_t *>(tri)[idx];
    return t > 0 ? 1 : (t == 0 ? 0 : -1);
}

// does the voxel block?  (The one-plane pack and sweepmap.hip decide on the value itself: one compare less per voxel than through
// the class.)
template <bool kF32>
__device__ __forceinline__ bool voxel_blocks(const void *__restrict__ tri, int idx, bool unknown_blocks)
{
    if (kF32) {
        const float t = static_cast<const float *>(tri)[idx];
        return t > 0.0f || (unknown_blocks && t == 0.0f);
    }
    const int t = static_cast<const int8_t *>(tri)[idx];
    return t > 0 || (unknown_blocks && t == 0);
}

__device__ __forceinline__ int map_swizzle(int w, int shift) { return w ^ ((w >> shift) & 31); }

// the bits of word w (voxels 32 w .. 32 w + 31) that lie in the run of voxels [b0, b1], for w in b0 >> 5 .. b1 >> 5
__device__ __forceinline__ uint32_t map_span(int w, int b0, int b1)
{
    const int first = max(b0, w << 5), last = min(b1, (w << 5) + 31);
    return (0xFFFFFFFFu >> (31 - (last - first))) << (first & 31);
}

// The packs: the whole workgroup (kWaves waves) turns voxels of one env's grid into LDS bit planes; the caller synchronises
// afterwards.  A wave takes GNBV_MAP_PACK_UNROLL ballots per turn and issues their loads together: one load per turn leaves the
// pack waiting for memory once per 64 voxels.  Two loops: the one-plane pack decides on the voxel's value, the two-plane pack on
// its class; folded into one, the int8 one-plane pack measured 1 % slower (DESIGN.md "The family's shared front end").
#ifndef GNBV_MAP_PACK_UNROLL
#define GNBV_MAP_PACK_UNROLL 8
#endif

// one env's whole G^3 grid as one swizzled plane, "this voxel blocks"
template <bool kF32, int kWaves>
__device__ __forceinline__ void map_pack_bits(const void *__restrict__ tri, int g, bool unknown_blocks, int shift, uint32_t *bits)
{
    constexpr int kUnroll = GNBV_MAP_PACK_UNROLL;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int g3 = g * g * g, groups = (g3 + kWave - 1) / kWave;
    for (int q0 = wave; q0 < groups; q0 += kWaves * kUnroll) {  // (q is the same in every lane of a wave: the ballots are whole)
        bool b[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vox = (q0 + u * kWaves) * kWave + lane;
            b[u] = voxel_blocks<kF32>(tri, min(vox, g3 - 1), unknown_blocks) && vox < g3;  // (the load is unconditional: no branch, no wait)
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int q = q0 + u * kWaves;
            const unsigned long long mask = __ballot(b[u]);
            if (q < groups && lane == 0) {
                bits[map_swizzle(2 * q, shift)] = (uint32_t)mask;
                bits[map_swizzle(2 * q + 1, shift)] = (uint32_t)(mask >> 32);
            }
        }
    }
}

// The two-plane pack: voxels first .. first + 64 groups - 1 of a grid of g3 voxels, bit i = voxel first + i, plane p =
// pred(class, p); every voxel is read once.  A voxel past the end of the grid has the class `outside`.
//   !kWindow: a whole grid, first = 0, word w of a plane kept at map_swizzle(w, shift).
//   kWindow: any run of voxels -- first may be negative, and `outside` holds below the grid too -- with word w kept at w (a reader
//     that walks consecutive words needs no swizzle).
template <bool kF32, int kWaves, bool kWindow, typename Pred>
__device__ __forceinline__ void map_pack(const void *__restrict__ tri, int g3, int first, int groups, int outside, int shift,
                                         uint32_t *plane0, uint32_t *plane1, Pred pred)
{
    constexpr int kUnroll = GNBV_MAP_PACK_UNROLL;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int q0 = wave; q0 < groups; q0 += kWaves * kUnroll) {
        int cls[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vox = first + (q0 + u * kWaves) * kWave + lane;
            const int at = min(kWindow ? max(vox, 0) : vox, g3 - 1);
            const int c = voxel_class<kF32>(tri, at);  // (the load is unconditional and clamped, as above)
            cls[u] = ((!kWindow || vox >= 0) && vox < g3) ? c : outside;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int q = q0 + u * kWaves;
            const unsigned long long m0 = __ballot(pred(cls[u], 0)), m1 = __ballot(pred(cls[u], 1));
            if (q < groups && lane == 0) {
                const int w0 = kWindow ? 2 * q : map_swizzle(2 * q, shift), w1 = kWindow ? 2 * q + 1 : map_swizzle(2 * q + 1, shift);
                plane0[w0] = (uint32_t)m0;
                plane0[w1] = (uint32_t)(m0 >> 32);
                plane1[w0] = (uint32_t)m1;
                plane1[w1] = (uint32_t)(m1 >> 32);
            }
        }
    }
}

// one env's whole G^3 grid as two swizzled planes, "occupied" and "unknown"
template <bool kF32, int kWaves>
__device__ __forceinline__ void map_pack_planes(const void *__restrict__ tri, int g, int shift, uint32_t *occ, uint32_t *unk)
{
    const int g3 = g * g * g;
    map_pack<kF32, kWaves, false>(tri, g3, 0, (g3 + kWave - 1) / kWave, -1, shift, occ, unk,
                                  [](int cls, int p) { return p == 0 ? cls > 0 : cls == 0; });
}

// a window of the grid (frontier.hip: a slab of x-planes with its halo) as two plain planes, "free" and "unknown": `words` (even:
// whole ballots) words of each, bit i = voxel first + i.  A bit past either end of the grid is clear in both planes, neither free
// nor unknown: the class of the outside is "occupied".
template <bool kF32, int kWaves>
__device__ __forceinline__ void map_pack_window(const void *__restrict__ tri, int g3, int first, int words, uint32_t *fre, uint32_t *unk)
{
    map_pack<kF32, kWaves, true>(tri, g3, first, words / 2, 1, 0, fre, unk, [](int cls, int p) { return p == 0 ? cls < 0 : cls == 0; });
}

// ---- host: the front end of the entry points -------------------------------------------------------------------------------

struct MapGrid {
    const void *base;   // env e's grid starts at base + e * row_bytes
    int64_t row_bytes;
    bool f32;           // fp32 values (the grid slice of an observation row), else int8
};

// exactly one of the two grid forms, 1 <= g <= kMapMaxGrid, rows of at least G^3 elements
static inline int map_grid(const int8_t *tri_i8, int64_t tri_i8_row_stride, const float *tri_f32, int64_t tri_f32_row_stride, int g,
                           MapGrid *grid)
{
    GNBV_CHECK_ARG((tri_i8 != nullptr) != (tri_f32 != nullptr));
    GNBV_CHECK_ARG(g >= 1 && g <= kMapMaxGrid);
    const bool f32 = tri_f32 != nullptr;
    GNBV_CHECK_ARG((f32 ? tri_f32_row_stride : tri_i8_row_stride) >= (int64_t)g * g * g);
    grid->base = f32 ? static_cast<const void *>(tri_f32) : static_cast<const void *>(tri_i8);
    grid->row_bytes = f32 ? 4 * tri_f32_row_stride : tri_i8_row_stride;
    grid->f32 = f32;
    return 0;
}

// f(kLds, kF32) with the two as std::bool_constant values: `decltype(kLds)::value` is a template argument
template <typename F>
int map_dispatch(bool lds, bool f32, F &&f)
{
    if (lds) return f32 ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return f32 ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// The workgroups of an env that has `items` pieces of work, `turn` of which a workgroup takes at a time: one turn per workgroup
// where the grid is read in place; with the bits in LDS every workgroup pays for packing the whole grid, so an env gets only as
// many workgroups as it takes to reach about two per CU (512) over all n envs.  The items are then dealt evenly.
struct MapChunks {
    int chunks, per;  // workgroups per env; items per workgroup
};

static inline MapChunks map_chunks(int64_t items, int turn, int n, bool lds)
{
    int64_t chunks = (items + turn - 1) / turn;
    if (lds) chunks = std::min<int64_t>(chunks, std::max<int64_t>(1, (512 + n - 1) / n));
    const int64_t per = (items + chunks - 1) / chunks;
    return {(int)((items + per - 1) / per), (int)per};
}

// a flight lattice: 1..1024 nodes per axis, finite lo and h, h > 0 on every axis that has more than one node
static inline bool lattice_ok(int nx, int ny, int nz, const double *lo, const double *h)
{
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        if (n[a] < 1 || n[a] > 1024 || !std::isfinite(lo[a]) || !std::isfinite(h[a])) return false;
        if (n[a] > 1 && !(h[a] > 0.0)) return false;
    }
    return true;
}

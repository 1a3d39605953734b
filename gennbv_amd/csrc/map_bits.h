// map_bits.h -- "this voxel blocks" of a tri-class grid (< 0 free, 0 unknown, > 0 occupied), read in place or packed into one bit
// per voxel in LDS.  Shared by the free set of the flight lattice (flightmap.hip) and the swept sphere on the map (sweepmap.hip):
// one pack, one swizzle, one LDS limit; nothing here may be restated elsewhere.  gnbv_flight_classify_tri keeps two such planes,
// "occupied" and "unknown" (map_pack_planes, map_planes_max_grid).
//
// The packed form: voxel (x G + y) G + z is bit (vox & 31) of word vox >> 5, 64 voxels per wave ballot.  Lanes of a wave that read
// x-neighbours touch words G^2 / 32 apart -- at G = 64 all on one bank -- so word w is kept at w ^ ((w >> shift) & 31),
// shift ~ log2(G^2 / 32), >= 5: a permutation inside each aligned group of 32 words that spreads x-neighbours over the banks.
#pragma once

#include <stddef.h>

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

constexpr int map_lds_max_grid()
{
    int g = 1;
    while (g < kMapMaxGrid && map_lds_bytes(g + 1) <= (size_t)kMapLdsBytes) ++g;
    return g;
}

// the swizzle's shift for a G^3 grid: ~ round(log2(G^2 / 32)), at least 5
static inline int map_swizzle_shift(int g)
{
    int shift = 5;
    while (shift < 20 && (2 << shift) * 3 <= (g * g / 32) * 4) ++shift;
    return shift;
}

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

// two planes of the packed form, "occupied" then "unknown", each map_lds_bytes(g) long (whole groups of 32 words: the swizzle of a
// plane stays inside it)
constexpr int map_planes_max_grid()
{
    int g = 1;
    while (g < kMapMaxGrid && 2 * map_lds_bytes(g + 1) <= (size_t)kMapLdsBytes) ++g;
    return g;
}

__device__ __forceinline__ int map_swizzle(int w, int shift) { return w ^ ((w >> shift) & 31); }

// the whole workgroup (kWaves waves) packs one env's grid into `bits`; the caller synchronises afterwards.  A wave takes
// GNBV_MAP_PACK_UNROLL ballots per turn and issues their loads together: one load per turn leaves the pack waiting for memory
// once per 64 voxels.
#ifndef GNBV_MAP_PACK_UNROLL
#define GNBV_MAP_PACK_UNROLL 8
#endif

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

// map_pack_bits for two planes at once: every voxel is read once, "occupied" goes to occ[], "unknown" to unk[] (the same word
// index and swizzle in both); the caller synchronises afterwards.
template <bool kF32, int kWaves>
__device__ __forceinline__ void map_pack_planes(const void *__restrict__ tri, int g, int shift, uint32_t *occ, uint32_t *unk)
{
    constexpr int kUnroll = GNBV_MAP_PACK_UNROLL;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int g3 = g * g * g, groups = (g3 + kWave - 1) / kWave;
    for (int q0 = wave; q0 < groups; q0 += kWaves * kUnroll) {
        int cls[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vox = (q0 + u * kWaves) * kWave + lane;
            const int c = voxel_class<kF32>(tri, min(vox, g3 - 1));  // (the load is unconditional, as above)
            cls[u] = vox < g3 ? c : -1;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int q = q0 + u * kWaves;
            const unsigned long long mo = __ballot(cls[u] > 0), mu = __ballot(cls[u] == 0);
            if (q < groups && lane == 0) {
                const int w0 = map_swizzle(2 * q, shift), w1 = map_swizzle(2 * q + 1, shift);
                occ[w0] = (uint32_t)mo;
                occ[w1] = (uint32_t)(mo >> 32);
                unk[w0] = (uint32_t)mu;
                unk[w1] = (uint32_t)(mu >> 32);
            }
        }
    }
}

// map_pack_planes for a window of the grid (frontier.hip: a slab of x-planes with its halo), planes "free" then "unknown": bit i of
// the window is voxel first + i -- the voxel order is the memory order, so a run of x-planes is one run of bits -- and a bit past
// either end of the grid (first may be negative) is clear in both planes: neither free nor unknown.  `words` (even: whole
// ballots) words of each plane are written, unswizzled: the reader walks consecutive words.  The caller synchronises afterwards.
template <bool kF32, int kWaves>
__device__ __forceinline__ void map_pack_window(const void *__restrict__ tri, int g3, int first, int words, uint32_t *fre, uint32_t *unk)
{
    constexpr int kUnroll = GNBV_MAP_PACK_UNROLL;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int groups = words / 2;
    for (int q0 = wave; q0 < groups; q0 += kWaves * kUnroll) {
        int cls[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vox = first + (q0 + u * kWaves) * kWave + lane;
            const int c = voxel_class<kF32>(tri, min(max(vox, 0), g3 - 1));  // (the load is unconditional, as above)
            cls[u] = (vox >= 0 && vox < g3) ? c : 1;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int q = q0 + u * kWaves;
            const unsigned long long mf = __ballot(cls[u] < 0), mu = __ballot(cls[u] == 0);
            if (q < groups && lane == 0) {
                fre[2 * q] = (uint32_t)mf;
                fre[2 * q + 1] = (uint32_t)(mf >> 32);
                unk[2 * q] = (uint32_t)mu;
                unk[2 * q + 1] = (uint32_t)(mu >> 32);
            }
        }
    }
}

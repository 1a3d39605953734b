// view_kernels.h -- what the candidate-view kernels share (viewgain.hip, viewcover.hip): "what would the camera see from
// candidate pose j", workgroup (env, chunk of candidates), one ray per lane.  The pixel lattice, the rules for candidates per
// workgroup and lanes, the LDS raise, the camera batch, the 2-bit class lookup and first-to-set.  The block sum and the XCD-aware
// block decode are in common.h.
#pragma once

#include "common.h"
#include "raytrace.h"  // camera_of_pose: k_render_camera's arithmetic (fp64 trig rounded to fp32, roll ignored)

constexpr int kViewMaxThreads = 1024;
constexpr int kCamBatch = 16;  // camera matrices built at a time

// ---- the pixel lattice u = s/2 + i s < w, v = s/2 + j s < h; ray r is (iu, iv) = (r % nu, r / nu)
struct ViewLattice {
    int nu, nv, nrays;
};

inline ViewLattice view_lattice(int h, int w, int stride)
{
    const int half = stride / 2;
    ViewLattice l;
    l.nu = half < w ? (w - half + stride - 1) / stride : 0;
    l.nv = half < h ? (h - half + stride - 1) / stride : 0;
    l.nrays = l.nu * l.nv;
    return l;
}

__device__ __forceinline__ int lattice_pixel(int i, int stride) { return stride / 2 + i * stride; }

// ---- candidates per workgroup: `requested`, or (0) the fewest chunks per env that give `target` workgroups when one chunk of
// every env makes `per_chunk` of them; clamped to [1, k]
inline int view_chunk(int requested, int k, int target, int per_chunk)
{
    int chunk = requested;
    if (chunk == 0) {
        const int want = (target + per_chunk - 1) / per_chunk;  // chunks per env
        chunk = (k + want - 1) / want;
    }
    return chunk < 1 ? 1 : (chunk > k ? k : chunk);
}

// ---- lanes: one ray per lane, whole waves; a workgroup whose LDS leaves room for several per compute unit stays at 256 lanes
inline int view_threads(int nrays, size_t lds)
{
    const int threads = ((nrays > 0 ? nrays : 1) + kWave - 1) / kWave * kWave, cap = lds > 32 * 1024 ? kViewMaxThreads : 256;
    return threads > cap ? cap : threads;
}

// ---- dynamic LDS above 64 KiB.  Per call: the attribute belongs to the current device's copy of the kernel.  false: the caller
// returns hipGetLastError()
template <typename Kernel>
inline bool view_raise_lds(Kernel kernel, size_t lds)
{
    return lds <= 64 * 1024 ||
           hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

// ---- the camera batch of a workgroup that takes candidates j0 <= j < j1 in turn.  Every thread calls it at the head of
// candidate j's turn and gets j's slot in s_cam.  At slot 0, lane t < kCamBatch builds the camera of candidate j + t from
// poses [k, 6] of the env (camera_of_pose; -ffp-contract=off) and calls extra(t, j + t, pose, matrix).  The caller owes two
// barriers: one after the call, before s_cam[slot] is read, and one after the last read of candidate j's turn, which frees the
// slots for the next batch's builders.
template <typename Extra>
__device__ __forceinline__ int camera_batch(float (*s_cam)[16], const float *poses, int j0, int j, int j1, Extra &&extra)
{
    const int slot = (j - j0) % kCamBatch, t = threadIdx.x;
    if (slot == 0 && t < kCamBatch && j + t < j1) {
        const float *q = poses + (size_t)(j + t) * 6;
        camera_of_pose(q, s_cam[t]);
        extra(t, j + t, q, s_cam[t]);
    }
    return slot;
}

// ---- class of voxel `lin` in a grid packed to 2 bits per voxel: unknown 0, occupied 1, free 3
__device__ __forceinline__ uint32_t grid_class(const uint32_t *words, int lin) { return (words[lin >> 4] >> ((lin & 15) * 2)) & 3u; }

// ---- set bit `bit` of a visited mask; whether this lane was the first to set it (atomicOr returns the old word)
__device__ __forceinline__ bool mark_first(uint32_t *mask, int bit)
{
    const uint32_t b = 1u << (bit & 31);
    return (atomicOr(&mask[bit >> 5], b) & b) == 0u;
}

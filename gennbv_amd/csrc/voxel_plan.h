// voxel_plan.h -- the launch plan of the voxel update (voxel.hip), as plain host C++17 without any HIP include: the launch
// constants the kernels and the host share, the workspace layout in numbers, which mask kernels a call runs (voxel_mask_plan)
// and how many voxels a lane of the grid update takes.  voxel.hip's host side only carries a plan out; tests/voxel_plan_dump.cpp
// compiles this header alone with a host compiler and prints plans, so the CPU suite checks the decisions the library makes.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- launch constants ----
constexpr int kHitThreads = 256;       // k_hit_mask
constexpr int kRayThreads = 1024;      // k_raycast
constexpr int kRayWordsPerLane = 8;
constexpr int kRayChunkWords = kRayThreads * kRayWordsPerLane;
constexpr int kQueueCap = 4096;        // k_raycast: targets per round (16 KiB of LDS)
#ifndef FUSED_THREADS
#define FUSED_THREADS 1024
#endif
constexpr int kFusedThreads = FUSED_THREADS;  // k_hit_list, k_hit_atomic
constexpr int kListThreads = 384;    // k_ray_list: rays per work item = lanes per workgroup (four workgroups of six waves per CU: their
                                     // 32 KiB masks are what limits the residency; 256 / 320 / 512 measured within 8 %, profiles/r05_notes.md)
constexpr int kListGridSlices = 5;   // k_ray_list: grid = this many workgroups per env on average
constexpr int kSlabThreads = 256;    // k_ray_slab: rays per slice
constexpr int kListSlices = 16;      // k_ray_slab: slices per env and slab at most
constexpr int kQueueCapPx = 2048;    // undecided pixels of the predictor per workgroup (LDS queue)
constexpr int kGridThreads = 256;    // k_grid_update*
// LDS staging of the masks: a gfx950 workgroup may use all 160 KiB.  Larger masks (G > 104) are split into windows of
// <= 128 KiB, one workgroup per window.
constexpr size_t kVoxelLdsMax = 160 * 1024;
constexpr size_t kVoxelWindowBytes = 128 * 1024;

// ---- workspace layout: [hit masks | path masks | ray counts | ray lists], the last two only in the h/w-sized workspace ----
static inline int mask_words(int g) { return (int)(((int64_t)g * g * g + 31) / 32); }
// words rounded so that every env's mask starts 256-byte aligned
static inline int mask_words_padded(int g) { return (mask_words(g) + 63) & ~63; }
// ray counts [n], padded to 64 ints, directly behind the masks: one fill zeroes masks + counts
static inline size_t ray_count_ints(int n) { return ((size_t)n + 63) & ~(size_t)63; }
// an env lists one ray per distinct voxel and chunk: never more than its pixels
static inline int64_t ray_list_cap(int g, int h, int w) { return ((int64_t)h * w + 63) & ~(int64_t)63; }

static inline size_t voxel_workspace_bytes(int n, int g)
{
    if (n <= 0 || g <= 0) return 0;
    return (size_t)2 * n * mask_words_padded(g) * sizeof(uint32_t);
}

static inline size_t voxel_workspace_bytes_hw(int n, int g, int h, int w)
{
    if (n <= 0 || g <= 0 || h <= 0 || w <= 0) return 0;
    return voxel_workspace_bytes(n, g) + (ray_count_ints(n) + (size_t)n * (size_t)ray_list_cap(g, h, w)) * sizeof(int32_t);
}

// ---- launches 1 + 2: hit mask and path mask of every env ----
enum class VoxelRegime {
    LIST,    // k_hit_list + k_ray_list: hit mask + ray list, then the load-balanced ray cast over the lists (G <= 93)
    LARGE,   // k_hit_atomic + k_ray_slab: the mask does not fit a workgroup's LDS next to its lists
    ROUND1,  // k_hit_mask + k_raycast: a workspace without ray lists, GENNBV_VOXEL_LARGE=0, or no slab that fits the LDS
};

struct VoxelMaskPlan {
    VoxelRegime regime;
    int words;                      // of one env's mask
    int env_groups;                 // every launch has env_groups * 8 * (workgroups per env) workgroups
    int fchunks, chunks, splits;    // workgroups per env of k_hit_list / k_hit_atomic, of k_hit_mask, of k_raycast (and window)
    int hit_windows, path_windows;  // ROUND1: windows of k_hit_mask / k_raycast (> 1: the <*, true> kernels)
    int hit_nw, path_nw;            // words per window
    size_t list_lds, ray_list_lds;  // dynamic LDS of k_hit_list, k_ray_list
    size_t hit_lds, path_lds;       // of k_hit_mask, k_raycast
    int slab_align, slab_planes, slabs, slab_slices;  // k_ray_slab (0 unless the call may take LARGE)
    size_t slab_lds;
    int hit_grid, ray_grid;         // workgroups of the regime's first and second launch
    size_t zero_offset, zero_bytes; // span of the workspace to zero in front of the launches.  LIST and LARGE skip it on a workspace
                                    // the previous call left clean (GNBV_VOXEL_WS_CLEAN); ROUND1 always zeroes
    bool zero_coverage;             // coverage_count is zeroed by a fill too (ROUND1; the other kernels store it)
};

// has_lists: the workspace has the h/w-sized ray lists; large_mode: GENNBV_VOXEL_LARGE (-1 unset, 0, 1);
// slab_planes_override: GENNBV_VOXEL_SLAB_PLANES (<= 0: none)
static inline VoxelMaskPlan voxel_mask_plan(int n, int g, int h, int w, bool has_lists, int large_mode, int slab_planes_override)
{
    (void)h; (void)w;
    VoxelMaskPlan p = {};
    const int words = p.words = mask_words_padded(g);
    const size_t mask_bytes = (size_t)words * sizeof(uint32_t);
    const size_t ray_fixed = (kQueueCap + 32) * sizeof(uint32_t);
    p.hit_windows = mask_bytes <= kVoxelLdsMax ? 1 : (int)((mask_bytes + kVoxelWindowBytes - 1) / kVoxelWindowBytes);
    p.path_windows = mask_bytes + ray_fixed <= kVoxelLdsMax ? 1 : (int)((mask_bytes + kVoxelWindowBytes - 1) / kVoxelWindowBytes);
    p.hit_nw = (words + p.hit_windows - 1) / p.hit_windows;
    p.path_nw = (words + p.path_windows - 1) / p.path_windows;
    p.hit_lds = (size_t)p.hit_nw * sizeof(uint32_t);
    p.path_lds = ray_fixed + (size_t)p.path_nw * sizeof(uint32_t);
    // ray-cast workgroups per env: ~4 per CU in total, so that an env with many hit voxels
    // (measured 4x the mean) is spread over several CUs (profiles/r01_notes.md)
    int splits = (1024 + n - 1) / n;
    p.splits = splits < 1 ? 1 : (splits > 8 ? 8 : splits);
    // k_hit_list / k_hit_atomic workgroups per env: two per CU in total (1024 threads each = 32 waves per CU).  (k_hit_list is capped
    // at 80 SGPRs: with the 96 it wanted, the SIMD's 800-entry SGPR file held 7 waves and a second 16-wave workgroup never became
    // resident beside the first -- 512 workgroups ran as two rounds, profiles/r02_notes.md.)
    int fchunks = (512 + n - 1) / n;
    p.fchunks = fchunks < 1 ? 1 : (fchunks > 16 ? 16 : fchunks);
    // k_hit_mask workgroups per env: enough to cover the chip several times
    int chunks = (8 * 256 + n - 1) / n;
    p.chunks = chunks < 1 ? 1 : (chunks > 16 ? 16 : chunks);
    p.env_groups = (n + 7) / 8;
    p.list_lds = mask_bytes + 64 * sizeof(uint32_t) + (size_t)((words + 1) & ~1) * sizeof(uint16_t) + kQueueCapPx * sizeof(int32_t);
    p.ray_list_lds = mask_bytes;
    const size_t path_offset = (size_t)n * mask_bytes, lists_end = 2 * path_offset + ray_count_ints(n) * sizeof(int32_t);

    if (has_lists && p.list_lds <= kVoxelLdsMax && words <= 65536 && large_mode != 1) {
        p.regime = VoxelRegime::LIST;
        p.hit_grid = p.env_groups * 8 * p.fchunks;
        // kListGridSlices workgroups per env on average (an env takes as many as it has slices of kListThreads rays; 256 x 240x320 x
        // 64^3: ~3.5); past that the workgroups take several items
        p.ray_grid = p.env_groups * 8 * kListGridSlices;
        // one fill: [hit (only when OR-accumulated: several chunks) | path | ray counts]
        p.zero_offset = p.fchunks > 1 ? 0 : path_offset;
        p.zero_bytes = lists_end - p.zero_offset;
        return p;
    }
    if (has_lists && large_mode != 0) {
        // slabs of whole x-planes whose first bit is word-aligned, <= 32 KiB of mask each where the grid allows it
        const int64_t gg = (int64_t)g * g;
        int align = 32;
        while (align > 1 && (gg * (align / 2)) % 32 == 0) align /= 2;
        int64_t per = (8192 * 32) / (gg * align);
        int slab_planes = (int)(align * (per < 1 ? 1 : per));
        if (slab_planes_override > 0) slab_planes = ((slab_planes_override + align - 1) / align) * align;
        slab_planes = slab_planes > g ? ((g + align - 1) / align) * align : slab_planes;
        p.slab_align = align;
        p.slab_planes = slab_planes;
        p.slabs = (g + slab_planes - 1) / slab_planes;
        p.slab_lds = (size_t)((slab_planes * gg + 31) / 32) * sizeof(uint32_t);
        int slab_slices = 32 / p.slabs;  // ~32 workgroups per env, at least two per slab
        p.slab_slices = slab_slices < 2 ? 2 : (slab_slices > kListSlices ? kListSlices : slab_slices);
        if (p.slab_lds <= kVoxelLdsMax) {
            p.regime = VoxelRegime::LARGE;
            p.hit_grid = p.env_groups * 8 * p.fchunks;
            p.ray_grid = p.env_groups * 8 * p.slabs * p.slab_slices;
            p.zero_bytes = lists_end;  // hit (OR-accumulated by global atomics) | path | ray counts
            return p;
        }
    }
    p.regime = VoxelRegime::ROUND1;
    p.hit_grid = p.env_groups * 8 * p.chunks * p.hit_windows;
    p.ray_grid = p.env_groups * 8 * p.splits * p.path_windows;
    // the hit masks are OR-accumulated by atomics; the path masks only with several splits (windows write disjoint word ranges)
    p.zero_bytes = (p.splits > 1 ? 2 : 1) * path_offset;
    p.zero_coverage = true;
    return p;
}

// ---- launch 3: the grid update ----
// the float4 kernel of k_grid_update / k_grid_update_packed; ptrs: the kernel's fp32 row pointers ORed together
static inline bool grid_update_vec4(int64_t g3, int64_t tri_row_stride, uintptr_t ptrs)
{
    return (g3 % 4 == 0) && (tri_row_stride % 4 == 0) && ((ptrs & 15) == 0);
}

// voxels per lane of k_grid_update_coded: 16, 4 or 1 (a pointer that is not passed: 0)
static inline int grid_update_vpl(int64_t g3, uintptr_t prob_code, uintptr_t tri_out, int64_t tri_row_stride, uintptr_t tri_i8,
                                  int64_t tri_i8_row_stride)
{
    const bool vec4 = (g3 % 4 == 0) && (tri_out == 0 || ((tri_row_stride % 4 == 0) && ((tri_out & 15) == 0))) && ((prob_code & 3) == 0) &&
                      (tri_i8 == 0 || (((tri_i8 | (uintptr_t)tri_i8_row_stride) & 3) == 0));
    const bool vec16 = tri_out == 0 && (g3 % 16 == 0) && ((prob_code & 15) == 0) && (((tri_i8 | (uintptr_t)tri_i8_row_stride) & 15) == 0);
    return vec16 ? 16 : vec4 ? 4 : 1;
}

static inline int grid_update_blocks(int64_t items, int n)
{
    int bx = (int)((items + kGridThreads - 1) / kGridThreads);
    const int cap = (4096 + n - 1) / n;  // ~16 workgroups per CU in total, grid-stride beyond
    return bx > cap ? cap : bx;
}

// viewgain.hip -- view gain of candidate camera poses against the tri-class grid an env holds now, on MI355X.
//
// "How much would the map change if the camera went to pose p?"  For env e, candidate j (DESIGN.md "View gain and baseline
// policies"; include/gennbv_hip.h gnbv_view_gain has the exact definition): the rays of the pixel lattice (view_kernels.h) end at
// the world point the voxel update would compute for that pixel at depth `range` (pixel_to_world of backproject.h, the canonical
// fp32 chain); source and target voxel are the unclamped pose_to_idx; each ray visits the in-grid voxels of the reference's
// integer Bresenham in order and stops in front of the first occupied one.  Three int32 per candidate: DISTINCT unknown voxels
// visited by any ray, the same over the rays that were stopped, stopped rays.
//
// This file holds what is the view gain's own: the grid packed to 2 bits per voxel, the two visited masks and who stores them,
// the ray record of the slab path, the host front ends.  The walk (set-up, range of steps, step loop) is ray_walk.h's; lattice,
// chunk and lane rules, camera batch, class lookup and first-to-set are view_kernels.h's; block sum and XCD decode common.h's.
//
//   k_view_gain   grids up to 64^3, workgroup (env, chunk of candidates):
//     1. the env's grid is packed into LDS once (unknown 0, occupied 1, free 3: 64 KiB at 64^3) and serves the whole chunk;
//     2. per candidate: the camera batch (plus c2w_out and the source voxel), then one ray per lane: make_walk / run_walk;
//     3. distinct counts from two visited bitmasks in LDS (all rays / stopped rays, 32 KiB each at 64^3): mark_first on unknown
//        voxels only.  A ray marks mask A on its way; a stopped ray walks again into mask B;
//     4. block_sum, lane 0 stores the three integers.  No global atomics, one writer per output: deterministic;
//     5. the workgroup clears both masks (16-byte stores) before the next candidate.
//   k_view_gain<true>   (gnbv_view_gain_masks) keeps the two masks: after step 4 every lane copies 16-byte pieces of s_a / s_b to
//     the candidate's rows of unknown_bits / hit_bits (lane i holds quad i: conflict-free 16-byte LDS reads, 1 KiB of consecutive
//     addresses per wave store), zeroes the row's pad words and clears the LDS words it has just read -- store-and-clear replaces
//     step 5 and also runs for the chunk's last candidate.  The workgroup owns its candidates' rows: no atomics.
//
//   k_vg_prep, k_vg_fate, k_vg_slab   the same integers for grids up to 128^3 (gnbv_view_gain_slab), and in their <true> forms
//     the same two masks (gnbv_view_gain_slab_masks): further down.
//
//   k_view_carve, k_vg_fate_depth, k_vg_carve_slab   the view gain of a MEASURED frame (GnbvViewGain depth_raw != NULL; DESIGN.md
//     "Free space along every ray"): the same bodies compiled with DEPTH.  A ray ends where its pixel's raw depth says
//     (ray_target_depth), a surface-ended ray leaves the line's last step -- its target voxel, where the surface is -- unmarked,
//     and after a candidate's counts every voxel of mask A may be stored as -1 into the caller's carve row (carve_quad: a lane
//     scatters the quads it is about to clear).  Kernels of their own names: the ones above are the code they were.
#include <cmath>
#include <type_traits>

#include "common.h"
#include "backproject.h"
#include "ray_walk.h"
#include "view_kernels.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kMaxGrid = 64;          // LDS: G^3 / 4 (grid) + 2 * G^3 / 8 (masks) bytes = 128 KiB at 64^3
constexpr int kMaxSlabGrid = 128;     // gnbv_view_gain_slab (the ray word keeps x in 8 bits, the step count in 8)

struct VgBase {  // what every kernel here takes; vg_fill fills it from GnbvViewGain
    int k, g, chunk, chunks;
    const int8_t *tri;
    int64_t tri_row_stride;
    int tri_aligned;
    const float *poses, *range_gt, *voxel_size;
    Intrinsics kinv;
    int stride, nu, nrays;
    float range;
    int32_t *gain;
    float *c2w_out;
    int grid_words, mask_words, ablate;
};

struct VgParams : VgBase {
    // k_view_gain<true> only
    uint32_t *unknown_bits, *hit_bits;  // [n, k, words] rows, 16-byte aligned, either may be NULL
    int words;                          // a multiple of 4, >= mask_words
};

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

// word w of a row's 2-bit codes: voxels 16 w .. 16 w + 15 (0 past the row's end)
__device__ __forceinline__ uint32_t pack_word(const int8_t *row, int w, int g3, int aligned)
{
    const int base = w * 16;
    uint32_t code = 0;
    if (aligned && base + 16 <= g3) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + base);
        code = pack_codes4(v.x) | (pack_codes4(v.y) << 8) | (pack_codes4(v.z) << 16) | (pack_codes4(v.w) << 24);
    } else {
        for (int b = 0; b < 16 && base + b < g3; ++b) {
            const int t = (int)row[base + b];
            code |= (t > 0 ? 1u : (t < 0 ? 3u : 0u)) << (2 * b);
        }
    }
    return code;
}

struct VgFrame {  // env e's voxel frame as axis_to_idx takes it
    float rmin[3], v[3];
};

__device__ __forceinline__ VgFrame vg_frame(const VgBase &p, int e)
{
    return {{p.range_gt[e * 6 + 1], p.range_gt[e * 6 + 3], p.range_gt[e * 6 + 5]},
            {p.voxel_size[e * 3 + 0], p.voxel_size[e * 3 + 1], p.voxel_size[e * 3 + 2]}};
}

__device__ __forceinline__ void voxel_of(const float *pt, const VgFrame &f, int *ix)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) ix[a] = axis_to_idx(pt[a], f.rmin[a], f.v[a]);
}

// the end voxel of lattice ray r from the camera M
__device__ __forceinline__ void ray_target(const VgBase &p, const float *M, const VgFrame &f, int r, int *ix)
{
    const int iv = r / p.nu, u = lattice_pixel(r - iv * p.nu, p.stride), v = lattice_pixel(iv, p.stride);
    float wp[3];
    pixel_to_world(p.range, (float)u, (float)v, p.kinv, M, wp);
    voxel_of(wp, f, ix);
}

// The view gain of a MEASURED frame (GnbvViewGain depth_raw != NULL; include/gennbv_hip.h has the rule): a lattice ray ends where
// its pixel's raw depth says, and the voxels it marked may be carved into an int8 row.  Compile-time variants under names of their
// own (k_view_carve, k_vg_fate_depth, k_vg_carve_slab): the kernels without a depth image are the code they were.
struct VgDepth {
    const float *depth;  // candidate j of env e: depth + e env_stride + j cand_stride, [h, w] row-major
    int64_t env_stride, cand_stride;
    float sense;         // the updater's depth_sense_dist (< 0)
    int w;
    int8_t *carve;       // [n, g^3] rows, row stride in bytes, or NULL
    int64_t carve_stride;
};

// the same for a measured ray; returns whether the ray is surface-ended (its target voxel then holds the surface)
__device__ __forceinline__ bool ray_target_depth(const VgBase &p, const VgDepth &d, const float *img, const float *M, const VgFrame &f,
                                                 int r, int *ix)
{
    const int iv = r / p.nu, u = lattice_pixel(r - iv * p.nu, p.stride), v = lattice_pixel(iv, p.stride);
    const float raw = img[(size_t)v * d.w + u], len = fabsf(raw);
    // finite, not +-0, above the clamp (process_depth keeps it) and within range; NaN fails every comparison
    const bool surface = len <= FLT_MAX && raw != 0.0f && raw > d.sense && len <= p.range;
    float wp[3];
    pixel_to_world(surface ? len : p.range, (float)u, (float)v, p.kinv, M, wp);
    voxel_of(wp, f, ix);
    return surface;
}

// row[bit] = -1 for every set bit of a quad of a visited mask; `bit0` is the quad's first bit
__device__ __forceinline__ void carve_quad(int8_t *row, const uint4 &q, int bit0)
{
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int t = 0; t < 4; ++t)
        for (uint32_t m = w[t]; m != 0u; m &= m - 1u) row[bit0 + 32 * t + __builtin_ctz(m)] = (int8_t)-1;
}

__device__ __forceinline__ void clear_quads(uint4 *s, int quads)
{
    for (int w = threadIdx.x; w < quads; w += blockDim.x) s[w] = make_uint4(0u, 0u, 0u, 0u);
}

template <bool MASKS, bool DEPTH>
__device__ __forceinline__ void view_gain_body(const VgParams &p, const VgDepth &d)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    __shared__ float s_cam[kCamBatch][16];
    __shared__ int s_src[kCamBatch][3];
    __shared__ int s_part[kViewMaxThreads / kWave][3];

    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int e = blockIdx.x / p.chunks, ch = blockIdx.x - e * p.chunks;
    const int j0 = ch * p.chunk, j1 = min(p.k, j0 + p.chunk);
    const int g = p.g, g3 = g * g * g;
    uint32_t *s_grid = s_mem, *s_a = s_mem + p.grid_words, *s_b = s_a + p.mask_words;

    // ---- 1. the env's grid, 2 bits per voxel
    const int8_t *row = p.tri + (size_t)e * p.tri_row_stride;
    for (int w = tid; w < p.grid_words; w += nthreads) s_grid[w] = pack_word(row, w, g3, p.tri_aligned);
    uint4 *s_masks4 = reinterpret_cast<uint4 *>(s_a);
    const int row_quads = p.mask_words / 4;  // of one mask (mask_words is a multiple of 4)
    clear_quads(s_masks4, 2 * row_quads);

    const VgFrame f = vg_frame(p, e);
    const bool mark = (p.ablate & 1) == 0, second = (p.ablate & 2) == 0;

    for (int j = j0; j < j1; ++j) {
        // ---- 2a. the camera batch, with c2w_out and the source voxel
        const int slot = camera_batch(s_cam, p.poses + (size_t)e * p.k * 6, j0, j, j1, [&](int t, int jt, const float *q, const float *m) {
            if (p.c2w_out != nullptr) {
                float *o = p.c2w_out + ((size_t)e * p.k + jt) * 16;
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i] = m[i];
            }
            voxel_of(q, f, s_src[t]);
        });
        __syncthreads();  // cameras ready; masks clear

        // ---- 2b / 3. one ray per lane
        const int x0 = s_src[slot][0], y0 = s_src[slot][1], z0 = s_src[slot][2];
        int cnt[3] = {0, 0, 0};  // unknown voxels, those of the stopped rays, stopped rays
        const float *img = nullptr;
        if constexpr (DEPTH) img = d.depth + (size_t)e * d.env_stride + (size_t)j * d.cand_stride;
        for (int r = tid; r < p.nrays; r += nthreads) {
            int t[3];
            bool surface = false;
            if constexpr (DEPTH) surface = ray_target_depth(p, d, img, s_cam[slot], f, r, t);
            else ray_target(p, s_cam[slot], f, r, t);
            const RayWalk rw = make_walk(x0, y0, z0, t[0], t[1], t[2], g);
            if (rw.n == 0) continue;
            const int skip = surface ? (rw.two_da >> 1) - rw.i0 : -1;  // the line's last step is the target voxel: a surface is there
            auto walk_into = [&](uint32_t *mask, int &count, bool marking) {
                return run_walk(rw, g, [&](int lin, int i) {
                    const uint32_t cls = grid_class(s_grid, lin);
                    if (cls == 1u) return true;
                    if (DEPTH && i == skip) return false;
                    if (cls == 0u && marking) count += mark_first(mask, lin);
                    return false;
                });
            };
            if (walk_into(s_a, cnt[0], mark)) {
                ++cnt[2];
                if (mark && second) walk_into(s_b, cnt[1], true);
            }
        }

        // ---- 4. the three sums.  block_sum's barrier: every ray of candidate j is done, masks and camera slot free
        block_sum(cnt, s_part);
        if (tid == 0) {
            int32_t *o = p.gain + ((size_t)e * p.k + j) * 3;
            o[0] = cnt[0]; o[1] = cnt[1]; o[2] = cnt[2];
        }
        // ---- 4b. carve: every voxel of mask A becomes free in the caller's row.  A lane reads the quads it clears in step 5.
        //          With carve == tri (k == 1: this workgroup owns the env) the row was packed in step 1, two barriers ago
        if constexpr (DEPTH) {
            if (d.carve != nullptr) {
                int8_t *crow = d.carve + (size_t)e * d.carve_stride;
                for (int q = tid; q < row_quads; q += nthreads) carve_quad(crow, s_masks4[q], 128 * q);
            }
        }
        // ---- 5. clear the masks for the next candidate (ordered in front of its rays by the barrier at the loop's head, which
        //         also is the barrier block_sum leaves to its caller)
        if constexpr (MASKS) {
            // store, then clear: a lane clears the quads it stored, so no barrier between the two.  Every word of the row is
            // written: mask_words from LDS (the bits at and past g^3 were never set), zeros from there to `words`.
            const size_t off = ((size_t)e * p.k + j) * (size_t)p.words;
            uint4 *ga = p.unknown_bits != nullptr ? reinterpret_cast<uint4 *>(p.unknown_bits + off) : nullptr;
            uint4 *gb = p.hit_bits != nullptr ? reinterpret_cast<uint4 *>(p.hit_bits + off) : nullptr;
            const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
            for (int w = tid; w < p.words / 4; w += nthreads) {
                if (w < row_quads) {
                    if (ga != nullptr) ga[w] = s_masks4[w];
                    if (gb != nullptr) gb[w] = s_masks4[row_quads + w];
                    s_masks4[w] = zero;
                    s_masks4[row_quads + w] = zero;
                } else {
                    if (ga != nullptr) ga[w] = zero;
                    if (gb != nullptr) gb[w] = zero;
                }
            }
        } else {
            if (j + 1 < j1 && mark) clear_quads(s_masks4, 2 * row_quads);
        }
    }
}

template <bool MASKS>
__global__ __launch_bounds__(kViewMaxThreads) void k_view_gain(VgParams p)
{
    view_gain_body<MASKS, false>(p, VgDepth{});
}

template <bool MASKS>
__global__ __launch_bounds__(kViewMaxThreads) void k_view_carve(VgParams p, VgDepth d)
{
    view_gain_body<MASKS, true>(p, d);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Grids above 64^3 (gnbv_view_gain_slab): the grid and its masks no longer fit in LDS, so a candidate's voxels are split into
// slabs of x-planes and a ray is known by its FATE before any slab sees it.  Per batch of envs (the workspace holds one batch):
//
//   k_vg_prep   the batch's grids packed to 2 bits per voxel in global memory (512 KiB per env at 128^3: an env's workgroups
//               run on one XCD, whose L2 keeps it), the camera matrix and source voxel of every candidate, gain zeroed;
//   k_vg_fate   one ray per lane, workgroup (env, candidate, 256 rays): the ray's end voxel, then k_view_gain's walk against
//               the packed grid, read-only.  Per ray a 16-byte record {end voxel, first in-grid step} and a 4-byte word
//               {steps to mark, blocked, the x-extent of those steps}: the steps run from the first in-grid voxel to the one
//               in front of the first occupied voxel (the in-grid steps of a line are contiguous: the grid is convex).
//               `blocked` is complete after this pass (one atomicAdd per workgroup);
//   k_vg_slab   workgroup (env, chunk of candidates, slab [X0, X1)): the slab's part of the packed grid and of both visited
//               masks in LDS ((X1 - X0) G^2 / 2 bytes).  A ray whose marked x-extent misses the slab is rejected on its
//               4-byte word alone.  Otherwise its recorded steps are cut to the slab (ray_walk.h make_slab_cut) and walked
//               once with a test of the slab-local index: mask A, and mask B too if it is blocked.  Distinct counts as in
//               k_view_gain; the slabs partition the voxels by x, so a candidate's counts are the sums over its slabs: int32
//               atomicAdd, one per workgroup, candidate and count -- integer sums, the same bits in any order.
//
// tests/test_ray_walk_host_cpu.py runs the record and the slab cut of ray_walk.h itself on the CPU against the oracle's
// Bresenham; tests/test_view_gain_slab_cpu.py holds a Python model of both (and of the 32-bit bound).
//
// gnbv_view_gain_slab_masks launches k_vg_prep<true> and k_vg_slab<true>, which also keep the two masks (k_vg_fate is shared).
// A candidate's row is cut by x-planes like its voxels: slab [X0, X1) holds the row's bits [X0 G^2, X1 G^2), which start and
// end inside a word unless G^2 s is a multiple of 32.
//   - The slab's LDS masks are biased by sh = X0 G^2 & 127: voxel `lin` of the slab is bit lin + sh, so LDS quad q IS row quad
//     (X0 G^2 >> 7) + q -- a 16-byte LDS read and an aligned 16-byte global store, no funnel shift.  Cost: at most 16 bytes per
//     mask, and none where G^2 s is a multiple of 128 (any s at G % 16 == 0, even s at G % 8 == 0).  s_grid and the counts
//     do not see sh.
//   - After block_sum's barrier a lane stores the quads it then clears (store-and-clear replaces the clear pass and also runs
//     for the chunk's last candidate).  A quad that lies whole inside the slab's bits (the last slab owns the row up to its last
//     quad: bits at and past G^3 are never set) is one 16-byte store.  In the at most two quads at the slab's ragged ends a word
//     inside the slab's bits is a 4-byte store, a word of another slab is left alone, and a word the slab SHARES with a neighbour
//     gets the slab's part by a global atomicOr.  The parts are disjoint bit sets and k_vg_prep<true> has zeroed the shared words
//     (and the pad words from ceil(G^3 / 32) to `words`) earlier on the stream, so the word does not depend on the order.  Every
//     other word of a row has one writer.  G^2 >= 32 bits per plane from G = 6 on, so a word is then shared by two slabs at most
//     (at G = 3, s = 1 by three; the rule is the same).  k_view_gain<true>'s store-and-clear is the case X0 = 0, X1 = G of this
//     one and stays apart: written through one shared function that kernel needs 97 VGPRs, one wave per SIMD fewer.
//   - With no ray (stride / 2 >= width or height) no slab kernel runs and k_vg_prep<true> zeroes the rows whole.
// tests/test_gain_masks_slab_cpu.py holds a numpy model of this word-ownership rule.
constexpr int kFateThreads = 256;
constexpr int kCamWords = 20;                      // per candidate in the workspace: c2w [16] f32, source voxel [3] i32, pad
constexpr size_t kSlabLdsBudget = 128 * 1024;      // default slab height: grid + masks within this
constexpr size_t kSlabLdsMax = 160 * 1024 - 256;   // a requested height is reduced to fit (static LDS: 128 B)
constexpr size_t kBatchBytes = (size_t)128 << 20;  // ray records of one batch of envs
constexpr int kSlabWorkgroups = 2560;              // k_vg_slab workgroups per batch the default chunk aims at

struct VsParams : VgBase {
    int slab, nslab, rblocks, pack_words;
    uint32_t *packed;  // [batch, pack_words]
    float *cams;       // [batch, k, kCamWords]
    int4 *rec;         // [batch, k, nrays]
    uint32_t *meta;    // [batch, k, nrays]
};

struct VsMaskParams : VsParams {        // k_vg_prep<true>, k_vg_slab<true>
    uint32_t *unknown_bits, *hit_bits;  // [n, k, words] rows, 16-byte aligned, either may be NULL
    int words;                          // a multiple of 4, >= ceil(g^3 / 32)
    int zero_words;                     // words of a row k_vg_prep<true> zeroes: nslab - 1 seams + the pad, or (zero_all, no
    int zero_all;                       // slab kernel follows) all `words`
};
template <bool MASKS> using VsArgs = std::conditional_t<MASKS, VsMaskParams, VsParams>;

template <bool MASKS>
__global__ __launch_bounds__(256) void k_vg_prep(VsArgs<MASKS> p, int e0, int ne)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int g3 = p.g * p.g * p.g;
    if constexpr (MASKS) {
        // the words no slab workgroup plain-stores: the word at each seam that is not a word boundary (the slabs OR their
        // parts into it), the pad words; with no ray, the whole row
        if (t < (int64_t)ne * p.k * p.zero_words) {
            const int64_t c = t / p.zero_words;  // (el, j)
            const int z = (int)(t - c * p.zero_words), row_words = (g3 + 31) / 32;
            int w = z;
            if (!p.zero_all && z < p.nslab - 1) {
                const int seam = (z + 1) * p.slab * p.g * p.g;  // the first bit of slab z + 1
                w = (seam & 31) != 0 ? seam >> 5 : -1;
            } else if (!p.zero_all) {
                w = row_words + (z - (p.nslab - 1));
            }
            if (w >= 0) {
                const size_t o = ((size_t)e0 * p.k + (size_t)c) * (size_t)p.words + w;
                if (p.unknown_bits != nullptr) p.unknown_bits[o] = 0u;
                if (p.hit_bits != nullptr) p.hit_bits[o] = 0u;
            }
        }
    }
    if (t < (int64_t)ne * p.pack_words) {
        const int el = (int)(t / p.pack_words), w = (int)(t - (int64_t)el * p.pack_words);
        p.packed[t] = pack_word(p.tri + (size_t)(e0 + el) * p.tri_row_stride, w, g3, p.tri_aligned);
    }
    if (t < (int64_t)ne * p.k * 3) p.gain[(size_t)e0 * p.k * 3 + t] = 0;
    if (t < (int64_t)ne * p.k) {
        const int el = (int)(t / p.k), e = e0 + el;
        const size_t c = (size_t)e0 * p.k + t;  // (e, j) over all envs
        const float *q = p.poses + c * 6;
        float m[16];
        camera_of_pose(q, m);
        float *o = p.cams + (size_t)t * kCamWords;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = m[i];
        if (p.c2w_out != nullptr) {
#pragma unroll
            for (int i = 0; i < 16; ++i) p.c2w_out[c * 16 + i] = m[i];
        }
        int *src = reinterpret_cast<int *>(o + 16);
        voxel_of(q, vg_frame(p, e), src);
        src[3] = 0;
    }
}

template <bool DEPTH>
__device__ __forceinline__ void vg_fate_body(const VsParams &p, const VgDepth &d, int e0, int ne)
{
    __shared__ int s_part[kFateThreads / kWave][1];
    int rem;  // (candidate, ray block)
    const int el = xcd_env(p.k * p.rblocks, rem);
    if (el >= ne) return;
    const int j = rem / p.rblocks, rb = rem - j * p.rblocks;
    const int e = e0 + el, tid = threadIdx.x, g = p.g;
    const size_t cj = (size_t)el * p.k + j;
    const float *M = p.cams + cj * kCamWords;
    const int *src = reinterpret_cast<const int *>(M + 16);
    const uint32_t *G = p.packed + (size_t)el * p.pack_words;
    const int r = rb * kFateThreads + tid;
    int cnt[1] = {0};  // stopped rays
    if (r < p.nrays) {
        int t[3];
        bool surface = false;
        if constexpr (DEPTH)
            surface = ray_target_depth(p, d, d.depth + (size_t)e * d.env_stride + (size_t)j * d.cand_stride, M, vg_frame(p, e), r, t);
        else ray_target(p, M, vg_frame(p, e), r, t);
        const RayWalk rw = make_walk(src[0], src[1], src[2], t[0], t[1], t[2], g);
        // a surface-ended ray leaves its target voxel, the line's last step, out of the record (a surface is there): the
        // recorded steps stay contiguous and k_vg_slab needs no word of it
        const int skip = surface && rw.n > 0 ? (rw.two_da >> 1) - rw.i0 : -1;
        int first = 0, last = -1, lin_first = 0, lin_last = 0;
        bool blocked = false;
        if (rw.n > 0)
            blocked = run_walk(rw, g, [&](int lin, int i) {
                if (grid_class(G, lin) == 1u) return true;
                if (DEPTH && i == skip) return false;
                if (last < 0) { first = i; lin_first = lin; }
                last = i; lin_last = lin;
                return false;
            });
        cnt[0] = blocked ? 1 : 0;
        const int count = last < 0 ? 0 : last - first + 1;  // <= g
        const int gg = g * g, xf = lin_first / gg, xl = lin_last / gg;
        p.rec[cj * p.nrays + r] = make_int4(t[0], t[1], t[2], rw.n > 0 ? rw.i0 + first : 0);
        p.meta[cj * p.nrays + r] = (uint32_t)count | (blocked ? 256u : 0u) | ((uint32_t)min(xf, xl) << 16) | ((uint32_t)max(xf, xl) << 24);
    }
    block_sum(cnt, s_part);
    if (tid == 0 && cnt[0] != 0) atomicAdd(p.gain + ((size_t)e * p.k + j) * 3 + 2, cnt[0]);
}

__global__ __launch_bounds__(kFateThreads) void k_vg_fate(VsParams p, int e0, int ne)
{
    vg_fate_body<false>(p, VgDepth{}, e0, ne);
}

__global__ __launch_bounds__(kFateThreads) void k_vg_fate_depth(VsParams p, VgDepth d, int e0, int ne)
{
    vg_fate_body<true>(p, d, e0, ne);
}

template <bool MASKS, bool DEPTH>
__device__ __forceinline__ void vg_slab_body(const VsArgs<MASKS> &p, const VgDepth &d, int e0, int ne)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    __shared__ int s_part[kViewMaxThreads / kWave][2];

    const int tid = threadIdx.x, nthreads = blockDim.x;
    int rem;  // (chunk, slab)
    const int el = xcd_env(p.chunks * p.nslab, rem);
    if (el >= ne) return;
    const int ch = rem / p.nslab, sl = rem - ch * p.nslab;
    const int e = e0 + el, g = p.g, gg = g * g;
    const int j0 = ch * p.chunk, j1 = min(p.k, j0 + p.chunk);
    const int X0 = sl * p.slab, X1 = min(g, X0 + p.slab);
    const unsigned svox = (unsigned)((X1 - X0) * gg);
    const int sh = MASKS ? (X0 * gg) & 127 : 0;  // <true>: voxel `lin` of the slab is bit lin + sh of the LDS masks
    uint32_t *s_grid = s_mem, *s_a = s_mem + p.grid_words, *s_b = s_a + p.mask_words;

    // ---- the slab's voxels, 2 bits each, from voxel X0 g^2 of the packed grid (not a word boundary in general; the packed
    //      row ends with a spare word, and the bits past the slab's last voxel are never looked at)
    const uint32_t *G = p.packed + (size_t)el * p.pack_words;
    for (int w = tid; w < (int)((svox + 15) / 16); w += nthreads) {
        const int off = X0 * gg + 16 * w, gw = off >> 4, sh = (off & 15) * 2;
        s_grid[w] = sh != 0 ? (G[gw] >> sh) | (G[gw + 1] << (32 - sh)) : G[gw];
    }
    uint4 *s_masks4 = reinterpret_cast<uint4 *>(s_a);
    const int row_quads = p.mask_words / 4;
    clear_quads(s_masks4, 2 * row_quads);
    const bool mark = (p.ablate & 1) == 0, second = (p.ablate & 2) == 0;

    for (int j = j0; j < j1; ++j) {
        __syncthreads();  // grid loaded; masks clear
        const size_t cj = (size_t)el * p.k + j;
        const int *src = reinterpret_cast<const int *>(p.cams + cj * kCamWords + 16);
        const int x0 = src[0], y0 = src[1], z0 = src[2];
        const uint32_t *meta = p.meta + cj * p.nrays;
        const int4 *rec = p.rec + cj * p.nrays;
        int cnt[2] = {0, 0};  // unknown voxels, those of the stopped rays
        for (int r = tid; r < p.nrays; r += nthreads) {
            const uint32_t m = meta[r];
            const int count = (int)(m & 255u), xa = (int)((m >> 16) & 255u), xb = (int)(m >> 24);
            if (count == 0 || xb < X0 || xa >= X1) continue;  // nothing to mark, or not in this slab
            const bool blocked = (m & 256u) != 0u && second;
            const int4 q = rec[r];
            const RayWalk w = make_slab_cut(x0, y0, z0, q.x, q.y, q.z, g, q.w, count, X0, X1);
            walk_steps(w, [svox](const RayWalk &s) { return (unsigned)s.lin < svox; }, [&](int lin, int) {
                if (grid_class(s_grid, lin) == 0u && mark) {
                    cnt[0] += mark_first(s_a, lin + sh);
                    if (blocked) cnt[1] += mark_first(s_b, lin + sh);
                }
                return false;
            });
        }
        block_sum(cnt, s_part);  // its barrier: every ray of candidate j is done, masks free
        if (tid == 0) {
            int32_t *o = p.gain + ((size_t)e * p.k + j) * 3;
            if (cnt[0] != 0) atomicAdd(o, cnt[0]);
            if (cnt[1] != 0) atomicAdd(o + 1, cnt[1]);
        }
        // carve: the slab's voxels of mask A (bit lin + sh) become free in the caller's row; a lane reads the quads it clears below
        if constexpr (DEPTH) {
            if (d.carve != nullptr) {
                int8_t *crow = d.carve + (size_t)e * d.carve_stride + (size_t)X0 * gg - sh;
                for (int q = tid; q < (int)((sh + svox + 127) >> 7); q += nthreads) carve_quad(crow, s_masks4[q], 128 * q);
            }
        }
        // (ordered in front of the next candidate's rays by the barrier at the loop's head, as in k_view_gain)
        if constexpr (MASKS) {
            // store, then clear: a lane clears the quads it stored, so no barrier between the two.  The slab's bits are
            // [lo, hi) of the LDS masks; the last slab owns the row to the end of its last quad.
            const int lo = sh, nq = (sh + (int)svox + 127) >> 7, hi = X1 == g ? nq * 128 : sh + (int)svox;
            const size_t off = ((size_t)e * p.k + j) * (size_t)p.words + 4 * (size_t)((X0 * gg) >> 7);
            uint32_t *ga = p.unknown_bits != nullptr ? p.unknown_bits + off : nullptr;
            uint32_t *gb = p.hit_bits != nullptr ? p.hit_bits + off : nullptr;
            const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
            for (int q = tid; q < nq; q += nthreads) {
                const uint4 a = s_masks4[q], c = s_masks4[row_quads + q];
                if (128 * q >= lo && 128 * q + 128 <= hi) {
                    if (ga != nullptr) reinterpret_cast<uint4 *>(ga)[q] = a;
                    if (gb != nullptr) reinterpret_cast<uint4 *>(gb)[q] = c;
                } else {
                    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int b0 = 128 * q + 32 * t, b1 = b0 + 32;
                        if (b1 <= lo || b0 >= hi) continue;  // another slab's word
                        if (b0 >= lo && b1 <= hi) {
                            if (ga != nullptr) ga[4 * q + t] = aw[t];
                            if (gb != nullptr) gb[4 * q + t] = cw[t];
                        } else {  // shared with a neighbour: zeroed by k_vg_prep<true>, the parts are disjoint
                            if (ga != nullptr && aw[t] != 0u) atomicOr(ga + 4 * q + t, aw[t]);
                            if (gb != nullptr && cw[t] != 0u) atomicOr(gb + 4 * q + t, cw[t]);
                        }
                    }
                }
                s_masks4[q] = zero;
                s_masks4[row_quads + q] = zero;
            }
        } else {
            if (j + 1 < j1 && mark) clear_quads(s_masks4, 2 * row_quads);
        }
    }
}

template <bool MASKS>
__global__ __launch_bounds__(kViewMaxThreads) void k_vg_slab(VsArgs<MASKS> p, int e0, int ne)
{
    vg_slab_body<MASKS, false>(p, VgDepth{}, e0, ne);
}

template <bool MASKS>
__global__ __launch_bounds__(kViewMaxThreads) void k_vg_carve_slab(VsArgs<MASKS> p, VgDepth d, int e0, int ne)
{
    vg_slab_body<MASKS, true>(p, d, e0, ne);
}

// what both host entry points of the slab path derive from the sizes
struct VsPlan {
    ViewLattice lat;
    int pack_words, batch;
    size_t off_cams, off_rec, off_meta, bytes;
};

inline bool vs_plan(int n, int k, int g, int h, int w, int stride, VsPlan &pl)
{
    if (!(n > 0 && k > 0 && g >= 2 && g <= kMaxSlabGrid && h > 0 && w > 0 && stride >= 1 && h <= 32768 && w <= 32768)) return false;
    pl.lat = view_lattice(h, w, stride);
    const int g3 = g * g * g, nrays = pl.lat.nrays;
    pl.pack_words = (((g3 + 15) / 16) + 1 + 3) & ~3;  // + 1: k_vg_slab reads one word past an unaligned slab
    // envs per batch: the ray records of a batch stay near kBatchBytes, so that the slab pass finds them in the last-level cache
    const size_t per_env = (size_t)k * (size_t)(nrays > 0 ? nrays : 1) * 20;
    size_t batch = kBatchBytes / per_env;
    batch = batch < 8 ? 8 : batch;
    pl.batch = batch > (size_t)n ? n : (int)batch;
    const size_t bn = (size_t)pl.batch, rays = bn * k * nrays;
    pl.off_cams = align256(bn * pl.pack_words * sizeof(uint32_t));
    pl.off_rec = align256(pl.off_cams + bn * k * kCamWords * sizeof(float));
    pl.off_meta = align256(pl.off_rec + rays * sizeof(int4));
    pl.bytes = align256(pl.off_meta + rays * sizeof(uint32_t));
    return true;
}

// `masks`: k_vg_slab<true> biases its masks by X0 g^2 & 127 bits, which is 0 in every slab where s g^2 is a multiple of 128
inline size_t slab_lds_bytes(int g, int s, int &grid_words, int &mask_words, bool masks = false)
{
    const int vox = s * g * g, bias = masks && (vox & 127) != 0 ? 127 : 0;
    grid_words = (((vox + 15) / 16) + 3) & ~3;
    mask_words = (((vox + bias + 31) / 32) + 3) & ~3;
    return (size_t)(grid_words + 2 * mask_words) * sizeof(uint32_t);
}

bool view_gain_args_ok(const GnbvViewGain &a, int max_grid)
{
    return a.n > 0 && a.k > 0 && a.g >= 2 && a.g <= max_grid && a.h > 0 && a.w > 0 && a.stride >= 1 && a.h <= 32768 && a.w <= 32768 &&
           std::isfinite(a.range) && a.range > 0.0f && a.chunk >= 0 && a.ablate >= 0 && a.ablate <= 3 && a.tri_i8 != nullptr &&
           a.poses != nullptr && a.range_gt != nullptr && a.voxel_size != nullptr && a.inv_intri != nullptr && a.gain != nullptr &&
           a.tri_row_stride >= (int64_t)a.g * a.g * a.g;
}

// the measured-frame fields (depth_raw NULL: only carve_i8 is looked at, and refused).  `lds`: the one-launch kernel, where a
// carve row may be the tri row only with one workgroup per env (k == 1); the slab path packs every grid in a launch of its own
bool depth_args_ok(const GnbvViewGain &a, bool lds)
{
    if (a.depth_raw == nullptr) return a.carve_i8 == nullptr;
    const int64_t hw = (int64_t)a.h * a.w, g3 = (int64_t)a.g * a.g * a.g;
    if (a.depth_env_stride < hw || !(a.depth_cand_stride >= hw || (a.depth_cand_stride == 0 && a.k == 1))) return false;
    if (!(std::isfinite(a.depth_sense_dist) && a.depth_sense_dist < 0.0f)) return false;
    if (a.carve_i8 == nullptr) return true;
    if (a.ablate != 0 || a.carve_row_stride < g3) return false;
    if (a.carve_i8 == a.tri_i8 && a.carve_row_stride == a.tri_row_stride) return !lds || a.k == 1;
    const uintptr_t t0 = (uintptr_t)a.tri_i8, t1 = t0 + (uintptr_t)(a.n - 1) * (uintptr_t)a.tri_row_stride + (uintptr_t)g3;
    const uintptr_t c0 = (uintptr_t)a.carve_i8, c1 = c0 + (uintptr_t)(a.n - 1) * (uintptr_t)a.carve_row_stride + (uintptr_t)g3;
    return c1 <= t0 || t1 <= c0;
}

VgDepth vg_depth(const GnbvViewGain &a)
{
    return {a.depth_raw, a.depth_env_stride, a.depth_cand_stride, a.depth_sense_dist, a.w, a.carve_i8, a.carve_row_stride};
}

// the mask arguments of gnbv_view_gain_masks and gnbv_view_gain_slab_masks
bool mask_args_ok(const GnbvViewGain &a, int words, const int32_t *unknown_bits, const int32_t *hit_bits)
{
    return a.ablate == 0 && (unknown_bits != nullptr || hit_bits != nullptr) && words > 0 && (words & 3) == 0 &&
           words >= (a.g * a.g * a.g + 31) / 32 && (((uintptr_t)unknown_bits | (uintptr_t)hit_bits) & 15) == 0 &&
           (int64_t)a.n * a.k * words <= 0x7fffffff;
}

// the common parameters, but grid_words / mask_words (the LDS layout is the caller's)
void vg_fill(VgBase &p, const GnbvViewGain &a, const ViewLattice &lat, int chunk)
{
    p.k = a.k; p.g = a.g;
    p.chunk = chunk;
    p.chunks = (a.k + chunk - 1) / chunk;
    p.tri = a.tri_i8;
    p.tri_row_stride = a.tri_row_stride;
    p.tri_aligned = (((uintptr_t)a.tri_i8 | (uintptr_t)a.tri_row_stride) & 15) == 0;
    p.poses = a.poses; p.range_gt = a.range_gt; p.voxel_size = a.voxel_size;
    for (int i = 0; i < 9; ++i) p.kinv.k[i] = a.inv_intri[i];
    p.stride = a.stride; p.nu = lat.nu; p.nrays = lat.nrays;
    p.range = a.range;
    p.gain = a.gain;
    p.c2w_out = a.c2w_out;
    p.ablate = a.ablate;
}

// gnbv_view_gain (MASKS false: the mask arguments are not looked at) and gnbv_view_gain_masks
template <bool MASKS>
int view_gain_impl(const GnbvViewGain *args, int words, int32_t *unknown_bits, int32_t *hit_bits, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvViewGain a = *args;
    GNBV_CHECK_ARG(view_gain_args_ok(a, kMaxGrid) && depth_args_ok(a, true));
    if (MASKS) GNBV_CHECK_ARG(mask_args_ok(a, words, unknown_bits, hit_bits));
    VgParams p;
    // candidates per workgroup: enough workgroups for two per compute unit, but the grid is packed once per workgroup
    vg_fill(p, a, view_lattice(a.h, a.w, a.stride), view_chunk(a.chunk, a.k, 512, a.n));
    GNBV_CHECK_ARG((int64_t)a.n * p.chunks <= 0x7fffffff);
    const int g3 = a.g * a.g * a.g;
    p.grid_words = (((g3 + 15) / 16) + 3) & ~3;
    p.mask_words = (((g3 + 31) / 32) + 3) & ~3;
    p.unknown_bits = MASKS ? reinterpret_cast<uint32_t *>(unknown_bits) : nullptr;
    p.hit_bits = MASKS ? reinterpret_cast<uint32_t *>(hit_bits) : nullptr;
    p.words = MASKS ? words : 0;
    const size_t lds = (size_t)(p.grid_words + 2 * p.mask_words) * sizeof(uint32_t);
    const dim3 grid((unsigned)(a.n * p.chunks)), block(view_threads(p.nrays, lds));
    if (a.depth_raw != nullptr) {
        if (!view_raise_lds(k_view_carve<MASKS>, lds)) return (int)hipGetLastError();
        hipLaunchKernelGGL(k_view_carve<MASKS>, grid, block, lds, gnbv_stream(stream), p, vg_depth(a));
        return gnbv_launch_status();
    }
    if (!view_raise_lds(k_view_gain<MASKS>, lds)) return (int)hipGetLastError();
    hipLaunchKernelGGL(k_view_gain<MASKS>, grid, block, lds, gnbv_stream(stream), p);
    return gnbv_launch_status();
}

// gnbv_view_gain_slab (MASKS false: the mask arguments are not looked at) and gnbv_view_gain_slab_masks
template <bool MASKS>
int view_gain_slab_impl(const GnbvViewGain *args, int slab, void *workspace, size_t workspace_bytes, int words,
                        int32_t *unknown_bits, int32_t *hit_bits, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvViewGain a = *args;
    GNBV_CHECK_ARG(view_gain_args_ok(a, kMaxSlabGrid) && depth_args_ok(a, false) && slab >= 0);
    VsPlan pl;
    GNBV_CHECK_ARG(vs_plan(a.n, a.k, a.g, a.h, a.w, a.stride, pl));
    GNBV_CHECK_ARG(workspace != nullptr && workspace_bytes >= pl.bytes && ((uintptr_t)workspace & 15) == 0);
    if (MASKS) GNBV_CHECK_ARG(mask_args_ok(a, words, unknown_bits, hit_bits));
    VsArgs<MASKS> p;
    // slab height: the fewest slabs whose grid + masks fit the LDS budget, of equal height; a requested height is kept if it fits
    int s = slab > a.g ? a.g : slab;
    if (s == 0) {
        int ns = 1;
        while (slab_lds_bytes(a.g, (a.g + ns - 1) / ns, p.grid_words, p.mask_words, MASKS) > kSlabLdsBudget) ++ns;
        s = (a.g + ns - 1) / ns;
    }
    while (slab_lds_bytes(a.g, s, p.grid_words, p.mask_words, MASKS) > kSlabLdsMax) --s;  // s = 1: 2 * 8 KiB at 128^3
    const size_t lds = slab_lds_bytes(a.g, s, p.grid_words, p.mask_words, MASKS);
    p.slab = s;
    p.nslab = (a.g + s - 1) / s;
    const int batch_pad = (pl.batch + 7) / 8 * 8;  // the XCD-aware grids are whole multiples of 8 envs
    // ten workgroups per compute unit even out the slabs' unequal shares of the rays (512 envs x 128^3, K = 32: 24.5 / 23.2 /
    // 22.8 ms at 16 / 8 / 4 candidates per workgroup; the slab's grid is re-read per workgroup)
    vg_fill(p, a, pl.lat, view_chunk(a.chunk, a.k, kSlabWorkgroups, pl.batch * p.nslab));
    p.rblocks = (p.nrays + kFateThreads - 1) / kFateThreads;
    GNBV_CHECK_ARG((int64_t)batch_pad * p.chunks * p.nslab <= 0x7fffffff && (int64_t)batch_pad * a.k * p.rblocks <= 0x7fffffff);
    p.pack_words = pl.pack_words;
    char *ws = static_cast<char *>(workspace);
    p.packed = reinterpret_cast<uint32_t *>(ws);
    p.cams = reinterpret_cast<float *>(ws + pl.off_cams);
    p.rec = reinterpret_cast<int4 *>(ws + pl.off_rec);
    p.meta = reinterpret_cast<uint32_t *>(ws + pl.off_meta);
    if constexpr (MASKS) {
        p.unknown_bits = reinterpret_cast<uint32_t *>(unknown_bits);
        p.hit_bits = reinterpret_cast<uint32_t *>(hit_bits);
        p.words = words;
        p.zero_all = p.nrays == 0;
        p.zero_words = p.zero_all ? words : p.nslab - 1 + (words - (a.g * a.g * a.g + 31) / 32);
    }
    const int threads = view_threads(p.nrays, lds);
    hipStream_t st = gnbv_stream(stream);
    const bool measured = a.depth_raw != nullptr;
    const VgDepth d = vg_depth(a);
    if (!(measured ? view_raise_lds(k_vg_carve_slab<MASKS>, lds) : view_raise_lds(k_vg_slab<MASKS>, lds))) return (int)hipGetLastError();
    for (int e0 = 0; e0 < a.n; e0 += pl.batch) {  // the workspace is reused: the stream orders the batches
        const int ne = a.n - e0 < pl.batch ? a.n - e0 : pl.batch, ne_pad = (ne + 7) / 8 * 8;
        int64_t items = (int64_t)ne * pl.pack_words;
        if ((int64_t)ne * a.k * 3 > items) items = (int64_t)ne * a.k * 3;
        if constexpr (MASKS)
            if ((int64_t)ne * a.k * p.zero_words > items) items = (int64_t)ne * a.k * p.zero_words;
        hipLaunchKernelGGL(k_vg_prep<MASKS>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, p, e0, ne);
        if (p.nrays == 0) continue;
        const dim3 fate_grid((unsigned)(ne_pad * a.k * p.rblocks)), slab_grid((unsigned)(ne_pad * p.chunks * p.nslab));
        if (measured) {
            hipLaunchKernelGGL(k_vg_fate_depth, fate_grid, dim3(kFateThreads), 0, st, p, d, e0, ne);
            hipLaunchKernelGGL(k_vg_carve_slab<MASKS>, slab_grid, dim3(threads), lds, st, p, d, e0, ne);
            continue;
        }
        hipLaunchKernelGGL(k_vg_fate, fate_grid, dim3(kFateThreads), 0, st, p, e0, ne);
        hipLaunchKernelGGL(k_vg_slab<MASKS>, slab_grid, dim3(threads), lds, st, p, e0, ne);
    }
    return gnbv_launch_status();
}

}  // namespace

GNBV_API int gnbv_view_gain(const GnbvViewGain *args, void *stream)
{
    return view_gain_impl<false>(args, 0, nullptr, nullptr, stream);
}

GNBV_API int gnbv_view_gain_masks(const GnbvViewGain *args, int words, int32_t *unknown_bits, int32_t *hit_bits, void *stream)
{
    return view_gain_impl<true>(args, words, unknown_bits, hit_bits, stream);
}

GNBV_API size_t gnbv_view_gain_slab_workspace_bytes(int n, int k, int g, int h, int w, int stride)
{
    VsPlan pl;
    return vs_plan(n, k, g, h, w, stride, pl) ? pl.bytes : 0;
}

GNBV_API int gnbv_view_gain_slab(const GnbvViewGain *args, int slab, void *workspace, size_t workspace_bytes, void *stream)
{
    return view_gain_slab_impl<false>(args, slab, workspace, workspace_bytes, 0, nullptr, nullptr, stream);
}

GNBV_API int gnbv_view_gain_slab_masks(const GnbvViewGain *args, int slab, void *workspace, size_t workspace_bytes, int words,
                                       int32_t *unknown_bits, int32_t *hit_bits, void *stream)
{
    return view_gain_slab_impl<true>(args, slab, workspace, workspace_bytes, words, unknown_bits, hit_bits, stream);
}

// viewcover.hip -- view coverage of candidate camera poses against an env's ground truth, on MI355X.
//
// "Which ground-truth voxels would the env's voxel update mark if the camera of env e stood at pose p?"  (DESIGN.md "View
// coverage, observable ground truth and the oracle planner"; include/gennbv_hip.h gnbv_view_cover has the exact definition.)
// For env e, candidate j and the pixel lattice u = s/2 + i s, v = s/2 + j s: the pixel's ray is traced with the renderer's own
// code (raytrace.h trace_pixel: the same bits as k_render_depth), a foreground hit is back-projected with the voxel update's
// canonical chain (backproject.h process_depth, pixel_to_world) and mapped to its voxel with the update's keep test
// (voxel_frame.h point_to_voxel, the update's own code).  No image is ever stored.
//
//   k_view_cover<WIN>   workgroup (env, chunk of candidates[, window of bit-set words]):
//     1. the camera batch (view_kernels.h: 16 lanes build the matrices of the next 16 candidates, off the per-candidate path);
//     2. one wave per 8 x 8 tile of lattice pixels (ray coherence, as the renderer), one ray per lane;
//     3. the seen set S is a bit set in LDS (G^3 / 8 bytes: 32 KiB at 64^3, 137 KiB at 104^3): atomicOr returns the old word,
//        and the lane that set a bit first reads the env's gt and scanned words (L2-resident: an env's workgroups run on one
//        XCD) and counts |S & gt| and |S & gt & ~scanned|;
//     4. block_sum (common.h), lane 0 stores the three integers;
//     5. seen_bits: the non-zero words of (bit set & gt) are OR-ed into global memory (device-scope atomicOr);
//     6. the workgroup clears the bit set (16-byte stores) before the next candidate.  With cover == NULL (accumulate only)
//        nothing is counted, the bit set is never cleared and it is flushed once, after the last candidate.
//   WIN (G > 105: the bit set exceeds the 144 KiB a workgroup keeps for it): the words are split into windows as in
//   k_hit_mask<.., WIN>; every window's workgroup traces all rays and keeps only its words.  The windows partition the voxels, so the per-window counts
//   are added with int32 atomicAdd (k_vc_zero clears cover first): integer sums, the same bits in any order.  `hits` is
//   counted by window 0 only.
//   MASK (gnbv_view_cover_masks): step 5 also stores (bit set & gt) as the workgroup's words of the candidate's mask row, plain
//   16-byte stores (the workgroup owns those words: no atomics, no zeroing launch), the zero words included; the workgroup of
//   the last window stores the row's pad words.  The bit set is cleared after every candidate, with or without `cover`.
#include "common.h"
#include "backproject.h"
#include "raytrace.h"
#include "scene_cells.h"
#include "view_kernels.h"
#include "voxel_frame.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kTile = 8;            // 8 x 8 lattice pixels = one wave
constexpr int kMaxGrid = 128;
constexpr size_t kLdsBitsMax = 144 * 1024;  // the bit set's share of the 160 KiB (static LDS: 1.2 KiB)

struct VcParams {
    GnbvMeshScene sc;
    int n, k, g, chunk, chunks, windows, nw, vwords, words;
    const float *poses, *range_gt, *voxel_size;
    Intrinsics kinv;
    int h, w, stride, nu, nv, tiles_x, tiles;
    float sense_dist;
    const uint32_t *gt, *scanned;
    int32_t *cover;
    uint32_t *seen;
    uint32_t *mask;  // [n, k, words], read by the MASK instantiations only
};

__global__ __launch_bounds__(256) void k_vc_zero(int32_t *cover, int64_t count)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) cover[t] = 0;
}

template <bool WIN, bool MASK>
__global__ __launch_bounds__(kViewMaxThreads) void k_view_cover(VcParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bits[];
    __shared__ float s_cam[kCamBatch][16];
    __shared__ int s_part[kViewMaxThreads / kWave][3];

    const int tid = threadIdx.x, nthreads = blockDim.x;
    int rem;  // (chunk[, window])
    const int e = xcd_env(p.chunks * p.windows, rem);
    if (e >= p.n) return;
    const int ch = rem % p.chunks, win = WIN ? rem / p.chunks : 0;
    const int w0 = win * p.nw;                                  // first bit-set word of this workgroup
    const int nw = WIN ? min(p.nw, p.vwords - w0) : p.vwords;   // a multiple of 4 (nw and vwords are)
    const int j0 = ch * p.chunk, j1 = min(p.k, j0 + p.chunk);
    const int g = p.g;

    uint4 *s_bits4 = reinterpret_cast<uint4 *>(s_bits);
    for (int i = tid; i < nw / 4; i += nthreads) s_bits4[i] = make_uint4(0u, 0u, 0u, 0u);

    const VoxelFrame f = load_frame(p.range_gt + e * 6, p.voxel_size + e * 3);
    const uint32_t *gt = p.gt + (size_t)e * p.words;
    const uint32_t *scanned = p.scanned != nullptr ? p.scanned + (size_t)e * p.words : nullptr;
    const bool count = p.cover != nullptr;
    const int wave = tid / kWave, nwaves = nthreads / kWave, lane = tid & (kWave - 1);

    // (bit set & gt) -> seen_bits: the non-zero words, 16 bytes at a time; `clear` also empties the words a lane flushed
    auto flush = [&](bool clear) {
        uint32_t *out = p.seen + (size_t)e * p.words + w0;
        for (int i = tid; i < nw / 4; i += nthreads) {
            const uint4 s = s_bits4[i];
            const uint4 t = *reinterpret_cast<const uint4 *>(gt + w0 + 4 * i);
            if ((s.x & t.x) != 0u) atomicOr(&out[4 * i + 0], s.x & t.x);
            if ((s.y & t.y) != 0u) atomicOr(&out[4 * i + 1], s.y & t.y);
            if ((s.z & t.z) != 0u) atomicOr(&out[4 * i + 2], s.z & t.z);
            if ((s.w & t.w) != 0u) atomicOr(&out[4 * i + 3], s.w & t.w);
            if (clear) s_bits4[i] = make_uint4(0u, 0u, 0u, 0u);
        }
    };

    for (int j = j0; j < j1; ++j) {
        // ---- 1. the camera batch (the slots' last readers passed the barrier that ended j - 1)
        const int cslot = camera_batch(s_cam, p.poses + (size_t)e * p.k * 6, j0, j, j1, [](int, int, const float *, const float *) {});
        __syncthreads();  // cameras ready; bit set clear

        // ---- 2 / 3. one wave per tile of lattice pixels, one ray per lane
        const float *M = s_cam[cslot];
        int cnt[3] = {0, 0, 0};  // new gt voxels, seen gt voxels, hits
        for (int tile = wave; tile < p.tiles; tile += nwaves) {
            const int iu = (tile % p.tiles_x) * kTile + (lane & 7);
            const int iv = (tile / p.tiles_x) * kTile + (lane >> 3);
            if (iu >= p.nu || iv >= p.nv) continue;
            const float fu = (float)lattice_pixel(iu, p.stride), fv = (float)lattice_pixel(iv, p.stride);
            float best;
            int obj;
            trace_pixel(p.sc, e, M, p.kinv.k, fu, fv, best, obj);
            if (obj <= 0) continue;  // the render's seg 0: the update's `seg > 50` drops the pixel
            const float d = process_depth(-best, p.sense_dist);
            float wp[3];
            pixel_to_world(d, fu, fv, p.kinv, M, wp);
            int ix[3];
            const int lin = point_to_voxel(wp, f, g, ix);
            if (lin < 0) continue;
            if (!WIN || win == 0) ++cnt[2];
            const unsigned wi = (unsigned)((lin >> 5) - w0);
            if (wi >= (unsigned)nw) continue;  // another window's word
            const uint32_t bit = 1u << (lin & 31);
            if (mark_first(s_bits + wi, lin & 31) && count && (gt[lin >> 5] & bit) != 0u) {
                ++cnt[1];
                if (scanned == nullptr || (scanned[lin >> 5] & bit) == 0u) ++cnt[0];
            }
        }

        // ---- 4. the three sums; without `cover` only the barrier (`count` is the same in every thread).  Either barrier: every
        //      ray of candidate j is done, the bit set is complete, the camera slot free
        if (count) block_sum(cnt, s_part);
        else __syncthreads();
        if (!count && !MASK) continue;  // accumulate only: the bit set keeps growing
        if (count && tid == 0) {
            int32_t *o = p.cover + ((size_t)e * p.k + j) * 3;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (!WIN) o[q] = cnt[q];
                else if (cnt[q] != 0) atomicAdd(o + q, cnt[q]);
            }
        }
        // ---- 5 / 6. flush, then clear for the next candidate (a lane clears the words it flushed: no barrier between the
        //      two; the clear is ordered in front of the next rays by the barrier at the loop's head, which also is the one
        //      block_sum leaves to its caller)
        if (MASK) {
            // the candidate's mask row: this workgroup owns words [w0, w0 + nw) of it, every one is stored
            uint32_t *row = p.mask + ((size_t)e * p.k + j) * p.words;
            uint32_t *out = p.seen != nullptr ? p.seen + (size_t)e * p.words + w0 : nullptr;
            for (int i = tid; i < nw / 4; i += nthreads) {
                const uint4 s = s_bits4[i];
                const uint4 t = *reinterpret_cast<const uint4 *>(gt + w0 + 4 * i);
                const uint4 m = make_uint4(s.x & t.x, s.y & t.y, s.z & t.z, s.w & t.w);
                *reinterpret_cast<uint4 *>(row + w0 + 4 * i) = m;
                if (out != nullptr) {
                    if (m.x != 0u) atomicOr(&out[4 * i + 0], m.x);
                    if (m.y != 0u) atomicOr(&out[4 * i + 1], m.y);
                    if (m.z != 0u) atomicOr(&out[4 * i + 2], m.z);
                    if (m.w != 0u) atomicOr(&out[4 * i + 3], m.w);
                }
                s_bits4[i] = make_uint4(0u, 0u, 0u, 0u);
            }
            if (w0 + nw == p.vwords)  // the pad words past the voxels (words - vwords is a multiple of 4)
                for (int i = tid; i < (p.words - p.vwords) / 4; i += nthreads)
                    *reinterpret_cast<uint4 *>(row + p.vwords + 4 * i) = make_uint4(0u, 0u, 0u, 0u);
        } else if (p.seen != nullptr) {
            flush(true);
        } else if (j + 1 < j1) {
            for (int i = tid; i < nw / 4; i += nthreads) s_bits4[i] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (!count && !MASK) flush(false);  // (the barrier that ended the last candidate completed the bit set)
}

}  // namespace

template <bool WIN, bool MASK>
static int launch_view_cover(const VcParams &p, unsigned blocks, int threads, size_t lds, hipStream_t st)
{
    if (!view_raise_lds(k_view_cover<WIN, MASK>, lds)) return (int)hipGetLastError();
    hipLaunchKernelGGL((k_view_cover<WIN, MASK>), dim3(blocks), dim3(threads), lds, st, p);
    return gnbv_launch_status();
}

// gnbv_view_cover (mask_bits == NULL, with_masks false) and gnbv_view_cover_masks
static int view_cover_impl(const GnbvMeshScene *scene, const GnbvViewCover *args, int32_t *mask_bits, bool with_masks, void *stream);

GNBV_API int gnbv_view_cover(const GnbvMeshScene *scene, const GnbvViewCover *args, void *stream)
{
    return view_cover_impl(scene, args, nullptr, false, stream);
}

GNBV_API int gnbv_view_cover_masks(const GnbvMeshScene *scene, const GnbvViewCover *args, int32_t *mask_bits, void *stream)
{
    return view_cover_impl(scene, args, mask_bits, true, stream);
}

static int view_cover_impl(const GnbvMeshScene *scene, const GnbvViewCover *args, int32_t *mask_bits, bool with_masks, void *stream)
{
    GNBV_CHECK_ARG(scene != nullptr && args != nullptr);
    const GnbvViewCover a = *args;
    const GnbvMeshScene sc = *scene;
    GNBV_CHECK_ARG(a.n > 0 && a.n <= 65535 && sc.n == a.n && a.k >= 1 && a.g >= 2 && a.g <= kMaxGrid && a.stride >= 1);
    GNBV_CHECK_ARG(a.h > 0 && a.w > 0 && a.h <= 32768 && a.w <= 32768 && a.chunk >= 0 && a.window >= 0);
    GNBV_CHECK_ARG(a.poses != nullptr && a.range_gt != nullptr && a.voxel_size != nullptr && a.inv_intri != nullptr && a.gt_bits != nullptr);
    if (with_masks)
        GNBV_CHECK_ARG(mask_bits != nullptr && ((uintptr_t)mask_bits & 15) == 0);
    else
        GNBV_CHECK_ARG(a.cover != nullptr || a.seen_bits != nullptr);
    GNBV_CHECK_ARG(scene_ok(sc));
    GNBV_CHECK_ARG((((uintptr_t)a.gt_bits | (uintptr_t)a.scanned_bits | (uintptr_t)a.seen_bits) & 15) == 0);
    VcParams p;
    p.sc = sc;
    p.n = a.n; p.k = a.k; p.g = a.g;
    const int g3 = a.g * a.g * a.g;
    p.words = gnbv_grid_bit_words(a.g);             // the updater's row length (a multiple of 64 words)
    p.vwords = (((g3 + 31) / 32) + 3) & ~3;         // the words that hold voxels, to 16 bytes (<= words)
    // windows: the fewest equal windows whose words fit the LDS; a requested window is kept if it fits
    int nw = a.window;
    if (nw == 0) {
        const int wins = (int)(((size_t)p.vwords * 4 + kLdsBitsMax - 1) / kLdsBitsMax);
        nw = (p.vwords + wins - 1) / wins;
    }
    nw = (nw + 3) & ~3;
    if ((size_t)nw * 4 > kLdsBitsMax) nw = (int)(kLdsBitsMax / 4);
    if (nw > p.vwords) nw = p.vwords;
    p.nw = nw;
    p.windows = (p.vwords + nw - 1) / nw;
    // candidates per workgroup: two workgroups per compute unit when n allows it; the cameras and the frame are built per workgroup
    p.chunk = view_chunk(a.chunk, a.k, 512, a.n * p.windows);
    p.chunks = (a.k + p.chunk - 1) / p.chunk;
    const int64_t blocks = (int64_t)((a.n + 7) / 8 * 8) * p.chunks * p.windows;
    GNBV_CHECK_ARG(blocks <= 0x7fffffff);
    p.poses = a.poses; p.range_gt = a.range_gt; p.voxel_size = a.voxel_size;
    for (int i = 0; i < 9; ++i) p.kinv.k[i] = a.inv_intri[i];
    p.h = a.h; p.w = a.w; p.stride = a.stride;
    const ViewLattice lat = view_lattice(a.h, a.w, a.stride);
    p.nu = lat.nu; p.nv = lat.nv;
    p.tiles_x = (p.nu + kTile - 1) / kTile;
    p.tiles = p.tiles_x * ((p.nv + kTile - 1) / kTile);
    p.sense_dist = a.depth_sense_dist;
    p.gt = reinterpret_cast<const uint32_t *>(a.gt_bits);
    p.scanned = reinterpret_cast<const uint32_t *>(a.scanned_bits);
    p.cover = a.cover;
    p.seen = reinterpret_cast<uint32_t *>(a.seen_bits);
    p.mask = reinterpret_cast<uint32_t *>(mask_bits);
    const size_t lds = (size_t)nw * sizeof(uint32_t);
    int threads = (p.tiles > 0 ? p.tiles : 1) * kWave;
    threads = threads > kViewMaxThreads ? kViewMaxThreads : threads;
    hipStream_t st = gnbv_stream(stream);
    if (p.windows > 1) {
        if (a.cover != nullptr) {
            const int64_t cnt = (int64_t)a.n * a.k * 3;
            hipLaunchKernelGGL(k_vc_zero, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, a.cover, cnt);
        }
        return with_masks ? launch_view_cover<true, true>(p, (unsigned)blocks, threads, lds, st)
                          : launch_view_cover<true, false>(p, (unsigned)blocks, threads, lds, st);
    }
    return with_masks ? launch_view_cover<false, true>(p, (unsigned)blocks, threads, lds, st)
                      : launch_view_cover<false, false>(p, (unsigned)blocks, threads, lds, st);
}

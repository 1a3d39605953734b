// frontier.hip -- the frontier of the scanned map (gnbv_frontier_tri): the unknown voxels with a free face neighbour, per env, as
// bits and as block records {count, sum x, sum y, sum z}.  Integers only: one right answer, tests compare with ==.
//
//   k_frontier_tri<kF32>   workgroup (env, slab of x-planes [X0, X1)), 512 lanes, three phases with a barrier between them.
//     1. pack: the slab, the plane below it, the plane above it and 32 voxels more go into two LDS bit planes, "free" and "unknown"
//        (map_bits.h: map_pack_window; coalesced reads of either grid form).  The voxel order (x G + y) G + z is the memory order, so
//        the window is one run of voxels and one run of bits; it starts at a multiple of 32 voxels, so word w of the window is word
//        w + base of bits_out.  Bits past either end of the grid are clear in both planes: a neighbour outside is no neighbour.
//     2. frontier words: a lane takes one 32-voxel word: unknown AND (the free plane read at the bit offsets -1, +1, -G, +G, -G^2,
//        +G^2).  The +-z reads are masked where z = 0 / G - 1 and the +-y reads where y = 0 / G - 1 (the voxel after (x, y, G - 1) in
//        memory is not its z-neighbour), masks built from the word's position alone; the +-x reads need none, the planes outside
//        the grid are clear.  Lanes read consecutive words: no bank conflict, no swizzle.  A slab owns the output words whose first
//        voxel lies in it -- one writer per word -- and such a word may reach up to 31 voxels into plane X1: that is what the extra
//        32 voxels of the window are for.  The word replaces the lane's own word of the unknown plane (nothing else reads it).
//     3. block records: a lane takes one block of the slab (the slab height is a multiple of B, so a block lies in one slab), walks
//        its at most B x B rows of at most B voxels in the frontier plane -- count by popcount, sum z by four masked popcounts -- and
//        stores the four ints of the record: every record one writer, no atomics, zeros where empty.
//   Every loop is bounded by G and constants: no loop count comes from the arrays.
//   The grid forms, the pack loop and the LDS limit are map_bits.h's, shared with the other kernels on the map.
#include <algorithm>

#include "common.h"
#include "map_bits.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kFrontLanes = 512;  // (256 and 1024 lanes, and 16 loads per pack turn, were measured: DESIGN.md)
constexpr int kFrontWaves = kFrontLanes / kWave;
constexpr int kFrontMaxBlock = 16;
// the auto slab: the tallest whose planes stay below this (three workgroups per CU) while all envs together still give kFrontGroups
constexpr size_t kFrontAutoLdsBytes = 48 * 1024;
constexpr int64_t kFrontGroups = 1024;

struct FrontierArgs {
    int g, g2, g3, block, nb, slab, chunks;
    int words_out;  // ceil(G^3 / 32)
    int lds_words;  // words of one LDS plane (even)
};

// words of one LDS plane for a slab of `slab` x-planes: slab + 2 planes, 32 voxels more, up to 31 voxels of alignment in front
constexpr size_t frontier_plane_words(int g, int slab)
{
    const size_t w = ((size_t)(slab + 2) * g * g + 63) / 32 + 2;
    return (w + 1) / 2 * 2;
}

// bits off .. off + 31 of a plane of `words` words; bits outside the plane read as 0
__device__ __forceinline__ uint32_t window_bits(const uint32_t *p, int words, int off)
{
    const int w = off >> 5, s = off & 31;  // (>> of a negative int floors on this target)
    const uint32_t lo = (w >= 0 && w < words) ? p[w] : 0u;
    const uint32_t hi = (w + 1 >= 0 && w + 1 < words) ? p[w + 1] : 0u;
    return s ? (lo >> s) | (hi << (32 - s)) : lo;
}

// bit i (0 .. 31) set iff (r + i) mod period < len, for 0 <= r < period, 1 <= len <= period: at most 32 / period + 2 turns
__device__ __forceinline__ uint32_t run_mask(int r, int period, int len)
{
    uint32_t m = 0u;
    for (int q = -r; q < 32; q += period) {
        const int a = max(q, 0), b = min(q + len, 32);
        if (b > a) m |= (b - a == 32 ? 0xFFFFFFFFu : ((1u << (b - a)) - 1u)) << a;
    }
    return m;
}

// the sum of the positions of the set bits of a 16-bit segment
__device__ __forceinline__ int bit_position_sum(uint32_t seg)
{
    return __popc(seg & 0xAAAAu) + 2 * __popc(seg & 0xCCCCu) + 4 * __popc(seg & 0xF0F0u) + 8 * __popc(seg & 0xFF00u);
}

template <bool kF32>
__global__ __launch_bounds__(kFrontLanes) void k_frontier_tri(const void *__restrict__ tri_base, int64_t row_bytes, FrontierArgs a,
                                                              uint32_t *__restrict__ bits_out, int32_t *__restrict__ blocks_out)
{
    extern __shared__ __attribute__((aligned(16))) char front_lds[];
    uint32_t *fre = reinterpret_cast<uint32_t *>(front_lds), *unk = fre + a.lds_words;
    const int e = blockIdx.x / a.chunks, chunk = blockIdx.x - e * a.chunks;
    const int g = a.g, g2 = a.g2, words = a.lds_words;
    const int x0 = chunk * a.slab, x1 = min(x0 + a.slab, g);
    const int lo_bit = x0 * g2, hi_bit = x1 * g2;  // the slab's voxels
    // the window starts one plane below the slab, rounded down to a whole word (for x0 = 0 below the grid: clear bits)
    const int base_w = x0 > 0 ? (lo_bit - g2) / 32 : -((g2 + 31) / 32);
    const int first = base_w * 32;
    const void *tri = static_cast<const char *>(tri_base) + (size_t)e * row_bytes;

    map_pack_window<kF32, kFrontWaves>(tri, a.g3, first, words, fre, unk);
    __syncthreads();

    // every word that holds a voxel of the slab; the first may begin in the plane below (the slab before owns it: not stored)
    uint32_t *out = bits_out != nullptr ? bits_out + (size_t)e * a.words_out : nullptr;
    for (int gw = (lo_bit >> 5) + (int)threadIdx.x; gw <= ((hi_bit - 1) >> 5); gw += kFrontLanes) {
        const int lw = gw - base_w, b = lw * 32, vox = gw * 32;
        const uint32_t u = unk[lw];
        uint32_t fr = 0u;
        if (u != 0u) {
            const int r2 = vox % g2, r1 = r2 % g;  // the word's first voxel inside its x-plane, inside its row
            const uint32_t z_first = run_mask(r1, g, 1), z_last = run_mask(r1 + 1 == g ? 0 : r1 + 1, g, 1);
            const uint32_t y_first = run_mask(r2, g2, g), y_last = run_mask(r2 + g >= g2 ? r2 + g - g2 : r2 + g, g2, g);
            uint32_t adj = window_bits(fre, words, b - 1) & ~z_first;
            adj |= window_bits(fre, words, b + 1) & ~z_last;
            adj |= window_bits(fre, words, b - g) & ~y_first;
            adj |= window_bits(fre, words, b + g) & ~y_last;
            adj |= window_bits(fre, words, b - g2);
            adj |= window_bits(fre, words, b + g2);
            fr = u & adj;
        }
        if (out != nullptr && vox >= lo_bit) out[gw] = fr;
        unk[lw] = fr;
    }
    __syncthreads();

    const int bsz = a.block, nb = a.nb;
    const int nbx = (x1 - x0 + bsz - 1) / bsz;
    int32_t *records = blocks_out + (size_t)e * nb * nb * nb * 4;
    for (int t = threadIdx.x; t < nbx * nb * nb; t += kFrontLanes) {
        const int bz = t % nb, by = (t / nb) % nb, bx = x0 / bsz + t / (nb * nb);
        const int z0 = bz * bsz;
        const uint32_t seg_mask = (1u << min(bsz, g - z0)) - 1u;
        int cnt = 0, sx = 0, sy = 0, sz = 0;
        for (int x = bx * bsz; x < min(bx * bsz + bsz, x1); ++x) {
            for (int y = by * bsz; y < min(by * bsz + bsz, g); ++y) {
                const uint32_t seg = window_bits(unk, words, (x * g + y) * g + z0 - first) & seg_mask;
                const int c = __popc(seg);
                cnt += c;
                sx += x * c;
                sy += y * c;
                sz += z0 * c + bit_position_sum(seg);
            }
        }
        int32_t *rec = records + (size_t)((bx * nb + by) * nb + bz) * 4;
        rec[0] = cnt;
        rec[1] = sx;
        rec[2] = sy;
        rec[3] = sz;
    }
}

template <bool kF32>
int launch_frontier(const MapGrid &grid, const FrontierArgs &a, int n, uint32_t *bits_out, int32_t *blocks_out, hipStream_t stream)
{
    const size_t lds = 8 * (size_t)a.lds_words;
    const int bad = gnbv_raise_lds<k_frontier_tri<kF32>>(lds, kMapLdsBytes);
    if (bad != 0) return bad;
    hipLaunchKernelGGL((k_frontier_tri<kF32>), dim3((unsigned)(n * a.chunks)), dim3(kFrontLanes), lds, stream, grid.base, grid.row_bytes, a,
                       bits_out, blocks_out);
    return gnbv_launch_status();
}

}  // namespace

GNBV_API int gnbv_frontier_tri(const int8_t *tri_i8, int64_t tri_i8_row_stride, const float *tri_f32, int64_t tri_f32_row_stride, int g,
                               int n, int block, uint32_t *bits_out, int32_t *blocks_out, int slab, void *stream)
{
    MapGrid grid;
    const int bad = map_grid(tri_i8, tri_i8_row_stride, tri_f32, tri_f32_row_stride, g, &grid);
    if (bad != 0) return bad;
    GNBV_CHECK_ARG(blocks_out != nullptr);
    GNBV_CHECK_ARG(n >= 1 && block >= 1 && block <= kFrontMaxBlock && slab >= 0);
    // the slab height: a multiple of B (a block record has one writer), at most what the two planes leave of LDS, at least B
    // (B = 16 at 128^3 is 72 KiB).  Auto: the tallest that keeps the planes small and the workgroups many.
    const int whole = (g + block - 1) / block * block;
    int s = slab == 0 ? whole : (int)std::min<int64_t>(((int64_t)slab + block - 1) / block * block, whole);
    while (s > block && 8 * frontier_plane_words(g, s) > (size_t)kMapLdsBytes) s -= block;
    if (slab == 0) {
        while (s > block && (8 * frontier_plane_words(g, s) > kFrontAutoLdsBytes || (int64_t)n * ((g + s - 1) / s) < kFrontGroups)) s -= block;
        const int chunks = (g + s - 1) / s;  // the same number of slabs, of even height: no short last slab behind tall ones
        s = ((g + chunks - 1) / chunks + block - 1) / block * block;
    }
    FrontierArgs a;
    a.g = g;
    a.g2 = g * g;
    a.g3 = g * g * g;
    a.block = block;
    a.nb = (g + block - 1) / block;
    a.slab = s;
    a.chunks = (g + s - 1) / s;
    a.words_out = (a.g3 + 31) / 32;
    a.lds_words = (int)frontier_plane_words(g, s);
    GNBV_CHECK_ARG((int64_t)n * a.chunks <= 0x7fffffff);
    return grid.f32 ? launch_frontier<true>(grid, a, n, bits_out, blocks_out, gnbv_stream(stream))
                    : launch_frontier<false>(grid, a, n, bits_out, blocks_out, gnbv_stream(stream));
}

// scan.hip -- reconstruction accuracy of the evaluation env on the device (env_eval_gennbv.py:156-164, :253-263):
// every env step adds the 1 cm keys of each env's foreground points to that env's set; when an env finishes, its set
// is scored against the env's GT cloud by Chamfer distance x 100, and a masked clear empties it (reset_idx :321-322).
//
// The set is a per-env open-addressing hash table of 64-bit keys (linear probing, `capacity` slots) plus an append list
// of the keys it holds.  A hash, not an append log de-duplicated at scoring, because most keys of a frame were already
// seen on the previous frames: a hit costs one load and no atomic (checked before the compare-and-swap), and the
// scoring sorts the unique keys only.  A key is the Morton code of the three 21-bit fields rint(100 p) + 2^20, so a
// 4 x 4 x 4 cm brick is 64 consecutive codes; the slot of a key is hash(brick) * 64 + (code & 63), which keeps the
// probes of neighbouring pixels in the same cache lines.  A table can never hold more than `capacity` keys: a key that
// finds no free slot after `capacity` probes sets the env's overflow flag instead of being dropped silently.
//
// Scoring (masked by the caller's done flags, batched over every env that is flagged, not yet scored and non-empty):
//   1. an LSD radix sort (4-bit digits, stable, 16 passes) orders the env's key list by Morton code;
//   2. the sorted keys become points k * 0.01f (unique_rounded_points' rows) grouped in leaves of 32 consecutive points
//      with an implicit binary tree of bounding boxes above them (heap layout, padded to a power of two);
//   3. every unique point queries the GT cloud's tree (built once at construction, gennbv_amd/eval/scan_accumulator.py)
//      and every GT point queries the scanned cloud's tree for its nearest squared distance, with the per-pair formula
//      of chamfer.hip's k_nn_sqdist.  A box is skipped only when its lower bound exceeds the current best by 2^-20
//      relative, which covers the fp32 rounding of the bound and of the pair formula: the minimum is the brute force's;
//   4. fixed-order fp64 sums with the block structure of chamfer.hip's k_sum_f64 + k_chamfer_finish.
#include "common.h"
#include "backproject.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr uint64_t kEmpty = ~0ull;   // no valid key has bit 63 set
constexpr int kKeyBits = 21, kKeyOffset = 1 << 20;
constexpr float kKeyLimit = 1048576.0f;  // |rint(100 p)| < 2^20, the range of unique_rounded_points' integer path
constexpr int kFlagOverflow = 1, kFlagRange = 2;
constexpr int kLeaf = 32;
constexpr int kSortThreads = 256, kSortPer = 8, kSortTile = kSortThreads * kSortPer, kSortPasses = 16;
constexpr int kSumBlocks = 512;  // == chamfer.hip's kSumBlocks: same partial-sum structure

__device__ __forceinline__ uint64_t spread3(uint64_t v)  // 21 bits -> every third bit
{
    v &= 0x1fffff;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}

__device__ __forceinline__ uint32_t compact3(uint64_t v)
{
    v &= 0x1249249249249249ull;
    v = (v ^ (v >> 2)) & 0x10c30c30c30c30c3ull;
    v = (v ^ (v >> 4)) & 0x100f00f00f00f00full;
    v = (v ^ (v >> 8)) & 0x1f0000ff0000ffull;
    v = (v ^ (v >> 16)) & 0x1f00000000ffffull;
    v = (v ^ (v >> 32)) & 0x1fffff;
    return (uint32_t)v;
}

// (x, y, z) fields (already offset by 2^20) <-> Morton code
__device__ __forceinline__ uint64_t morton(uint32_t x, uint32_t y, uint32_t z) { return spread3(x) << 2 | spread3(y) << 1 | spread3(z); }

__device__ __forceinline__ void unmorton(uint64_t c, int *k)
{
    k[0] = (int)compact3(c >> 2) - kKeyOffset;
    k[1] = (int)compact3(c >> 1) - kKeyOffset;
    k[2] = (int)compact3(c) - kKeyOffset;
}

// unique_rounded_points' row of a key: k.to(float32) / 100.0 -- torch divides by a CPU scalar as a * (1.0f / 100.0f)
__device__ __forceinline__ float key_to_coord(int k) { return __fmul_rn((float)k, 0.01f); }

__device__ __forceinline__ int64_t first_slot(uint64_t code, int64_t cap)
{
    const uint64_t h = ((code >> 6) * 0x9E3779B97F4A7C15ull) >> 32;  // brick hash, 32 bits
    return (int64_t)(((h * (uint64_t)(cap >> 6)) >> 32) << 6 | (code & 63));
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// ---------------------------------------------------------------------------
// accumulate: one launch per env step, grid (ceil(H*W / 256), N)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scan_add(const float *__restrict__ depth_raw, const float *__restrict__ seg_raw,
                                                const float *__restrict__ c2w, Intrinsics K, int h, int w, float sense,
                                                int64_t cap, uint64_t *__restrict__ table, uint64_t *__restrict__ list,
                                                int32_t *__restrict__ counts, int32_t *__restrict__ flags)
{
    const int e = blockIdx.y;
    const int hw = h * w;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    bool fg = false, bad = false;
    uint64_t code = 0;
    if (p < hw) {
        const size_t i = (size_t)e * hw + p;
        fg = nan_to_num_neginf0(seg_raw[i]) > 50.0f;
        if (fg) {
            float M[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) M[k] = c2w[(size_t)e * 16 + k];
            const int y = p / w, x = p - y * w;
            float wp[3];
            pixel_to_world(process_depth(depth_raw[i], sense), (float)x, (float)y, K, M, wp);
            uint32_t f[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float r = rintf(__fmul_rn(wp[a], 100.0f));  // torch.round(p * 100.0): half to even
                bad = bad || !(fabsf(r) < kKeyLimit);               // also NaN / inf
                f[a] = bad ? 0u : (uint32_t)((int)r + kKeyOffset);
            }
            code = morton(f[0], f[1], f[2]);
            fg = !bad;
        }
    }
    bool claimed = false, lost = false;
    if (fg) {
        uint64_t *tab = table + (size_t)e * cap;
        int64_t s = first_slot(code, cap);
        bool done = false;
        for (int64_t probe = 0; probe < cap && !done; ++probe) {
            const uint64_t cur = __hip_atomic_load(tab + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == code) {
                done = true;  // seen on an earlier frame or by another lane: no atomic
            } else if (cur == kEmpty) {
                const uint64_t old = atomicCAS((unsigned long long *)(tab + s), (unsigned long long)kEmpty, (unsigned long long)code);
                claimed = old == kEmpty;
                done = claimed || old == code;
            }
            if (++s == cap) s = 0;
        }
        lost = !done;
    }
    // one atomic per wave for the new keys and for each flag
    const uint64_t mc = __ballot(claimed), mb = __ballot(bad), ml = __ballot(lost);
    const int lane = threadIdx.x & (kWave - 1);
    int base = 0;
    if (mc) {
        const int leader = __ffsll((unsigned long long)mc) - 1;
        if (lane == leader) base = atomicAdd(counts + e, (int)__popcll(mc));
        base = __shfl(base, leader);
    }
    if (claimed) {
        const int64_t pos = (int64_t)base + lanes_below(mc);
        if (pos < cap) list[(size_t)e * cap + pos] = code;  // (always: one list entry per claimed slot)
    }
    if (lane == 0 && (mb | ml)) atomicOr(flags + e, (mb ? kFlagRange : 0) | (ml ? kFlagOverflow : 0));
}

// ---------------------------------------------------------------------------
// masked clear: grid (blocks, N)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scan_clear(const uint8_t *__restrict__ mask, int64_t cap, uint64_t *__restrict__ table,
                                                  int32_t *__restrict__ counts)
{
    const int e = blockIdx.y;
    if (!mask[e]) return;
    uint4 *t = (uint4 *)(table + (size_t)e * cap);  // cap is a multiple of 64: 16-B stores
    const int64_t n = cap / 2;
    const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) t[i] = ones;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[e] = 0;
}

// ---------------------------------------------------------------------------
// scoring
// ---------------------------------------------------------------------------
__global__ void k_score_prep(const uint8_t *__restrict__ mask, const int32_t *__restrict__ scored, const int32_t *__restrict__ counts,
                             const int32_t *__restrict__ flags, int n, int32_t *__restrict__ active)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) active[e] = (mask[e] && !scored[e] && counts[e] > 0 && flags[e] == 0) ? 1 : 0;
}

// LSD radix sort of each active env's keys [e * stride, e * stride + counts[e]); hist [N][16][tmax]
__global__ __launch_bounds__(kSortThreads) void k_radix_hist(const uint64_t *__restrict__ src, int64_t stride, const int32_t *__restrict__ counts,
                                                           const int32_t *__restrict__ active, int shift, uint32_t *__restrict__ hist, int tmax)
{
    const int e = blockIdx.y;
    if (!active[e]) return;
    const int n = counts[e], tiles = (n + kSortTile - 1) / kSortTile;
    const uint64_t *s = src + (size_t)e * stride;
    __shared__ uint32_t hs[16];
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        if (threadIdx.x < 16) hs[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSortPer; ++k) {
            const int i = t * kSortTile + k * kSortThreads + threadIdx.x;
            if (i < n) atomicAdd(&hs[(s[i] >> shift) & 15], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 16) hist[((size_t)e * 16 + threadIdx.x) * tmax + t] = hs[threadIdx.x];
        __syncthreads();
    }
}

// exclusive scan of [digit][tile] per env, in place (digit-major: stable LSD order)
__global__ __launch_bounds__(256) void k_radix_scan(const int32_t *__restrict__ counts, const int32_t *__restrict__ active,
                                                  uint32_t *__restrict__ hist, int tmax)
{
    const int e = blockIdx.x;
    if (!active[e]) return;
    const int tiles = (counts[e] + kSortTile - 1) / kSortTile, total = 16 * tiles;
    __shared__ uint32_t s[256];
    uint32_t carry = 0;
    for (int b = 0; b < total; b += 256) {
        const int i = b + threadIdx.x;
        const int d = i / max(tiles, 1), t = i - d * tiles;
        uint32_t *slot = hist + ((size_t)e * 16 + d) * tmax + t;
        const uint32_t v = i < total ? *slot : 0u;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const uint32_t a = threadIdx.x >= o ? s[threadIdx.x - o] : 0u;
            __syncthreads();
            s[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < total) *slot = carry + s[threadIdx.x] - v;
        carry += s[255];
        __syncthreads();
    }
}

__device__ __forceinline__ int pad16(int i) { return i + (i >> 4); }

__global__ __launch_bounds__(kSortThreads) void k_radix_scatter(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int64_t stride,
                                                              const int32_t *__restrict__ counts, const int32_t *__restrict__ active, int shift,
                                                              const uint32_t *__restrict__ offs, int tmax)
{
    const int e = blockIdx.y;
    if (!active[e]) return;
    const int n = counts[e], tiles = (n + kSortTile - 1) / kSortTile;
    const uint64_t *s = src + (size_t)e * stride;
    uint64_t *o = dst + (size_t)e * stride;
    __shared__ uint32_t cnt[16 * 272];  // [digit][pad16(thread)]: per-thread counts, then their exclusive prefix
    __shared__ uint32_t seg[16][16];
    __shared__ uint32_t base[16];
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        // thread tid owns keys [tid * 8, tid * 8 + 8) of the tile: thread order = key order (stable)
        uint64_t key[kSortPer];
        uint64_t c = 0;  // 16 nibble counters
#pragma unroll
        for (int k = 0; k < kSortPer; ++k) {
            const int i = t * kSortTile + tid * kSortPer + k;
            key[k] = i < n ? s[i] : 0;
            if (i < n) c += 1ull << (4 * ((key[k] >> shift) & 15));
        }
#pragma unroll
        for (int d = 0; d < 16; ++d) cnt[d * 272 + pad16(tid)] = (uint32_t)(c >> (4 * d)) & 15u;
        if (tid < 16) base[tid] = offs[((size_t)e * 16 + tid) * tmax + t];
        __syncthreads();
        {   // per digit, prefix over the 256 threads: thread (d, q) scans threads [16 q, 16 q + 16)
            const int d = tid >> 4, q = tid & 15;
            uint32_t run = 0;
            for (int j = 0; j < 16; ++j) {
                uint32_t *x = &cnt[d * 272 + pad16(q * 16 + j)];
                const uint32_t v = *x;
                *x = run;
                run += v;
            }
            seg[d][q] = run;
            __syncthreads();
            uint32_t pre = 0;
            for (int j = 0; j < q; ++j) pre += seg[d][j];
            for (int j = 0; j < 16; ++j) cnt[d * 272 + pad16(q * 16 + j)] += pre;
        }
        __syncthreads();
        uint64_t r = 0;
#pragma unroll
        for (int k = 0; k < kSortPer; ++k) {
            const int i = t * kSortTile + tid * kSortPer + k;
            if (i < n) {
                const int d = (int)((key[k] >> shift) & 15);
                const uint32_t pos = base[d] + cnt[d * 272 + pad16(tid)] + (uint32_t)((r >> (4 * d)) & 15);
                r += 1ull << (4 * d);
                o[pos] = key[k];
            }
        }
        __syncthreads();
    }
}

// sorted codes -> points (float4, w unused) and the leaf boxes of the scanned cloud's tree.
// nodes [N][node_stride = 2 * pmax][2] float4 (lo, hi); heap: root 1, children 2i and 2i+1, leaf j at P + j; a node
// without points is the empty box (lo = +inf, hi = -inf), whose bound is +inf.
__device__ __forceinline__ int tree_pow2(int leaves)
{
    int p = 1;
    while (p < leaves) p <<= 1;
    return p;
}

__global__ __launch_bounds__(256) void k_x_points(const uint64_t *__restrict__ keys, int64_t cap, const int32_t *__restrict__ counts,
                                                const int32_t *__restrict__ active, float4 *__restrict__ pts, float4 *__restrict__ nodes,
                                                int64_t node_stride)
{
    const int e = blockIdx.y;
    if (!active[e]) return;
    const int n = counts[e], P = tree_pow2((n + kLeaf - 1) / kLeaf);
    float4 *ne = nodes + (size_t)e * node_stride * 2;
    const int64_t total = (int64_t)P * kLeaf;  // multiple of the 256 stride: a leaf's 32 lanes run together
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float x = INFINITY, y = INFINITY, z = INFINITY, X = -INFINITY, Y = -INFINITY, Z = -INFINITY;
        if (i < n) {
            int k[3];
            unmorton(keys[(size_t)e * cap + i], k);
            x = X = key_to_coord(k[0]);
            y = Y = key_to_coord(k[1]);
            z = Z = key_to_coord(k[2]);
            pts[(size_t)e * cap + i] = make_float4(x, y, z, 0.0f);
        }
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            x = fminf(x, __shfl_xor(x, m)); y = fminf(y, __shfl_xor(y, m)); z = fminf(z, __shfl_xor(z, m));
            X = fmaxf(X, __shfl_xor(X, m)); Y = fmaxf(Y, __shfl_xor(Y, m)); Z = fmaxf(Z, __shfl_xor(Z, m));
        }
        if ((i & (kLeaf - 1)) == 0) {
            const int64_t node = P + i / kLeaf;
            ne[2 * node] = make_float4(x, y, z, 0.0f);
            ne[2 * node + 1] = make_float4(X, Y, Z, 0.0f);
        }
    }
}

__global__ __launch_bounds__(1024) void k_x_levels(const int32_t *__restrict__ counts, const int32_t *__restrict__ active,
                                                 float4 *__restrict__ nodes, int64_t node_stride)
{
    const int e = blockIdx.x;
    if (!active[e]) return;
    const int P = tree_pow2((counts[e] + kLeaf - 1) / kLeaf);
    float4 *ne = nodes + (size_t)e * node_stride * 2;
    for (int s = P >> 1; s >= 1; s >>= 1) {
        for (int i = s + threadIdx.x; i < 2 * s; i += blockDim.x) {
            const float4 a = ne[4 * i], b = ne[4 * i + 2], A = ne[4 * i + 1], B = ne[4 * i + 3];
            ne[2 * i] = make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), 0.0f);
            ne[2 * i + 1] = make_float4(fmaxf(A.x, B.x), fmaxf(A.y, B.y), fmaxf(A.z, B.z), 0.0f);
        }
        __syncthreads();
    }
}

// k_nn_sqdist's pair formula, dx = q.x - y.x
__device__ __forceinline__ float pair_d(float qx, float qy, float qz, float4 y)
{
    const float dx = qx - y.x, dy = qy - y.y, dz = qz - y.z;
    return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
}

__device__ __forceinline__ float box_lb(float qx, float qy, float qz, const float4 *__restrict__ nd, int i)
{
    const float4 lo = nd[2 * i], hi = nd[2 * i + 1];
    const float dx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.0f), dy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.0f),
                dz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.0f);
    return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
}

__device__ __forceinline__ float leaf_min(float qx, float qy, float qz, const float4 *__restrict__ pts, int n, int leaf, float best)
{
    const int hi = min(n, (leaf + 1) * kLeaf);
    for (int j = leaf * kLeaf; j < hi; ++j) best = fminf(best, pair_d(qx, qy, qz, pts[j]));
    return best;
}

// Exact nearest squared distance of q to the tree's points.  A box is skipped only when its bound lb satisfies
// lb > best (1 + 2^-20) and lb > 2^-100: the computed pair value of any point in it then exceeds best (the bound and the
// pair formula each lose at most ~5 ulps relative; 2^-100 keeps underflowing terms out of the argument).
__device__ float nn_tree(float qx, float qy, float qz, const float4 *__restrict__ pts, int n, const float4 *__restrict__ nd, int P)
{
    int i = 1;  // greedy descent to a first candidate leaf
    while (i < P) {
        const float a = box_lb(qx, qy, qz, nd, 2 * i), b = box_lb(qx, qy, qz, nd, 2 * i + 1);
        i = b < a ? 2 * i + 1 : 2 * i;
    }
    float best = leaf_min(qx, qy, qz, pts, n, i - P, FLT_MAX);
    const int greedy = i - P;
    i = 1;  // stackless depth-first walk of the implicit tree
    while (true) {
        bool down = false;
        const float lb = box_lb(qx, qy, qz, nd, i);
        if (!(lb > __fmaf_rn(best, 0x1p-20f, best)) || !(lb > 0x1p-100f)) {
            if (i >= P) {
                if (i - P != greedy) best = leaf_min(qx, qy, qz, pts, n, i - P, best);
            } else {
                i = 2 * i;
                down = true;
            }
        }
        if (!down) {
            while (i & 1) i >>= 1;
            if (i == 0) break;
            ++i;
        }
    }
    return best;
}

// scanned -> GT: dx[e][i] for the env's unique points in sorted order
__global__ __launch_bounds__(256) void k_nn_x2gt(const float4 *__restrict__ xpts, int64_t cap, const int32_t *__restrict__ counts,
                                               const int32_t *__restrict__ active, const int64_t *__restrict__ gt_start,
                                               const float4 *__restrict__ gt_pts, const int64_t *__restrict__ gt_node_start,
                                               const int32_t *__restrict__ gt_pow2, const float4 *__restrict__ gt_nodes, float *__restrict__ dx)
{
    const int e = blockIdx.y;
    if (!active[e]) return;
    const int n = counts[e];
    const int64_t g0 = gt_start[e];
    const int m = (int)(gt_start[e + 1] - g0), P = gt_pow2[e];
    const float4 *yp = gt_pts + g0, *nd = gt_nodes + 2 * gt_node_start[e];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 q = xpts[(size_t)e * cap + i];
        dx[(size_t)e * cap + i] = nn_tree(q.x, q.y, q.z, yp, m, nd, P);
    }
}

// GT -> scanned: dy[gt_start[e] + orig[j]], queries in the GT cloud's sorted (spatially coherent) order
__global__ __launch_bounds__(256) void k_nn_gt2x(const float4 *__restrict__ xpts, int64_t cap, const int32_t *__restrict__ counts,
                                               const int32_t *__restrict__ active, const float4 *__restrict__ xnodes, int64_t node_stride,
                                               const int64_t *__restrict__ gt_start, const float4 *__restrict__ gt_pts,
                                               const int32_t *__restrict__ gt_orig, float *__restrict__ dy)
{
    const int e = blockIdx.y;
    if (!active[e]) return;
    const int n = counts[e], P = tree_pow2((n + kLeaf - 1) / kLeaf);
    const int64_t g0 = gt_start[e];
    const int m = (int)(gt_start[e + 1] - g0);
    const float4 *xp = xpts + (size_t)e * cap, *nd = xnodes + (size_t)e * node_stride * 2;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const float4 q = gt_pts[g0 + j];
        dy[g0 + gt_orig[g0 + j]] = nn_tree(q.x, q.y, q.z, xp, n, nd, P);
    }
}

// k_sum_f64 per env and side (blockIdx.z: 0 = scanned, 1 = GT), grid (512, N, 2)
__global__ __launch_bounds__(256) void k_score_sum(const float *__restrict__ dx, int64_t cap, const int32_t *__restrict__ counts,
                                                 const int32_t *__restrict__ active, const float *__restrict__ dy,
                                                 const int64_t *__restrict__ gt_start, double *__restrict__ partial)
{
    const int e = blockIdx.y, side = blockIdx.z;
    if (!active[e]) return;
    const float *v = side == 0 ? dx + (size_t)e * cap : dy + gt_start[e];
    const int64_t n = side == 0 ? (int64_t)counts[e] : gt_start[e + 1] - gt_start[e];
    __shared__ double s[256];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += (double)v[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[((size_t)e * 2 + side) * kSumBlocks + blockIdx.x] = s[0];
}

// k_chamfer_finish per env, then x 100.0f (reconstruction_accuracy_cm); grid N
__global__ __launch_bounds__(256) void k_score_finish(const int32_t *__restrict__ counts, const int32_t *__restrict__ active,
                                                    const int64_t *__restrict__ gt_start, const double *__restrict__ partial,
                                                    float *__restrict__ acc, int32_t *__restrict__ scored)
{
    const int e = blockIdx.x;
    if (!active[e]) return;
    const double *px = partial + (size_t)e * 2 * kSumBlocks, *py = px + kSumBlocks;
    __shared__ double s[2][256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < kSumBlocks; i += 256) a += px[i];
    for (int i = threadIdx.x; i < kSumBlocks; i += 256) b += py[i];
    s[0][threadIdx.x] = a;
    s[1][threadIdx.x] = b;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            s[0][threadIdx.x] += s[0][threadIdx.x + d];
            s[1][threadIdx.x] += s[1][threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double nx = (double)counts[e], ny = (double)(gt_start[e + 1] - gt_start[e]);
        acc[e] = __fmul_rn((float)(s[0][0] / nx + s[1][0] / ny), 100.0f);
        scored[e] = 1;
    }
}

// export: env's Morton codes -> packed keys (x << 42 | y << 21 | z, the order of unique_rounded_points), and back
__global__ __launch_bounds__(256) void k_export_prep(const uint64_t *__restrict__ list, const int32_t *__restrict__ count,
                                                   uint64_t *__restrict__ out, int32_t *__restrict__ active)
{
    const int n = *count;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int k[3];
        unmorton(list[i], k);
        out[i] = (uint64_t)(k[0] + kKeyOffset) << (2 * kKeyBits) | (uint64_t)(k[1] + kKeyOffset) << kKeyBits | (uint64_t)(k[2] + kKeyOffset);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *active = n > 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_export_write(const uint64_t *__restrict__ keys, const int32_t *__restrict__ count,
                                                    float *__restrict__ xyz)
{
    const int n = *count;
    const uint64_t mask = (1ull << kKeyBits) - 1;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t c = keys[i];
        xyz[3 * (size_t)i + 0] = key_to_coord((int)((c >> (2 * kKeyBits)) & mask) - kKeyOffset);
        xyz[3 * (size_t)i + 1] = key_to_coord((int)((c >> kKeyBits) & mask) - kKeyOffset);
        xyz[3 * (size_t)i + 2] = key_to_coord((int)(c & mask) - kKeyOffset);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct ScoreLayout {
    int tmax, pmax;
    size_t off_b, off_pts, off_nodes, off_dx, off_dy, off_hist, off_partial, off_active, total;
};

ScoreLayout score_layout(int n, int64_t cap, int64_t gt_points)
{
    ScoreLayout L;
    L.tmax = (int)((cap + kSortTile - 1) / kSortTile);
    int leaves = (int)((cap + kLeaf - 1) / kLeaf), p = 1;
    while (p < leaves) p <<= 1;
    L.pmax = p;
    size_t o = 0;
    L.off_b = o;       o = align256(o + (size_t)n * cap * 8);
    L.off_pts = o;     o = align256(o + (size_t)n * cap * 16);
    L.off_nodes = o;   o = align256(o + (size_t)n * 2 * L.pmax * 32);
    L.off_dx = o;      o = align256(o + (size_t)n * cap * 4);
    L.off_dy = o;      o = align256(o + (size_t)gt_points * 4);
    L.off_hist = o;    o = align256(o + (size_t)n * 16 * L.tmax * 4);
    L.off_partial = o; o = align256(o + (size_t)n * 2 * kSumBlocks * 8);
    L.off_active = o;  o = align256(o + (size_t)n * 4);
    L.total = o;
    return L;
}

int blocks_per_env(int n) { return max(4, min(256, (4096 + n - 1) / n)); }

bool set_ok(const GnbvScanSet *s)
{
    return s && s->n > 0 && s->capacity >= 64 && s->capacity % 64 == 0 && s->capacity < (int64_t)1 << 31 && s->table && s->keys &&
           s->counts && s->flags;
}

// sorts keys [e * stride, + counts[e]) of the active envs in place (16 passes: the result ends where it started)
int radix_sort(uint64_t *a, uint64_t *b, int64_t stride, int n, const int32_t *counts, const int32_t *active, uint32_t *hist, int tmax,
               hipStream_t st)
{
    const dim3 grid(blocks_per_env(n), n);
    for (int pass = 0; pass < kSortPasses; ++pass) {
        const int shift = 4 * pass;
        hipLaunchKernelGGL(k_radix_hist, grid, dim3(kSortThreads), 0, st, (const uint64_t *)a, stride, counts, active, shift, hist, tmax);
        hipLaunchKernelGGL(k_radix_scan, dim3(n), dim3(256), 0, st, counts, active, hist, tmax);
        hipLaunchKernelGGL(k_radix_scatter, grid, dim3(kSortThreads), 0, st, (const uint64_t *)a, b, stride, counts, active, shift,
                           (const uint32_t *)hist, tmax);
        uint64_t *t = a;
        a = b;
        b = t;
    }
    return gnbv_launch_status();
}

}  // namespace

GNBV_API size_t gnbv_scan_set_bytes(int n, int64_t capacity)
{
    if (n <= 0 || capacity <= 0) return 0;
    return (size_t)n * capacity * 16 + (size_t)n * 8;
}

GNBV_API int gnbv_scan_add_frame(const GnbvScanSet *set, const float *depth_raw, const float *seg_raw, const float *c2w,
                                 const float *inv_intri, int h, int w, float depth_sense_dist, void *stream)
{
    GNBV_CHECK_ARG(set_ok(set) && depth_raw && seg_raw && c2w && inv_intri && h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31));
    Intrinsics K;
    for (int i = 0; i < 9; ++i) K.k[i] = inv_intri[i];
    const dim3 grid((unsigned)((h * w + 255) / 256), set->n);
    hipLaunchKernelGGL(k_scan_add, grid, dim3(256), 0, gnbv_stream(stream), depth_raw, seg_raw, c2w, K, h, w, depth_sense_dist,
                       set->capacity, set->table, set->keys, set->counts, set->flags);
    return gnbv_launch_status();
}

GNBV_API int gnbv_scan_clear(const GnbvScanSet *set, const uint8_t *mask, void *stream)
{
    GNBV_CHECK_ARG(set_ok(set) && mask);
    const int64_t per = (set->capacity / 2 + 255) / 256;
    const dim3 grid((unsigned)(per < blocks_per_env(set->n) ? per : blocks_per_env(set->n)), set->n);
    hipLaunchKernelGGL(k_scan_clear, grid, dim3(256), 0, gnbv_stream(stream), mask, set->capacity, set->table, set->counts);
    return gnbv_launch_status();
}

GNBV_API size_t gnbv_scan_workspace_bytes(int n, int64_t capacity, int64_t gt_points)
{
    if (n <= 0 || capacity <= 0 || gt_points < 0) return 0;
    return score_layout(n, capacity, gt_points).total;
}

GNBV_API int gnbv_scan_score(const GnbvScanSet *set, const GnbvScanGt *gt, const uint8_t *mask, float *accuracy, int32_t *scored,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    GNBV_CHECK_ARG(set_ok(set) && gt && gt->n == set->n && gt->num_points > 0 && gt->pt_start && gt->pts && gt->orig && gt->node_start &&
                   gt->pow2 && gt->nodes && mask && accuracy && scored && workspace && ((uintptr_t)workspace & 255) == 0);
    const int n = set->n;
    const int64_t cap = set->capacity;
    const ScoreLayout L = score_layout(n, cap, gt->num_points);
    GNBV_CHECK_ARG(workspace_bytes >= L.total);
    hipStream_t st = gnbv_stream(stream);
    char *ws = (char *)workspace;
    uint64_t *b = (uint64_t *)(ws + L.off_b);
    float4 *pts = (float4 *)(ws + L.off_pts), *nodes = (float4 *)(ws + L.off_nodes);
    float *dx = (float *)(ws + L.off_dx), *dy = (float *)(ws + L.off_dy);
    uint32_t *hist = (uint32_t *)(ws + L.off_hist);
    double *partial = (double *)(ws + L.off_partial);
    int32_t *active = (int32_t *)(ws + L.off_active);
    const int64_t node_stride = 2 * (int64_t)L.pmax;  // heap nodes per env (two float4 each)
    hipLaunchKernelGGL(k_score_prep, dim3((n + 255) / 256), dim3(256), 0, st, mask, (const int32_t *)scored, (const int32_t *)set->counts,
                       (const int32_t *)set->flags, n, active);
    int err;
    if ((err = radix_sort(set->keys, b, cap, n, set->counts, active, hist, L.tmax, st))) return err;
    const dim3 grid(blocks_per_env(n), n);
    hipLaunchKernelGGL(k_x_points, grid, dim3(256), 0, st, (const uint64_t *)set->keys, cap, (const int32_t *)set->counts,
                       (const int32_t *)active, pts, nodes, node_stride);
    hipLaunchKernelGGL(k_x_levels, dim3(n), dim3(1024), 0, st, (const int32_t *)set->counts, (const int32_t *)active, nodes, node_stride);
    hipLaunchKernelGGL(k_nn_x2gt, grid, dim3(256), 0, st, (const float4 *)pts, cap, (const int32_t *)set->counts, (const int32_t *)active,
                       gt->pt_start, (const float4 *)gt->pts, gt->node_start, gt->pow2, (const float4 *)gt->nodes, dx);
    hipLaunchKernelGGL(k_nn_gt2x, grid, dim3(256), 0, st, (const float4 *)pts, cap, (const int32_t *)set->counts, (const int32_t *)active,
                       (const float4 *)nodes, node_stride, gt->pt_start, (const float4 *)gt->pts, gt->orig, dy);
    hipLaunchKernelGGL(k_score_sum, dim3(kSumBlocks, n, 2), dim3(256), 0, st, (const float *)dx, cap, (const int32_t *)set->counts,
                       (const int32_t *)active, (const float *)dy, gt->pt_start, partial);
    hipLaunchKernelGGL(k_score_finish, dim3(n), dim3(256), 0, st, (const int32_t *)set->counts, (const int32_t *)active, gt->pt_start,
                       (const double *)partial, accuracy, scored);
    return gnbv_launch_status();
}

GNBV_API int gnbv_scan_export(const GnbvScanSet *set, int env, float *xyz, void *workspace, size_t workspace_bytes, void *stream)
{
    GNBV_CHECK_ARG(set_ok(set) && env >= 0 && env < set->n && xyz && workspace && ((uintptr_t)workspace & 255) == 0);
    const int64_t cap = set->capacity;
    const ScoreLayout L = score_layout(1, cap, 0);
    GNBV_CHECK_ARG(workspace_bytes >= L.total);
    hipStream_t st = gnbv_stream(stream);
    char *ws = (char *)workspace;
    uint64_t *b = (uint64_t *)(ws + L.off_b), *a = (uint64_t *)(ws + L.off_pts);  // the points region holds the keys here
    uint32_t *hist = (uint32_t *)(ws + L.off_hist);
    int32_t *active = (int32_t *)(ws + L.off_active);
    const int32_t *count = set->counts + env;
    const int blocks = blocks_per_env(1);
    hipLaunchKernelGGL(k_export_prep, dim3(blocks), dim3(256), 0, st, (const uint64_t *)(set->keys + (size_t)env * cap), count, a, active);
    int err;
    if ((err = radix_sort(a, b, cap, 1, count, active, hist, L.tmax, st))) return err;
    hipLaunchKernelGGL(k_export_write, dim3(blocks), dim3(256), 0, st, (const uint64_t *)a, count, xyz);
    return gnbv_launch_status();
}

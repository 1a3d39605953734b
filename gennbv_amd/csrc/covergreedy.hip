// covergreedy.hip -- greedy set cover over per-candidate bit masks, on MI355X.
//
// "Which of the env's K cached views adds the most ground-truth voxels to the covered set, T times in a row?"  (DESIGN.md "View
// pool: cached visibility masks and the greedy set-cover planner"; include/gennbv_hip.h gnbv_cover_greedy has the exact
// definition.)  The masks are gnbv_view_cover_masks' rows; everything is integer, so there is one right answer.
//
//   k_cg_gains    round 0, exhaustive: one wave per (env, candidate), 16 bytes of mask and of the env's covered row per lane
//                 and trip (the row is L2-resident: an env's workgroups run on one XCD), __popc, a wave reduction, lane 0
//                 stores the gain.  HBM-bound: n k words 4 bytes.  Launched when gains0 is wanted, or lazy == 0 with a ub row.
//   k_cg_rounds   one workgroup per env, one wave per candidate evaluation.  The bounds, the round each bound was refreshed in
//                 and the contacts live in LDS; the covered row lives in covered_out (global: 256 KiB at 128^3 does not fit
//                 the LDS), which this workgroup alone touches: barrier + __threadfence_block() between the OR of the winner
//                 and the next round's reads.  Per round, passes of
//                   a. every wave scans its share of the candidates (j = wave, wave + waves, ...) for its largest key among
//                      the candidates refreshed this round ("fresh") and among the others ("stale");
//                   b. barrier; every lane takes the two maxima over the waves.  The largest fresh key above every stale
//                      key: that candidate wins (a stale bound is >= its true gain, so nothing can overtake it);
//                   c. else every wave whose stale top lies above the best fresh key refreshes it (the others cannot win this
//                      round); barrier; again.
//                 The overall top is refreshed in every pass, so a round ends after at most ceil(k / waves) + 1 passes.  Which
//                 further stale candidates a pass refreshes changes the work, never the result: a refresh only replaces a
//                 bound by the exact gain.  lazy == 0 refreshes every candidate at the start of every round instead.
//                 key = (score + 1) k + (k - 1 - j) in 64 bits: unique per candidate, larger for the lower j at equal score.
//   k_cgw_gains<P>, k_cgw_rounds<P>   gnbv_cover_greedy_w: the same pair over P = 1..4 planes of masks with a weighted score
//                 (further down; k_cg_gains and k_cg_rounds are left as they were).
// No global atomics; every output element is stored once per call; no host synchronisation, no allocation.
#include "common.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kCgMaxK = 4096;
constexpr int kCgMaxRounds = 4096;
constexpr int kCgMaxWaves = 16;
constexpr int kCgGainWaves = 4;  // candidates per workgroup of k_cg_gains
constexpr int kCgUnknown = 0x7fffffff;

struct CgParams {
    int n, k, words, rounds, lazy, exact0;
    const uint32_t *mask;
    const uint32_t *cov_in;
    const uint8_t *contact;
    int32_t *choice, *gain;
    uint32_t *cov_out;
    int32_t *gains0, *ub;
};

// popcount(mask row & ~covered row) over n4 16-byte groups, summed over the wave: the same value in every lane
__device__ __forceinline__ int wave_gain(const uint32_t *m, const uint32_t *c, int n4, int lane)
{
    const uint4 *m4 = reinterpret_cast<const uint4 *>(m);
    const uint4 *c4 = reinterpret_cast<const uint4 *>(c);
    int s = 0;
    for (int i = lane; i < n4; i += kWave) {
        const uint4 a = m4[i];
        const uint4 b = c != nullptr ? c4[i] : make_uint4(0u, 0u, 0u, 0u);
        s += __popc(a.x & ~b.x) + __popc(a.y & ~b.y) + __popc(a.z & ~b.z) + __popc(a.w & ~b.w);
    }
    return __shfl(wave_reduce_sum(s), 0, kWave);
}

__global__ __launch_bounds__(kCgGainWaves * kWave) void k_cg_gains(CgParams p)
{
    // XCD-aware block -> (env, group of candidates): all workgroups of an env run on one XCD (viewcover.hip k_view_cover)
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
    const int per_env = (p.k + kCgGainWaves - 1) / kCgGainWaves;
    const int e = (slot / per_env) * 8 + xcd;
    const int lane = threadIdx.x & (kWave - 1);
    const int j = (slot % per_env) * kCgGainWaves + (int)threadIdx.x / kWave;
    if (e >= p.n || j >= p.k) return;
    const uint32_t *cov = p.cov_in != nullptr ? p.cov_in + (size_t)e * p.words : nullptr;
    const int g = wave_gain(p.mask + ((size_t)e * p.k + j) * p.words, cov, p.words / 4, lane);
    if (lane == 0) {
        if (p.gains0 != nullptr) p.gains0[(size_t)e * p.k + j] = g;
        if (p.ub != nullptr) p.ub[(size_t)e * p.k + j] = g;  // (lazy == 0 without gains0: k_cg_rounds reads them back)
    }
}

__global__ __launch_bounds__(kCgMaxWaves * kWave) void k_cg_rounds(CgParams p)
{
    __shared__ int s_ub[kCgMaxK];          // upper bound of the gain; exact where s_at == round + 1
    __shared__ int s_at[kCgMaxK];          // 1 + the round the bound was refreshed in, 0 = never
    __shared__ uint8_t s_contact[kCgMaxK];
    __shared__ long long s_fresh[kCgMaxWaves], s_stale[kCgMaxWaves];

    const int e = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = tid / kWave, nwaves = nthreads / kWave, lane = tid & (kWave - 1);
    const int k = p.k, n4 = p.words / 4;
    const uint32_t *mask = p.mask + (size_t)e * k * p.words;
    // the covered row this workgroup reads and grows: covered_out when there is one (rounds == 1 may go without)
    uint32_t *cov_out = p.cov_out != nullptr ? p.cov_out + (size_t)e * p.words : nullptr;
    const uint32_t *cov_in = p.cov_in != nullptr ? p.cov_in + (size_t)e * p.words : nullptr;
    const uint32_t *cov = cov_out != nullptr ? cov_out : cov_in;

    // bounds: the exact round-0 gains of k_cg_gains, the caller's bounds, or unknown
    const int32_t *src = p.exact0 ? (p.gains0 != nullptr ? p.gains0 : p.ub) : (p.lazy ? p.ub : nullptr);
    for (int j = tid; j < k; j += nthreads) {
        const int u = src != nullptr ? src[(size_t)e * k + j] : kCgUnknown;
        s_ub[j] = u < 0 ? 0 : u;  // (keys stay >= 0 whatever the caller's row holds)
        s_at[j] = p.exact0 ? 1 : 0;
        s_contact[j] = p.contact != nullptr ? p.contact[(size_t)e * k + j] : 0;
    }
    if (cov_out != nullptr && cov_out != cov_in) {
        uint4 *o4 = reinterpret_cast<uint4 *>(cov_out);
        const uint4 *i4 = reinterpret_cast<const uint4 *>(cov_in);
        for (int i = tid; i < n4; i += nthreads) o4[i] = cov_in != nullptr ? i4[i] : make_uint4(0u, 0u, 0u, 0u);
    }
    __threadfence_block();
    __syncthreads();

    for (int t = 0; t < p.rounds; ++t) {
        const int now = t + 1;
        if (!p.lazy && !(t == 0 && p.exact0)) {  // exhaustive: every candidate, every round
            for (int j = wave; j < k; j += nwaves) {
                const int g = wave_gain(mask + (size_t)j * p.words, cov, n4, lane);
                if (lane == 0) {
                    s_ub[j] = g;
                    s_at[j] = now;
                }
            }
            __syncthreads();
        }
        long long win;
        for (;;) {
            // ---- a. this wave's largest fresh and stale keys
            long long kf = -1, ks = -1;
            for (int j = wave + nwaves * lane; j < k; j += nwaves * kWave) {
                const long long score = s_contact[j] != 0 ? -1ll : (long long)s_ub[j];
                const long long key = (score + 1) * k + (k - 1 - j);
                if (s_at[j] == now) kf = key > kf ? key : kf;
                else ks = key > ks ? key : ks;
            }
            kf = wave_max_all(kf);
            ks = wave_max_all(ks);
            if (lane == 0) {
                s_fresh[wave] = kf;
                s_stale[wave] = ks;
            }
            __syncthreads();
            // ---- b. the two maxima over the waves
            long long gf = -1, gs = -1;
            for (int w = 0; w < nwaves; ++w) {
                gf = s_fresh[w] > gf ? s_fresh[w] : gf;
                gs = s_stale[w] > gs ? s_stale[w] : gs;
            }
            if (gf > gs) {  // (keys are distinct and k >= 1: one of the two is a candidate's)
                win = gf;
                break;
            }
            // ---- c. refresh this wave's stale top if it can still win
            if (ks > gf) {
                const int j = k - 1 - (int)(ks % k);
                const int g = wave_gain(mask + (size_t)j * p.words, cov, n4, lane);
                if (lane == 0) {
                    s_ub[j] = g;
                    s_at[j] = now;
                }
            }
            __syncthreads();  // bounds written; s_fresh / s_stale read by every lane
        }
        const int jw = k - 1 - (int)(win % k);
        if (tid == 0) {
            p.choice[(size_t)e * p.rounds + t] = jw;
            p.gain[(size_t)e * p.rounds + t] = s_ub[jw];  // refreshed this round: the true gain, also of a contact winner
        }
        if (cov_out != nullptr) {
            uint4 *o4 = reinterpret_cast<uint4 *>(cov_out);
            const uint4 *m4 = reinterpret_cast<const uint4 *>(mask + (size_t)jw * p.words);
            for (int i = tid; i < n4; i += nthreads) {
                const uint4 a = o4[i], m = m4[i];
                o4[i] = make_uint4(a.x | m.x, a.y | m.y, a.z | m.z, a.w | m.w);
            }
        }
        __threadfence_block();
        __syncthreads();  // the covered row is complete; s_fresh / s_stale and s_ub[jw] were read
    }
    if (p.ub != nullptr)  // exact or stale, every bound is >= the gain against covered_out
        for (int j = tid; j < k; j += nthreads) p.ub[(size_t)e * k + j] = s_ub[j];
}

// ---- the weighted form over P planes (gnbv_cover_greedy_w): the same two kernels with P mask rows and P covered rows per
// candidate evaluation and one weighted score per candidate.  The bounds, the keys and the fresh / stale passes are those above
// on the score; the per-plane gains of the winner come from the pass that ORs its rows into the covered rows.
constexpr int kCgMaxPlanes = 4;

struct CgwParams {
    int n, k, words, rounds, lazy, exact0;
    int weight[kCgMaxPlanes];
    const uint32_t *mask[kCgMaxPlanes];
    const uint32_t *cov_in[kCgMaxPlanes];
    uint32_t *cov_out[kCgMaxPlanes];
    const uint8_t *contact;
    int32_t *choice, *gain, *plane_gain;
    int32_t *gains0, *ub;
};

// sum over the planes of weight_p popcount(mask_p row & ~covered_p row): P rows of n4 16-byte groups in one trip, the popcounts
// kept per plane and multiplied once after the trip; the same value in every lane.
template <int P>
__device__ __forceinline__ int wave_score(const CgwParams &p, size_t row, const uint32_t *const *cov, int n4, int lane)
{
    const uint4 *m4[P], *c4[P];
    int s[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        m4[q] = reinterpret_cast<const uint4 *>(p.mask[q] + row);
        c4[q] = reinterpret_cast<const uint4 *>(cov[q]);
        s[q] = 0;
    }
    bool all_cov = true;
#pragma unroll
    for (int q = 0; q < P; ++q) all_cov = all_cov && c4[q] != nullptr;
    // every load of a trip is issued before the first popcount waits for one: no branch between them
    if (all_cov) {
        for (int i = lane; i < n4; i += kWave) {
            uint4 a[P], b[P];
#pragma unroll
            for (int q = 0; q < P; ++q) a[q] = m4[q][i];
#pragma unroll
            for (int q = 0; q < P; ++q) b[q] = c4[q][i];
#pragma unroll
            for (int q = 0; q < P; ++q)
                s[q] += __popc(a[q].x & ~b[q].x) + __popc(a[q].y & ~b[q].y) + __popc(a[q].z & ~b[q].z) + __popc(a[q].w & ~b[q].w);
        }
    } else {
        for (int i = lane; i < n4; i += kWave) {
            uint4 a[P];
#pragma unroll
            for (int q = 0; q < P; ++q) a[q] = m4[q][i];
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const uint4 b = c4[q] != nullptr ? c4[q][i] : make_uint4(0u, 0u, 0u, 0u);
                s[q] += __popc(a[q].x & ~b.x) + __popc(a[q].y & ~b.y) + __popc(a[q].z & ~b.z) + __popc(a[q].w & ~b.w);
            }
        }
    }
    int v = 0;
#pragma unroll
    for (int q = 0; q < P; ++q) v += p.weight[q] * s[q];  // (the sum over the wave fits: sum_p weight_p 32 words <= INT32_MAX)
    return __shfl(wave_reduce_sum(v), 0, kWave);
}

template <int P>
__global__ __launch_bounds__(kCgGainWaves * kWave) void k_cgw_gains(CgwParams p)
{
    // the block -> (env, group of candidates) mapping of k_cg_gains: all workgroups of an env run on one XCD
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
    const int per_env = (p.k + kCgGainWaves - 1) / kCgGainWaves;
    const int e = (slot / per_env) * 8 + xcd;
    const int lane = threadIdx.x & (kWave - 1);
    const int j = (slot % per_env) * kCgGainWaves + (int)threadIdx.x / kWave;
    if (e >= p.n || j >= p.k) return;
    const uint32_t *cov[P];
#pragma unroll
    for (int q = 0; q < P; ++q) cov[q] = p.cov_in[q] != nullptr ? p.cov_in[q] + (size_t)e * p.words : nullptr;
    const int g = wave_score<P>(p, ((size_t)e * p.k + j) * p.words, cov, p.words / 4, lane);
    if (lane == 0) {
        if (p.gains0 != nullptr) p.gains0[(size_t)e * p.k + j] = g;
        if (p.ub != nullptr) p.ub[(size_t)e * p.k + j] = g;
    }
}

template <int P>
__global__ __launch_bounds__(kCgMaxWaves * kWave) void k_cgw_rounds(CgwParams p)
{
    __shared__ int s_ub[kCgMaxK];          // upper bound of the score; exact where s_at == round + 1
    __shared__ int s_at[kCgMaxK];          // 1 + the round the bound was refreshed in, 0 = never
    __shared__ uint8_t s_contact[kCgMaxK];
    __shared__ long long s_fresh[kCgMaxWaves], s_stale[kCgMaxWaves];
    __shared__ int s_pg[kCgMaxWaves][kCgMaxPlanes];  // the winner's plane gains, one partial sum per wave

    const int e = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = tid / kWave, nwaves = nthreads / kWave, lane = tid & (kWave - 1);
    const int k = p.k, n4 = p.words / 4;
    const size_t env_row = (size_t)e * k * p.words;
    // the covered rows this workgroup reads and grows: covered_out where there is one (rounds == 1 may go without)
    uint32_t *cov_out[P];
    const uint32_t *cov[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        cov_out[q] = p.cov_out[q] != nullptr ? p.cov_out[q] + (size_t)e * p.words : nullptr;
        const uint32_t *cov_in = p.cov_in[q] != nullptr ? p.cov_in[q] + (size_t)e * p.words : nullptr;
        cov[q] = cov_out[q] != nullptr ? cov_out[q] : cov_in;
        if (cov_out[q] != nullptr && cov_out[q] != cov_in) {
            uint4 *o4 = reinterpret_cast<uint4 *>(cov_out[q]);
            const uint4 *i4 = reinterpret_cast<const uint4 *>(cov_in);
            for (int i = tid; i < n4; i += nthreads) o4[i] = cov_in != nullptr ? i4[i] : make_uint4(0u, 0u, 0u, 0u);
        }
    }

    // bounds: the exact round-0 scores of k_cgw_gains, the caller's bounds, or unknown
    const int32_t *src = p.exact0 ? (p.gains0 != nullptr ? p.gains0 : p.ub) : (p.lazy ? p.ub : nullptr);
    for (int j = tid; j < k; j += nthreads) {
        const int u = src != nullptr ? src[(size_t)e * k + j] : kCgUnknown;
        s_ub[j] = u < 0 ? 0 : u;  // (keys stay >= 0 whatever the caller's row holds)
        s_at[j] = p.exact0 ? 1 : 0;
        s_contact[j] = p.contact != nullptr ? p.contact[(size_t)e * k + j] : 0;
    }
    __threadfence_block();
    __syncthreads();

    for (int t = 0; t < p.rounds; ++t) {
        const int now = t + 1;
        if (!p.lazy && !(t == 0 && p.exact0)) {  // exhaustive: every candidate, every round
            for (int j = wave; j < k; j += nwaves) {
                const int g = wave_score<P>(p, env_row + (size_t)j * p.words, cov, n4, lane);
                if (lane == 0) {
                    s_ub[j] = g;
                    s_at[j] = now;
                }
            }
            __syncthreads();
        }
        long long win;
        for (;;) {
            // ---- a. this wave's largest fresh and stale keys
            long long kf = -1, ks = -1;
            for (int j = wave + nwaves * lane; j < k; j += nwaves * kWave) {
                const long long score = s_contact[j] != 0 ? -1ll : (long long)s_ub[j];
                const long long key = (score + 1) * k + (k - 1 - j);
                if (s_at[j] == now) kf = key > kf ? key : kf;
                else ks = key > ks ? key : ks;
            }
            kf = wave_max_all(kf);
            ks = wave_max_all(ks);
            if (lane == 0) {
                s_fresh[wave] = kf;
                s_stale[wave] = ks;
            }
            __syncthreads();
            // ---- b. the two maxima over the waves
            long long gf = -1, gs = -1;
            for (int w = 0; w < nwaves; ++w) {
                gf = s_fresh[w] > gf ? s_fresh[w] : gf;
                gs = s_stale[w] > gs ? s_stale[w] : gs;
            }
            if (gf > gs) {  // (keys are distinct and k >= 1: one of the two is a candidate's)
                win = gf;
                break;
            }
            // ---- c. refresh this wave's stale top if it can still win
            if (ks > gf) {
                const int j = k - 1 - (int)(ks % k);
                const int g = wave_score<P>(p, env_row + (size_t)j * p.words, cov, n4, lane);
                if (lane == 0) {
                    s_ub[j] = g;
                    s_at[j] = now;
                }
            }
            __syncthreads();  // bounds written; s_fresh / s_stale read by every lane
        }
        const int jw = k - 1 - (int)(win % k);
        if (tid == 0) {
            p.choice[(size_t)e * p.rounds + t] = jw;
            p.gain[(size_t)e * p.rounds + t] = s_ub[jw];  // refreshed this round: the true score, also of a contact winner
        }
        // the winner's rows into the covered rows; popcount(m & ~a) before the OR is its gain in that plane
        int pg[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            pg[q] = 0;
            if (cov_out[q] == nullptr && p.plane_gain == nullptr) continue;
            uint4 *o4 = reinterpret_cast<uint4 *>(cov_out[q]);
            const uint4 *a4 = reinterpret_cast<const uint4 *>(cov[q]);
            const uint4 *m4 = reinterpret_cast<const uint4 *>(p.mask[q] + env_row + (size_t)jw * p.words);
            for (int i = tid; i < n4; i += nthreads) {
                const uint4 a = a4 != nullptr ? a4[i] : make_uint4(0u, 0u, 0u, 0u), m = m4[i];
                pg[q] += __popc(m.x & ~a.x) + __popc(m.y & ~a.y) + __popc(m.z & ~a.z) + __popc(m.w & ~a.w);
                if (o4 != nullptr) o4[i] = make_uint4(a.x | m.x, a.y | m.y, a.z | m.z, a.w | m.w);
            }
        }
        if (p.plane_gain != nullptr) {
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const int v = wave_reduce_sum(pg[q]);
                if (lane == 0) s_pg[wave][q] = v;
            }
        }
        __threadfence_block();
        __syncthreads();  // the covered rows are complete; s_fresh / s_stale and s_ub[jw] were read; s_pg is written
        if (p.plane_gain != nullptr && tid < P) {  // (s_pg is written again only after the next round's first barrier)
            int v = 0;
            for (int w = 0; w < nwaves; ++w) v += s_pg[w][tid];
            p.plane_gain[((size_t)e * p.rounds + t) * P + tid] = v;
        }
    }
    if (p.ub != nullptr)  // exact or stale, every bound is >= the score against covered_out
        for (int j = tid; j < k; j += nthreads) p.ub[(size_t)e * k + j] = s_ub[j];
}

template <int P>
void cgw_launch(const CgwParams &p, hipStream_t st)
{
    if (p.exact0) {
        CgwParams q = p;
        if (p.gains0 != nullptr) q.ub = nullptr;  // ub is this pass's output only where there is no gains0 row to hold the scores
        const int64_t blocks = (int64_t)((p.n + 7) / 8 * 8) * ((p.k + kCgGainWaves - 1) / kCgGainWaves);
        hipLaunchKernelGGL(k_cgw_gains<P>, dim3((unsigned)blocks), dim3(kCgGainWaves * kWave), 0, st, q);
    }
    const int waves = p.k < kCgMaxWaves ? p.k : kCgMaxWaves;
    hipLaunchKernelGGL(k_cgw_rounds<P>, dim3((unsigned)p.n), dim3(waves * kWave), 0, st, p);
}

}  // namespace

GNBV_API int gnbv_cover_greedy_w(const GnbvCoverGreedyW *args, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvCoverGreedyW a = *args;
    GNBV_CHECK_ARG(a.n >= 1 && a.n <= 65535 && a.k >= 1 && a.k <= kCgMaxK && a.rounds >= 1 && a.rounds <= kCgMaxRounds);
    GNBV_CHECK_ARG(a.words >= 4 && (a.words & 3) == 0 && a.words <= (1 << 25) && (a.lazy == 0 || a.lazy == 1));
    GNBV_CHECK_ARG(a.planes >= 1 && a.planes <= kCgMaxPlanes);
    GNBV_CHECK_ARG(a.choice != nullptr && a.gain != nullptr);
    CgwParams p = {};
    int64_t weights = 0;
    for (int q = 0; q < a.planes; ++q) {
        GNBV_CHECK_ARG(a.weight[q] >= 0 && a.mask_bits[q] != nullptr);
        GNBV_CHECK_ARG(a.rounds == 1 || a.covered_out[q] != nullptr);
        GNBV_CHECK_ARG((((uintptr_t)a.mask_bits[q] | (uintptr_t)a.covered_in[q] | (uintptr_t)a.covered_out[q]) & 15) == 0);
        for (int r = 0; r < q; ++r) GNBV_CHECK_ARG(a.covered_out[q] == nullptr || a.covered_out[q] != a.covered_out[r]);
        weights += a.weight[q];
        p.weight[q] = a.weight[q];
        p.mask[q] = reinterpret_cast<const uint32_t *>(a.mask_bits[q]);
        p.cov_in[q] = reinterpret_cast<const uint32_t *>(a.covered_in[q]);
        p.cov_out[q] = reinterpret_cast<uint32_t *>(a.covered_out[q]);
    }
    GNBV_CHECK_ARG(weights <= 0x7fffffff / (32 * a.words));  // every score fits in int32
    p.n = a.n; p.k = a.k; p.words = a.words; p.rounds = a.rounds; p.lazy = a.lazy;
    p.contact = a.contact;
    p.choice = a.choice; p.gain = a.gain; p.plane_gain = a.plane_gain;
    p.gains0 = a.gains0; p.ub = a.ub;
    p.exact0 = (a.gains0 != nullptr || (a.lazy == 0 && a.ub != nullptr)) ? 1 : 0;
    GNBV_CHECK_ARG((int64_t)((a.n + 7) / 8 * 8) * ((a.k + kCgGainWaves - 1) / kCgGainWaves) <= 0x7fffffff);
    hipStream_t st = gnbv_stream(stream);
    switch (a.planes) {
    case 1: cgw_launch<1>(p, st); break;
    case 2: cgw_launch<2>(p, st); break;
    case 3: cgw_launch<3>(p, st); break;
    default: cgw_launch<4>(p, st); break;
    }
    return gnbv_launch_status();
}

GNBV_API int gnbv_cover_greedy(const GnbvCoverGreedy *args, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvCoverGreedy a = *args;
    GNBV_CHECK_ARG(a.n >= 1 && a.n <= 65535 && a.k >= 1 && a.k <= kCgMaxK && a.rounds >= 1 && a.rounds <= kCgMaxRounds);
    GNBV_CHECK_ARG(a.words >= 4 && (a.words & 3) == 0 && a.words <= (1 << 25) && (a.lazy == 0 || a.lazy == 1));
    GNBV_CHECK_ARG(a.mask_bits != nullptr && a.choice != nullptr && a.gain != nullptr);
    GNBV_CHECK_ARG(a.rounds == 1 || a.covered_out != nullptr);
    GNBV_CHECK_ARG((((uintptr_t)a.mask_bits | (uintptr_t)a.covered_in | (uintptr_t)a.covered_out) & 15) == 0);
    CgParams p;
    p.n = a.n; p.k = a.k; p.words = a.words; p.rounds = a.rounds; p.lazy = a.lazy;
    p.mask = reinterpret_cast<const uint32_t *>(a.mask_bits);
    p.cov_in = reinterpret_cast<const uint32_t *>(a.covered_in);
    p.contact = a.contact;
    p.choice = a.choice; p.gain = a.gain;
    p.cov_out = reinterpret_cast<uint32_t *>(a.covered_out);
    p.gains0 = a.gains0; p.ub = a.ub;
    // round 0 for every candidate in a wide launch when its gains are wanted, or exhaustive evaluation has a row to keep them
    p.exact0 = (a.gains0 != nullptr || (a.lazy == 0 && a.ub != nullptr)) ? 1 : 0;
    hipStream_t st = gnbv_stream(stream);
    if (p.exact0) {
        CgParams q = p;
        if (a.gains0 != nullptr) q.ub = nullptr;  // ub is this pass's output only where there is no gains0 row to hold the gains
        const int64_t blocks = (int64_t)((a.n + 7) / 8 * 8) * ((a.k + kCgGainWaves - 1) / kCgGainWaves);
        GNBV_CHECK_ARG(blocks <= 0x7fffffff);
        hipLaunchKernelGGL(k_cg_gains, dim3((unsigned)blocks), dim3(kCgGainWaves * kWave), 0, st, q);
    }
    const int waves = a.k < kCgMaxWaves ? a.k : kCgMaxWaves;
    hipLaunchKernelGGL(k_cg_rounds, dim3((unsigned)a.n), dim3(waves * kWave), 0, st, p);
    return gnbv_launch_status();
}

// covergreedy.hip -- greedy set cover over per-candidate bit masks, on MI355X.
//
// "Which of the env's K cached views adds the most ground-truth voxels to the covered set, T times in a row?"  (DESIGN.md "View
// pool: cached visibility masks and the greedy set-cover planner"; include/gennbv_hip.h gnbv_cover_greedy has the exact
// definition.)  gnbv_cover_greedy_w asks the same over P = 1..4 planes of masks, each with a covered row of its own, under the
// score sum_p weight_p gain_p (DESIGN.md "Weighted set cover ...").  Everything is integer, so there is one right answer.
// One kernel pair, templated on the plane count P and on W ("weighted"): <1, false> serves gnbv_cover_greedy -- the score is the
// popcount itself, and nothing of the weights or the plane gains is compiled in -- and <1..4, true> serve gnbv_cover_greedy_w.
//
//   k_cg_gains<P, W>   round 0, exhaustive: one wave per (env, candidate), 16 bytes of each plane's mask row and of the env's
//                 covered row per lane and trip (the row is L2-resident: an env's workgroups run on one XCD), __popc, a wave
//                 reduction, lane 0 stores the score.  HBM-bound: n k words 4 bytes per plane.  Launched when gains0 is wanted,
//                 or lazy == 0 with a ub row.
//   k_cg_rounds<P, W>  one workgroup per env, one wave per candidate evaluation.  The bounds, the round each bound was refreshed
//                 in and the contacts live in LDS; the covered rows live in covered_out (global: 256 KiB at 128^3 does not fit
//                 the LDS), which this workgroup alone touches: barrier + __threadfence_block() between the OR of the winner
//                 and the next round's reads.  Per round, passes of
//                   a. every wave scans its share of the candidates (j = wave, wave + waves, ...) for its largest key among
//                      the candidates refreshed this round ("fresh") and among the others ("stale");
//                   b. barrier; every lane takes the two maxima over the waves.  The largest fresh key above every stale
//                      key: that candidate wins (a stale bound is >= its true score, so nothing can overtake it);
//                   c. else every wave whose stale top lies above the best fresh key refreshes it (the others cannot win this
//                      round); barrier; again.
//                 The overall top is refreshed in every pass, so a round ends after at most ceil(k / waves) + 1 passes.  Which
//                 further stale candidates a pass refreshes changes the work, never the result: a refresh only replaces a
//                 bound by the exact score.  lazy == 0 refreshes every candidate at the start of every round instead.
//                 key = (score + 1) k + (k - 1 - j) in 64 bits: unique per candidate, larger for the lower j at equal score.
//                 W: the winner's gain per plane comes from the pass that ORs its rows into the covered rows.
// No global atomics; every output element is stored once per call; no host synchronisation, no allocation.
#include "common.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kCgMaxN = 65535;
constexpr int kCgMaxK = 4096;
constexpr int kCgMaxRounds = 4096;
constexpr int kCgMaxWaves = 16;
constexpr int kCgGainWaves = 4;  // candidates per workgroup of k_cg_gains
constexpr int kCgMaxPlanes = 4;
constexpr int kCgUnknown = 0x7fffffff;
// k_cg_gains' grid, envs rounded up to whole groups of 8, fits a launch at every n and k the entry points let through
static_assert((int64_t)((kCgMaxN + 7) / 8 * 8) * (kCgMaxK / kCgGainWaves) <= 0x7fffffff, "k_cg_gains' grid");

struct CgPlane {
    const uint32_t *mask;
    const uint32_t *cov_in;
    uint32_t *cov_out;
    int weight;
};

struct CgParams {  // (what one plane alone reads is the first 96 bytes)
    int n, k, words, rounds, lazy, exact0;
    const uint8_t *contact;
    int32_t *choice, *gain;
    int32_t *gains0, *ub;
    CgPlane plane[kCgMaxPlanes];
    int32_t *plane_gain;
};

__device__ __forceinline__ int new_bits(const uint4 m, const uint4 c)
{
    return __popc(m.x & ~c.x) + __popc(m.y & ~c.y) + __popc(m.z & ~c.z) + __popc(m.w & ~c.w);
}

// sum over the planes of weight_p popcount(mask_p row & ~covered_p row) (!W: of popcount(mask_0 row & ~covered_0 row)): P rows
// of n4 16-byte groups in one trip, the popcounts kept per plane and multiplied once after the trip; the same value in every lane.
template <int P, bool W>
__device__ __forceinline__ int wave_score(const CgParams &p, size_t row, const uint32_t *const *cov, int n4, int lane)
{
    static_assert(W || P == 1, "the unweighted score is one plane's gain");
    const uint4 *m4[P], *c4[P];
    int s[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        m4[q] = reinterpret_cast<const uint4 *>(p.plane[q].mask + row);
        c4[q] = reinterpret_cast<const uint4 *>(cov[q]);
        s[q] = 0;
    }
    // W: a loop of its own where every covered row is there -- every load of a trip is issued before the first popcount waits
    // for one, no branch between them.  One plane alone is cheapest in the one loop with the select (20 VGPRs against 36).
    bool all_cov = W;
#pragma unroll
    for (int q = 0; q < P; ++q) all_cov = all_cov && c4[q] != nullptr;
    if (all_cov) {
        for (int i = lane; i < n4; i += kWave) {
            uint4 a[P], b[P];
#pragma unroll
            for (int q = 0; q < P; ++q) a[q] = m4[q][i];
#pragma unroll
            for (int q = 0; q < P; ++q) b[q] = c4[q][i];
#pragma unroll
            for (int q = 0; q < P; ++q) s[q] += new_bits(a[q], b[q]);
        }
    } else {
        for (int i = lane; i < n4; i += kWave) {
            uint4 a[P];
#pragma unroll
            for (int q = 0; q < P; ++q) a[q] = m4[q][i];
#pragma unroll
            for (int q = 0; q < P; ++q) s[q] += new_bits(a[q], c4[q] != nullptr ? c4[q][i] : make_uint4(0u, 0u, 0u, 0u));
        }
    }
    int v = s[0];
    if (W) {
        v = 0;
#pragma unroll
        for (int q = 0; q < P; ++q) v += p.plane[q].weight * s[q];  // (the sum over the wave fits: sum_p weight_p 32 words <= INT32_MAX)
    }
    return __shfl(wave_reduce_sum(v), 0, kWave);
}

template <int P, bool W>
__global__ __launch_bounds__(kCgGainWaves * kWave) void k_cg_gains(CgParams p)
{
    int group;  // of candidates, one per wave
    const int e = xcd_env((p.k + kCgGainWaves - 1) / kCgGainWaves, group);
    const int lane = threadIdx.x & (kWave - 1);
    const int j = group * kCgGainWaves + (int)threadIdx.x / kWave;
    if (e >= p.n || j >= p.k) return;
    const uint32_t *cov[P];
#pragma unroll
    for (int q = 0; q < P; ++q) cov[q] = p.plane[q].cov_in != nullptr ? p.plane[q].cov_in + (size_t)e * p.words : nullptr;
    const int g = wave_score<P, W>(p, ((size_t)e * p.k + j) * p.words, cov, p.words / 4, lane);
    if (lane == 0) {
        if (p.gains0 != nullptr) p.gains0[(size_t)e * p.k + j] = g;
        if (p.ub != nullptr) p.ub[(size_t)e * p.k + j] = g;  // (lazy == 0 without gains0: k_cg_rounds reads them back)
    }
}

template <int P, bool W>
__global__ __launch_bounds__(kCgMaxWaves * kWave) void k_cg_rounds(CgParams p)
{
    __shared__ int s_ub[kCgMaxK];          // upper bound of the score; exact where s_at == round + 1
    __shared__ int s_at[kCgMaxK];          // 1 + the round the bound was refreshed in, 0 = never
    __shared__ uint8_t s_contact[kCgMaxK];
    __shared__ long long s_fresh[kCgMaxWaves], s_stale[kCgMaxWaves];
    __shared__ int s_pg[W ? kCgMaxWaves : 1][kCgMaxPlanes];  // W: the winner's plane gains, one partial sum per wave

    const int e = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = tid / kWave, nwaves = nthreads / kWave, lane = tid & (kWave - 1);
    const int k = p.k, n4 = p.words / 4;
    const size_t env_row = (size_t)e * k * p.words;
    int32_t *const plane_gain = W ? p.plane_gain : nullptr;
    // the covered rows this workgroup reads and grows: covered_out where there is one (rounds == 1 may go without)
    uint32_t *cov_out[P];
    const uint32_t *cov[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        cov_out[q] = p.plane[q].cov_out != nullptr ? p.plane[q].cov_out + (size_t)e * p.words : nullptr;
        const uint32_t *cov_in = p.plane[q].cov_in != nullptr ? p.plane[q].cov_in + (size_t)e * p.words : nullptr;
        cov[q] = cov_out[q] != nullptr ? cov_out[q] : cov_in;
        if (cov_out[q] != nullptr && cov_out[q] != cov_in) {
            uint4 *o4 = reinterpret_cast<uint4 *>(cov_out[q]);
            const uint4 *i4 = reinterpret_cast<const uint4 *>(cov_in);
            for (int i = tid; i < n4; i += nthreads) o4[i] = cov_in != nullptr ? i4[i] : make_uint4(0u, 0u, 0u, 0u);
        }
    }

    // bounds: the exact round-0 scores of k_cg_gains, the caller's bounds, or unknown
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
                const int g = wave_score<P, W>(p, env_row + (size_t)j * p.words, cov, n4, lane);
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
                const int g = wave_score<P, W>(p, env_row + (size_t)j * p.words, cov, n4, lane);
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
        // the winner's rows into the covered rows; W: popcount(m & ~a) before the OR is its gain in that plane
        int pg[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            pg[q] = 0;
            if (cov_out[q] == nullptr && plane_gain == nullptr) continue;
            uint4 *o4 = reinterpret_cast<uint4 *>(cov_out[q]);
            const uint4 *a4 = reinterpret_cast<const uint4 *>(cov[q]);
            const uint4 *m4 = reinterpret_cast<const uint4 *>(p.plane[q].mask + env_row + (size_t)jw * p.words);
            for (int i = tid; i < n4; i += nthreads) {
                const uint4 a = a4 != nullptr ? a4[i] : make_uint4(0u, 0u, 0u, 0u), m = m4[i];
                if (W) pg[q] += new_bits(m, a);
                if (o4 != nullptr) o4[i] = make_uint4(a.x | m.x, a.y | m.y, a.z | m.z, a.w | m.w);
            }
        }
        if (plane_gain != nullptr) {
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const int v = wave_reduce_sum(pg[q]);
                if (lane == 0) s_pg[wave][q] = v;
            }
        }
        __threadfence_block();
        __syncthreads();  // the covered rows are complete; s_fresh / s_stale and s_ub[jw] were read; s_pg is written
        if (plane_gain != nullptr && tid < P) {  // (s_pg is written again only after the next round's first barrier)
            int v = 0;
            for (int w = 0; w < nwaves; ++w) v += s_pg[w][tid];
            plane_gain[((size_t)e * p.rounds + t) * P + tid] = v;
        }
    }
    if (p.ub != nullptr)  // exact or stale, every bound is >= the score against covered_out
        for (int j = tid; j < k; j += nthreads) p.ub[(size_t)e * k + j] = s_ub[j];
}

template <int P, bool W>
void cg_launch(const CgParams &p, hipStream_t st)
{
    if (p.exact0) {
        CgParams q = p;
        if (p.gains0 != nullptr) q.ub = nullptr;  // ub is this pass's output only where there is no gains0 row to hold the scores
        const int blocks = (p.n + 7) / 8 * 8 * ((p.k + kCgGainWaves - 1) / kCgGainWaves);
        hipLaunchKernelGGL((k_cg_gains<P, W>), dim3((unsigned)blocks), dim3(kCgGainWaves * kWave), 0, st, q);
    }
    const int waves = p.k < kCgMaxWaves ? p.k : kCgMaxWaves;
    hipLaunchKernelGGL((k_cg_rounds<P, W>), dim3((unsigned)p.n), dim3(waves * kWave), 0, st, p);
}

// what both entry points refuse alike, and the params that do not depend on the plane
int cg_params(CgParams &p, int n, int k, int words, int rounds, int lazy, const uint8_t *contact, int32_t *choice, int32_t *gain,
              int32_t *gains0, int32_t *ub)
{
    GNBV_CHECK_ARG(n >= 1 && n <= kCgMaxN && k >= 1 && k <= kCgMaxK && rounds >= 1 && rounds <= kCgMaxRounds);
    GNBV_CHECK_ARG(words >= 4 && (words & 3) == 0 && words <= (1 << 25) && (lazy == 0 || lazy == 1));
    GNBV_CHECK_ARG(choice != nullptr && gain != nullptr);
    p = {};
    p.n = n; p.k = k; p.words = words; p.rounds = rounds; p.lazy = lazy;
    p.contact = contact;
    p.choice = choice; p.gain = gain;
    p.gains0 = gains0; p.ub = ub;
    // round 0 for every candidate in a wide launch when its scores are wanted, or exhaustive evaluation has a row to keep them
    p.exact0 = (gains0 != nullptr || (lazy == 0 && ub != nullptr)) ? 1 : 0;
    return (int)hipSuccess;
}

// ... and of one plane's rows
int cg_plane(CgParams &p, int q, int weight, const int32_t *mask, const int32_t *cov_in, int32_t *cov_out)
{
    GNBV_CHECK_ARG(mask != nullptr && (p.rounds == 1 || cov_out != nullptr));
    GNBV_CHECK_ARG((((uintptr_t)mask | (uintptr_t)cov_in | (uintptr_t)cov_out) & 15) == 0);
    p.plane[q].weight = weight;
    p.plane[q].mask = reinterpret_cast<const uint32_t *>(mask);
    p.plane[q].cov_in = reinterpret_cast<const uint32_t *>(cov_in);
    p.plane[q].cov_out = reinterpret_cast<uint32_t *>(cov_out);
    return (int)hipSuccess;
}

}  // namespace

GNBV_API int gnbv_cover_greedy(const GnbvCoverGreedy *args, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvCoverGreedy a = *args;
    CgParams p;
    GNBV_CHECK_ARG(cg_params(p, a.n, a.k, a.words, a.rounds, a.lazy, a.contact, a.choice, a.gain, a.gains0, a.ub) == 0);
    GNBV_CHECK_ARG(cg_plane(p, 0, 1, a.mask_bits, a.covered_in, a.covered_out) == 0);
    cg_launch<1, false>(p, gnbv_stream(stream));
    return gnbv_launch_status();
}

GNBV_API int gnbv_cover_greedy_w(const GnbvCoverGreedyW *args, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvCoverGreedyW a = *args;
    CgParams p;
    GNBV_CHECK_ARG(cg_params(p, a.n, a.k, a.words, a.rounds, a.lazy, a.contact, a.choice, a.gain, a.gains0, a.ub) == 0);
    GNBV_CHECK_ARG(a.planes >= 1 && a.planes <= kCgMaxPlanes);
    int64_t weights = 0;
    for (int q = 0; q < a.planes; ++q) {
        GNBV_CHECK_ARG(a.weight[q] >= 0);
        GNBV_CHECK_ARG(cg_plane(p, q, a.weight[q], a.mask_bits[q], a.covered_in[q], a.covered_out[q]) == 0);
        for (int r = 0; r < q; ++r) GNBV_CHECK_ARG(a.covered_out[q] == nullptr || a.covered_out[q] != a.covered_out[r]);
        weights += a.weight[q];
    }
    GNBV_CHECK_ARG(weights <= 0x7fffffff / (32 * a.words));  // every score fits in int32
    p.plane_gain = a.plane_gain;
    hipStream_t st = gnbv_stream(stream);
    switch (a.planes) {
    case 1: cg_launch<1, true>(p, st); break;
    case 2: cg_launch<2, true>(p, st); break;
    case 3: cg_launch<3, true>(p, st); break;
    default: cg_launch<4, true>(p, st); break;
    }
    return gnbv_launch_status();
}

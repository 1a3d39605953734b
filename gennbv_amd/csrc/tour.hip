// tour.hip -- plan-then-fly on MI355X: order a set of views into a short open flight tour.
//
// "In which order should the drone fly the planned views?"  (DESIGN.md "Plan-then-fly: pairwise flight costs and the tour
// kernel"; include/gennbv_hip.h gnbv_tour_route has the exact rule.)  The input is a matrix of integer leg lengths in mm
// (FlightField.pairwise_mm, or euclid_mm), point 0 is the start; the tour is nearest neighbour from 0 improved by
// best-improvement 2-opt on the open path.  Everything is integer with fixed tie rules, so there is one right answer.
//
//   k_tour_route<kLanes>   one workgroup per env (256 lanes for p <= 64, 1024 above).  LDS: the per-wave keys of the argmin,
//     the published result of the round, the tour t[] and the whole matrix D (4 p^2 bytes: 64 KiB at p = 128, which with the
//     header is above the 64 KiB a launch may ask for by default -- the host opts in through hipFuncSetAttribute).
//       1. stage D with coalesced dword loads; barrier.
//       2. wave 0 alone: the route set (ballots: lane l owns points l and l + 64), the tail of `order`, and the nearest-
//          neighbour construction -- per step two LDS reads per lane and one 64-bit wave minimum of (D << 7 | j), no barrier.
//       3. 2-opt rounds: wave w takes i = 1 + w, 1 + w + waves, ..., its lanes j = i + 1 + lane, + 64, ...; per lane the
//          smallest key = (delta + 2^34) << 14 | i << 7 | j, a wave minimum, one slot per wave, barrier, every lane takes the
//          minimum over the slots (the same value in every lane: the loop conditions are workgroup-uniform), the lanes swap
//          t[i + q] <-> t[j - q] in LDS, barrier.  delta lies in (-2^33, 2^33), so the biased value fits 35 bits and a plain
//          minimum carries "most negative delta, then lowest i, then lowest j".
//       4. wave 0: the length (64-bit wave sum), the route part of `order`, routed, length, status.
// No global atomics; every output element is stored once; no allocation, no host synchronisation.
#include "common.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kTourMaxP = 128;
constexpr int kTourMaxWaves = 16;
constexpr uint32_t kTourInf = 0xFFFFFFFFu;
constexpr long long kTourNoKey = 0x7fffffffffffffffll;
constexpr long long kTourBias = 1ll << 34;
// LDS header: keys of the waves, the tour, flags; the matrix follows (16-byte aligned)
constexpr int kTourKeysOff = 0;                                // long long [16]
constexpr int kTourTourOff = kTourKeysOff + 8 * kTourMaxWaves;  // int [128]
constexpr int kTourFlagOff = kTourTourOff + 4 * kTourMaxP;      // int [4]: [0] a 0xFFFFFFFF leg was read
constexpr int kTourHeader = kTourFlagOff + 16;
constexpr size_t kTourLdsMax = (size_t)kTourHeader + 4u * kTourMaxP * kTourMaxP;

struct TourParams {
    int p, max_moves;
    const uint32_t *dist;
    const int32_t *count;
    int32_t *order, *routed;
    int64_t *length;
    int32_t *status;
};

template <int kLanes>
__global__ __launch_bounds__(kLanes) void k_tour_route(TourParams a)
{
    extern __shared__ __attribute__((aligned(16))) char tour_lds[];
    long long *s_key = reinterpret_cast<long long *>(tour_lds + kTourKeysOff);
    int *t = reinterpret_cast<int *>(tour_lds + kTourTourOff);
    int *s_flag = reinterpret_cast<int *>(tour_lds + kTourFlagOff);
    uint32_t *D = reinterpret_cast<uint32_t *>(tour_lds + kTourHeader);

    constexpr int kWaves = kLanes / kWave;
    const int e = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const int p = a.p;
    int32_t *order = a.order + (size_t)e * p;
    const int count = a.count != nullptr ? a.count[e] : p;  // the same value in every lane: the branch below is uniform

    if (count < 1 || count > p) {  // status bit 4: the identity order, the start alone
        for (int j = tid; j < p; j += kLanes) order[j] = j;
        if (tid == 0) {
            a.routed[e] = 1;
            a.length[e] = 0;
            a.status[e] = 4;
        }
        return;
    }

    // ---- 1. the matrix
    const uint32_t *src = a.dist + (size_t)e * p * p;
    for (int q = tid; q < p * p; q += kLanes) D[q] = src[q];
    if (tid == 0) s_flag[0] = 0;
    __syncthreads();

    bool saw_inf = false;
    int routed = 0;
    // ---- 2. wave 0: route set, tail, nearest neighbour (lane l owns points l and l + 64)
    if (wave == 0) {
        const int j0 = lane, j1 = lane + kWave;
        const bool v0 = j0 < p, v1 = j1 < p;
        const bool in0 = v0 && (j0 == 0 || (j0 < count && D[j0] != kTourInf));
        const bool in1 = v1 && j1 < count && D[j1] != kTourInf;
        const unsigned long long m0 = __ballot(in0), m1 = __ballot(in1);
        const unsigned long long out0 = __ballot(v0 && !in0), out1 = __ballot(v1 && !in1);
        routed = __popcll(m0) + __popcll(m1);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (v0 && !in0) order[routed + __popcll(out0 & below)] = j0;
        if (v1 && !in1) order[routed + __popcll(out0) + __popcll(out1 & below)] = j1;
        bool left0 = in0 && j0 != 0, left1 = in1;  // in the route set, not visited yet
        int cur = 0;
        if (lane == 0) t[0] = 0;
        for (int s = 1; s < routed; ++s) {
            long long key = kTourNoKey;
            if (left0) {
                const uint32_t d = D[cur * p + j0];
                saw_inf |= d == kTourInf;
                key = ((long long)d << 7) | j0;
            }
            if (left1) {
                const uint32_t d = D[cur * p + j1];
                saw_inf |= d == kTourInf;
                const long long k1 = ((long long)d << 7) | j1;
                key = k1 < key ? k1 : key;
            }
            key = wave_min_all(key);
            cur = (int)(key & 127);
            if (cur == j0) left0 = false;
            if (cur == j1) left1 = false;
            if (lane == 0) t[s] = cur;
        }
        if (lane == 0) s_flag[1] = routed;
    }
    __syncthreads();
    const int R = s_flag[1];

    // ---- 3. best-improvement 2-opt on the open path t[0 .. R - 1]
    int moves = 0, capped = 0;
    for (;;) {  // `moves` and the published minimum are the same in every lane
        long long key = kTourNoKey;
        for (int i = 1 + wave; i < R - 1; i += kWaves) {
            const int ta = t[i - 1], ti = t[i];
            const uint32_t d_ai = D[ta * p + ti];
            for (int j = i + 1 + lane; j < R; j += kWave) {
                const int tj = t[j];
                const uint32_t d_aj = D[ta * p + tj];
                saw_inf |= d_ai == kTourInf || d_aj == kTourInf;
                long long delta = (long long)d_aj - (long long)d_ai;
                if (j + 1 < R) {
                    const int tn = t[j + 1];
                    const uint32_t d_in = D[ti * p + tn], d_jn = D[tj * p + tn];
                    saw_inf |= d_in == kTourInf || d_jn == kTourInf;
                    delta += (long long)d_in - (long long)d_jn;
                }
                const long long k = ((delta + kTourBias) << 14) | ((long long)i << 7) | j;
                key = k < key ? k : key;
            }
        }
        key = wave_min_all(key);
        if (lane == 0) s_key[wave] = key;
        __syncthreads();
        long long best = kTourNoKey;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) best = s_key[w] < best ? s_key[w] : best;
        if ((best >> 14) >= kTourBias) break;  // no delta below 0 (or no pair at all)
        if (moves >= a.max_moves) {
            capped = 1;
            break;
        }
        const int bi = (int)((best >> 7) & 127), bj = (int)(best & 127);
        int x = 0, y = 0;
        const bool swap = tid < (bj - bi + 1) / 2;
        if (swap) {
            x = t[bi + tid];
            y = t[bj - tid];
        }
        if (swap) {
            t[bi + tid] = y;
            t[bj - tid] = x;
        }
        ++moves;
        __syncthreads();  // the reversed tour is complete; every lane has read s_key
    }

    // ---- 4. length, order, status
    long long len = 0;
    if (wave == 0) {
        for (int q = lane; q + 1 < R; q += kWave) {
            const uint32_t d = D[t[q] * p + t[q + 1]];
            saw_inf |= d == kTourInf;
            len += (long long)d;
        }
        len = wave_sum_all(len);
        for (int q = lane; q < R; q += kWave) order[q] = t[q];
    }
    if (saw_inf) s_flag[0] = 1;  // (every writer stores the same value)
    __syncthreads();
    if (tid == 0) {
        a.routed[e] = R;
        a.length[e] = len;
        a.status[e] = (s_flag[0] != 0 ? 1 : 0) | (capped ? 2 : 0);
    }
}

}  // namespace

GNBV_API int gnbv_tour_route(const GnbvTourRoute *args, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvTourRoute g = *args;
    GNBV_CHECK_ARG(g.n >= 1 && g.n <= 65535 && g.p >= 1 && g.p <= kTourMaxP && g.max_moves >= 0);
    GNBV_CHECK_ARG(g.dist_mm != nullptr && g.order != nullptr && g.routed != nullptr && g.length_mm != nullptr && g.status != nullptr);
    TourParams a;
    a.p = g.p;
    a.max_moves = g.max_moves;
    a.dist = g.dist_mm;
    a.count = g.count;
    a.order = g.order;
    a.routed = g.routed;
    a.length = g.length_mm;
    a.status = g.status;
    const size_t lds = (size_t)kTourHeader + 4 * (size_t)g.p * g.p;
    if (g.p <= 64) {
        hipLaunchKernelGGL(k_tour_route<256>, dim3(g.n), dim3(256), lds, gnbv_stream(stream), a);
    } else {
        static size_t lds_allowed = 64 * 1024;  // what a launch may ask for without the attribute
        if (lds > lds_allowed) {
            const hipError_t err = hipFuncSetAttribute((const void *)k_tour_route<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTourLdsMax);
            if (err != hipSuccess) return (int)err;
            lds_allowed = kTourLdsMax;
        }
        hipLaunchKernelGGL(k_tour_route<1024>, dim3(g.n), dim3(1024), lds, gnbv_stream(stream), a);
    }
    return gnbv_launch_status();
}

// imitation.hip -- the soft-target imitation loss of gennbv_amd/sb3/imitation.py on MI355X: K weighted candidate action tuples per
// sample (a planner's scores over its K candidates) against the policy's MultiCategorical heads.
//   * k_imitation_fused    per-head marginal of the candidates, log-softmax, cross-entropy against the marginal, entropy bonus,
//                          value regression, the analytic gradient with respect to the logits and the values, agreement with the
//                          teacher's best candidate, and the statistics row -- ONE launch, row-local: a wave per sample.
// The only cross-sample quantity is W, the weight of the LIVE samples.  Whether a sample is live depends on all of its k * n_heads
// candidate indices, so a workgroup that summed W for itself (as k_ppo_fused takes its advantage statistics from B floats) would read
// B * k * n_heads indices in each of B / 4 workgroups.  Instead every wave leaves the gradient of its sample WITHOUT the common factor
// 1 / W, and the workgroup that finishes last -- it adds the per-sample terms in a fixed order anyway -- adds W in that same fixed
// order and applies 1 / W to the B * n_logits + B gradient elements.  One launch, no atomics on floats, the same bits whatever the grid.
// The few device helpers this file shares with ppo.hip are restated here, so that the code generation of the PPO loss cannot move.
#include "common.h"
#include "../../include/gennbv_hip.h"

constexpr int kImThreads = 256;
constexpr int kImWaves = kImThreads / 64;  // samples per workgroup
constexpr int kImMaxHeads = 8;
constexpr int kImMaxDim = 1024;
constexpr int kImStageK = 64;  // candidates of a sample staged in LDS (one per lane); above: read from memory where they are used

__device__ __forceinline__ float im_sum_all(float v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// largest value, lowest index among equals (torch.argmax semantics); every lane ends with the pair
__device__ __forceinline__ void im_argmax_all(float &v, int &idx)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const float ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(idx, d, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}

// The last workgroup: the seven per-sample terms added in a fixed order (thread-strided partial sums, wave reduction, the four
// wave partials in wave order), the statistics row, and 1 / W on every gradient element.
__device__ void imitation_finish(const GnbvImitationLoss &a, float *__restrict__ terms)
{
    __shared__ float part[7][kImWaves];
    const int B = a.batch, tid = threadIdx.x;
    float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = tid; j < B; j += kImThreads) {
        const volatile float *t = terms + (size_t)j * 8;
#pragma unroll
        for (int q = 0; q < 7; ++q) s[q] += t[q];
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) s[q] = wave_reduce_sum(s[q]);
    __syncthreads();
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 7; ++q) part[q][tid >> 6] = s[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        s[q] = 0.f;
#pragma unroll
        for (int w = 0; w < kImWaves; ++w) s[q] += part[q][w];
    }
    const float W = s[5], live = s[6];
    const float invW = W > 0.f ? 1.0f / W : 0.f, invL = live > 0.f ? 1.0f / live : 0.f;
    if (tid == 0) {
        const int64_t row_i = *a.stats_row;
        float *row = a.stats + (size_t)row_i * 8;
        const float ce = s[0] * invW, vl = s[1] * invW, en = s[2] * invW;
        row[0] = ce; row[1] = vl; row[2] = en;
        row[3] = s[3] * invL; row[4] = s[4] * invL;
        row[5] = W > 0.f ? ce - a.ent_coef * en + a.vf_coef * vl : 0.f;
        row[6] = live; row[7] = 0.f;
        *a.stats_row = row_i + 1;
    }
    // (the other workgroups' stores are visible: their release fence came before the ticket, this workgroup's acquire after it)
    const size_t n = (size_t)B * a.n_logits;
    for (size_t e = tid; e < n; e += kImThreads) a.d_logits[e] = a.d_logits[e] * invW;
    if (a.d_values)
        for (int e = tid; e < B; e += kImThreads) a.d_values[e] = a.d_values[e] * invW;
}

// SMALL: every head has <= 128 categories -- its logits live in two registers per lane and head, all requested before the first is
// used; otherwise the passes of a head read its logits where they lie (<= 16 per lane and pass, out of the L1 after the first).
template <bool SMALL>
__global__ __launch_bounds__(kImThreads) void k_imitation_fused(GnbvImitationLoss a, float *__restrict__ terms /*[B][8]*/, int *__restrict__ counter)
{
    __shared__ int s_idx[kImWaves][kImStageK * kImMaxHeads];  // candidate indices of the wave's sample, [j][h]
    __shared__ float s_wn[kImWaves][kImStageK];               // cand_w / Q
    __shared__ int s_last;
    const int B = a.batch, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = blockIdx.x * kImWaves + wv;
    const int nh = a.n_heads;
    const int k = a.cand_w ? a.k : 1;  // (no weights: candidate 0 alone carries weight 1, the others are never read)
    const bool staged = k <= kImStageK;
    int64_t r = 0;
    float w_b = 0.f, Q = 0.f;
    bool live = false;
    int jstar = 0;
    // ---- pass over the candidates: weights, ranges, Q, j* (the first candidate of the largest weight) ----
    if (i < B) {
        r = a.rows ? a.rows[i] : (int64_t)i;
        w_b = a.sample_w ? a.sample_w[r] : 1.0f;
        const int64_t *cd = a.cand + (size_t)r * a.k * nh;
        const float *cw = a.cand_w ? a.cand_w + (size_t)r * a.k : nullptr;
        bool bad_w = !(w_b >= 0.f && w_b < INFINITY), bad_i = false;
        float q = 0.f, best = -INFINITY;
        int best_j = 0x7fffffff;
        for (int j = lane; j < k; j += 64) {
            const float wj = cw ? cw[j] : 1.0f;
            bad_w = bad_w || !(wj >= 0.f && wj < INFINITY);
            for (int h = 0; h < nh; ++h) {
                const int64_t c = cd[(size_t)j * nh + h];
                // (a candidate of weight 0 takes part in nothing: its indices are not judged)
                if (wj != 0.f && (c < 0 || c >= (int64_t)a.head_dims[h])) bad_i = true;
                if (staged) s_idx[wv][j * kImMaxHeads + h] = (c < 0 || c >= kImMaxDim) ? -1 : (int)c;
            }
            q += wj;
            if (wj > best) { best = wj; best_j = j; }  // (j ascends per lane: strict > keeps the first)
        }
        Q = im_sum_all(q);
        im_argmax_all(best, best_j);
        jstar = best_j;
        const bool any_bad_w = __ballot(bad_w) != 0ull;
        const bool weighs = !any_bad_w && w_b != 0.f && Q != 0.f;
        const bool any_bad_i = weighs && __ballot(bad_i) != 0ull;
        live = weighs && !any_bad_i;
        if (staged && lane < k) s_wn[wv][lane] = live ? (cw ? cw[lane] : 1.0f) / Q : 0.f;
        if (lane == 0 && (any_bad_w || any_bad_i)) atomicOr(a.flags, (any_bad_i ? 1 : 0) | (any_bad_w ? 2 : 0));
    }
    __syncthreads();  // (block-uniform: the staged candidates of every wave are in LDS)
    if (i < B) {
        const float *lg = a.logits + (size_t)i * a.n_logits;
        float *dl = a.d_logits + (size_t)i * a.n_logits;
        if (!live) {
            for (int e = lane; e < a.n_logits; e += 64) dl[e] = 0.f;
            if (lane == 0) {
                if (a.d_values) a.d_values[i] = 0.f;
                float *t = terms + (size_t)i * 8;
#pragma unroll
                for (int q = 0; q < 8; ++q) t[q] = 0.f;
            }
        } else {
            const int64_t *cd = a.cand + (size_t)r * a.k * nh;
            const float *cw = a.cand_w ? a.cand_w + (size_t)r * a.k : nullptr;
            const float eps = a.label_smoothing;
            // the value term's operands and (SMALL) every head's logits are requested together
            const float v = a.values ? a.values[i] : 0.f;
            const float ret = (a.values && a.returns) ? a.returns[r] : v;
            float x0[kImMaxHeads], x1[kImMaxHeads];
            if (SMALL) {
                int off = 0;
#pragma unroll
                for (int h = 0; h < kImMaxHeads; ++h) {
                    if (h < nh) {
                        const int n = a.head_dims[h];
                        x0[h] = lg[off + min(lane, n - 1)];
                        x1[h] = lg[off + min(lane + 64, n - 1)];
                        off += n;
                    }
                }
            }
            float ce = 0.f, ent = 0.f, nll = 0.f;
            bool agree = true;
            int off = 0;
#pragma unroll
            for (int h = 0; h < kImMaxHeads; ++h) {
                if (h < nh) {
                    const int n = a.head_dims[h];
                    if (n == 1) {  // a head of one category: log-prob 0, entropy 0, no gradient
                        if (lane == 0) dl[off] = 0.f;
                    } else {
                        auto X = [&](int j) -> float { return SMALL ? (j == lane ? x0[h] : x1[h]) : lg[off + j]; };
                        // log-sum-exp, first arg-max
                        float mx = -INFINITY;
                        int am = 0x7fffffff;
                        for (int j = lane; j < n; j += 64) {
                            const float xv = X(j);
                            if (xv > mx) { mx = xv; am = j; }
                        }
                        im_argmax_all(mx, am);
                        float se = 0.f;
                        for (int j = lane; j < n; j += 64) se += expf(X(j) - mx);
                        se = im_sum_all(se);
                        const float lse = mx + logf(se);
                        float pe = 0.f;
                        for (int j = lane; j < n; j += 64) {
                            const float lp = X(j) - lse;
                            pe += expf(lp) * lp;
                        }
                        const float H = -im_sum_all(pe);
                        ent += H;
                        // the teacher's best candidate on this head
                        const int cs = staged ? s_idx[wv][jstar * kImMaxHeads + h] : (int)cd[(size_t)jstar * nh + h];
                        agree = agree && cs == am;
                        nll -= lg[off + cs] - lse;
                        // marginal of the candidates (added in candidate order), cross-entropy, gradient without 1 / W
                        const float unif = eps / (float)n;
                        float cep = 0.f;
                        for (int j = lane; j < n; j += 64) {
                            float m = 0.f;
                            if (staged) {
                                for (int c = 0; c < k; ++c) m += s_idx[wv][c * kImMaxHeads + h] == j ? s_wn[wv][c] : 0.f;
                            } else {
                                for (int c = 0; c < k; ++c) m += cd[(size_t)c * nh + h] == (int64_t)j ? cw[c] / Q : 0.f;
                            }
                            m = (1.0f - eps) * m + unif;
                            const float lp = X(j) - lse, p = expf(lp);
                            cep += m * lp;
                            dl[off + j] = w_b * ((p - m) + a.ent_coef * (p * (lp + H)));
                        }
                        ce -= im_sum_all(cep);
                    }
                    off += n;
                }
            }
            const float err = v - ret;
            if (lane == 0) {
                if (a.d_values) a.d_values[i] = w_b * (2.0f * a.vf_coef * err);
                float *t = terms + (size_t)i * 8;
                t[0] = w_b * ce;
                t[1] = w_b * (err * err);
                t[2] = w_b * ent;
                t[3] = agree ? 1.f : 0.f;
                t[4] = nll;
                t[5] = w_b;
                t[6] = 1.f;
                t[7] = 0.f;
            }
        }
    }
    // ---- the workgroup that finishes last: statistics and 1 / W (fixed order: deterministic) ----
    __syncthreads();  // (every wave's stores have left the CU)
    if (tid == 0) {
        __threadfence();
        s_last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (tid == 0) *counter = 0;  // ready for the next call
    imitation_finish(a, terms);
}

GNBV_API int gnbv_imitation_loss(const GnbvImitationLoss *a, void *stream)
{
    GNBV_CHECK_ARG(a && a->batch >= 1 && a->n_logits >= 1 && a->n_heads >= 1 && a->n_heads <= kImMaxHeads && a->k >= 1);
    int sum = 0;
    bool small_heads = true;
    for (int h = 0; h < a->n_heads; ++h) {
        GNBV_CHECK_ARG(a->head_dims[h] >= 1 && a->head_dims[h] <= kImMaxDim);
        sum += a->head_dims[h];
        small_heads = small_heads && a->head_dims[h] <= 128;
    }
    GNBV_CHECK_ARG(sum == a->n_logits);
    GNBV_CHECK_ARG(a->label_smoothing >= 0.0f && a->label_smoothing < 1.0f && a->ent_coef >= 0.0f && a->vf_coef >= 0.0f);
    GNBV_CHECK_ARG(a->logits && a->cand && a->d_logits && a->stats && a->stats_row && a->flags && a->scratch);
    GNBV_CHECK_ARG(a->values == nullptr || a->d_values != nullptr);
    GNBV_CHECK_ARG(!(a->values != nullptr && a->vf_coef > 0.0f) || a->returns != nullptr);
    hipStream_t st = gnbv_stream(stream);
    const int blocks = (a->batch + kImWaves - 1) / kImWaves;
    float *terms = a->scratch;
    int *counter = (int *)(a->scratch + 8 * (size_t)a->batch);
    if (small_heads)
        hipLaunchKernelGGL((k_imitation_fused<true>), dim3(blocks), dim3(kImThreads), 0, st, *a, terms, counter);
    else
        hipLaunchKernelGGL((k_imitation_fused<false>), dim3(blocks), dim3(kImThreads), 0, st, *a, terms, counter);
    return gnbv_launch_status();
}

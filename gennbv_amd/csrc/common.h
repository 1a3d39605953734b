// Shared helpers for the gfx950 kernels (device + host).  CDNA4 only: wave = 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>

#define GNBV_API extern "C" __attribute__((visibility("default")))

#define GNBV_CHECK_ARG(cond) \
    do {                     \
        if (!(cond)) return (int)hipErrorInvalidValue; \
    } while (0)

static inline int gnbv_launch_status() { return (int)hipGetLastError(); }

static inline hipStream_t gnbv_stream(void *s) { return (hipStream_t)s; }

constexpr int kWave = 64;

// ---- wave / block primitives ------------------------------------------------
__device__ __forceinline__ int wave_inclusive_scan(int v)
{
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        int o = __shfl_up(v, d, kWave);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ int wave_reduce_sum(int v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
    return v;
}

__device__ __forceinline__ float wave_reduce_sum(float v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
    return v;
}

// ---- block sum of N counts per lane: wave reductions -> one partial per wave in `part` (the caller's LDS, one row per wave of
// the block) -> barrier -> thread 0 adds the partials in wave order; v[] holds the block's sums in thread 0 only.  Every thread
// of the block calls it (the barrier is inside).  The caller owes the barrier between thread 0's reads of `part` and the next
// call's writes: in a loop over candidates the barrier at the loop's head is that one, since thread 0 reads before it arrives there
// and the waves write after.
template <int N>
__device__ __forceinline__ void block_sum(int (&v)[N], int (*part)[N])
{
#pragma unroll
    for (int q = 0; q < N; ++q) {
        v[q] = wave_reduce_sum(v[q]);
        if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = 0;
    for (int w = 0; w < (int)blockDim.x / kWave; ++w)
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] += part[w][q];
}

// ---- XCD-aware decode of blockIdx.x: consecutive workgroups go to the 8 XCDs in turn, so with env = 8 (slot / per_env) + xcd all
// per_env workgroups of an env run on one XCD and share its L2.  The launch has ceil(n / 8) * 8 * per_env workgroups; the caller
// drops env >= n.  rem: the workgroup's number within its env, in [0, per_env).
__device__ __forceinline__ int xcd_env(int per_env, int &rem)
{
    const int b = blockIdx.x, slot = b >> 3;
    rem = slot % per_env;
    return (slot / per_env) * 8 + (b & 7);
}

// ---- all-lanes reductions: a butterfly, every lane ends with the same bits.  The fp64 sum adds in the order d = 1, 2, .. 32:
// the winding number of collide.hip is these bits.  The integer ones give the same value in any order.
__device__ __forceinline__ double wave_sum_all(double v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

__device__ __forceinline__ long long wave_sum_all(long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

__device__ __forceinline__ long long wave_min_all(long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_min_all(unsigned long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ long long wave_max_all(long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

// ---- host: a launch may ask for 64 KiB of dynamic LDS without the attribute; the first launch of kKernel that asks for more raises
// its limit to `limit` bytes (once per process and kernel).  Keyed on the kernel itself, not on its type: the instantiations of a
// kernel template may share one function type.
template <auto kKernel>
int gnbv_raise_lds(size_t lds_bytes, int limit)
{
    static bool raised = false;
    if (lds_bytes <= 64 * 1024 || raised) return 0;
    if (hipFuncSetAttribute((const void *)kKernel, hipFuncAttributeMaxDynamicSharedMemorySize, limit) != hipSuccess)
        return (int)hipGetLastError();
    raised = true;
    return 0;
}

// ---- host: workspace carving
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

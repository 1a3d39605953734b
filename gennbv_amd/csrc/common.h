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

// ---- host: workspace carving
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

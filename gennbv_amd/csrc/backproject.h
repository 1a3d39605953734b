// backproject.h -- the A1/A2 per-pixel chain shared by the voxel update (voxel.hip) and the scan accumulator
// (scan.hip): torch.nan_to_num(neginf=0), the depth clamp of post_process_camera_tensor and the canonical fp32
// pixel -> world product of back_projection_fg.  Included by translation units built with -ffp-contract=off;
// every product / sum below is an explicit _rn intrinsic, so both users compute the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <cfloat>

// ---------------------------------------------------------------------------
// canonical fp32 arithmetic (DESIGN.md "canonical order"); file is built with
// -ffp-contract=off and every product/sum below is an explicit _rn intrinsic.
// ---------------------------------------------------------------------------
struct Intrinsics { float k[9]; };

__device__ __forceinline__ float nan_to_num_neginf0(float x)
{
    // torch.nan_to_num(x, neginf=0): NaN -> 0, +inf -> FLT_MAX, -inf -> 0
    if (x != x) return 0.0f;
    if (__builtin_isinf(x)) return x > 0.0f ? FLT_MAX : 0.0f;
    return x;
}

__device__ __forceinline__ float process_depth(float raw, float sense_dist)
{
    float d = nan_to_num_neginf0(raw);
    d = d < sense_dist ? sense_dist : d;  // clamp(min=-50)
    return fabsf(d);
}

__device__ __forceinline__ void pixel_to_world(float d, float u, float v, const Intrinsics &K, const float *M, float *out)
{
    const float pu = __fmul_rn(d, u), pv = __fmul_rn(d, v), pw = d;  // d * 1.0f == d
    float cam[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float acc = __fmul_rn(K.k[i * 3 + 0], pu);
        acc = __fmaf_rn(K.k[i * 3 + 1], pv, acc);
        acc = __fmaf_rn(K.k[i * 3 + 2], pw, acc);
        cam[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float acc = __fmul_rn(M[i * 4 + 0], cam[0]);
        acc = __fmaf_rn(M[i * 4 + 1], cam[1], acc);
        acc = __fmaf_rn(M[i * 4 + 2], cam[2], acc);
        acc = __fmaf_rn(M[i * 4 + 3], 1.0f, acc);
        out[i] = acc;
    }
}

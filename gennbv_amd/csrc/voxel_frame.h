// voxel_frame.h -- the updater's voxel frame (scanned_pts_to_idx_3D / pose_coord_to_idx_3D, gennbv/utils.py:230-270): the
// per-env bounds from range_gt and voxel_size, the keep test and voxel of a world point, the voxel of a pose.  Shared by
// the voxel update (voxel.hip) and the view coverage kernel (viewcover.hip): explicit _rn intrinsics, so the one
// expression sequence gives the same bits in both; nothing here may be restated elsewhere.  frame_min is the lower bound of the
// frame on one axis, wherever it is needed (here, ray_walk.h); voxel_frame_f64 is that frame widened to fp64, the one the belief-map
// kernels place the grid with (flightmap.hip, sweepmap.hip, frontview.hip).
#pragma once

#include <hip/hip_runtime.h>

// the lower bound of the frame on one axis: fp32(range_min - fp32(0.5 v))
__device__ __forceinline__ float frame_min(float range_min, float v) { return __fsub_rn(range_min, __fmul_rn(0.5f, v)); }

// the frame of env e in fp64 (gnbv_pose_to_idx's, the subtraction in fp32): voxel i of axis a is [o[a] + i v[a], o[a] + (i + 1) v[a]]
__device__ __forceinline__ void voxel_frame_f64(const float *__restrict__ range_gt, const float *__restrict__ voxel_size, int e, double *o,
                                                double *v)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float vf = voxel_size[e * 3 + a];
        o[a] = (double)frame_min(range_gt[e * 6 + 2 * a + 1], vf);
        v[a] = (double)vf;
    }
}

struct VoxelFrame {  // per-env constants of scanned_pts_to_idx_3D
    float vmin[3], vmax[3], vox[3];
};

__device__ __forceinline__ VoxelFrame load_frame(const float *range6, const float *vox3)
{
    VoxelFrame f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = vox3[a];
        const float half = __fmul_rn(0.5f, v);
        f.vox[a] = v;
        f.vmax[a] = __fadd_rn(range6[2 * a], half);
        f.vmin[a] = __fsub_rn(range6[2 * a + 1], half);  // (frame_min with vmax's `half`; through frame_min voxel.hip schedules differently)
    }
    return f;
}

// returns the linear voxel index (x*G + y)*G + z, or -1 when the point is dropped (strict bounds); ix: the three indices
__device__ __forceinline__ int point_to_voxel(const float *p, const VoxelFrame &f, int g, int *ix)
{
    bool keep = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = __fdiv_rn(__fsub_rn(p[a], f.vmin[a]), f.vox[a]);
        const float fl = floorf(q);
        keep = keep && (f.vmax[a] > p[a]) && (p[a] > f.vmin[a]);
        int i = (fl == fl && fabsf(fl) < 1.0e9f) ? (int)fl : 0;
        i = i < 0 ? 0 : (i > g - 1 ? g - 1 : i);
        ix[a] = i;
    }
    return keep ? (ix[0] * g + ix[1]) * g + ix[2] : -1;
}

__device__ __forceinline__ int pose_axis_to_idx(float p, float range_min, float v)
{
    const float fl = floorf(__fdiv_rn(__fsub_rn(p, frame_min(range_min, v)), v));
    // float -> int64 -> int32 (pts_source.int(), utils.py:32); poses are finite
    return (int)(long long)fl;
}

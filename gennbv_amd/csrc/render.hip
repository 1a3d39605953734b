// render.hip -- closed-loop depth / segmentation / RGBA render from the agent's pose on MI355X.
//
// Replaces the Isaac Gym camera sensors of the reference step (gennbv/env/env_train_gennbv.py:346-354): after
// step() has turned the actions into poses, every env is rendered from its own pose, so the voxel update
// back-projects the view the policy chose.  The scene is a triangle soup per env with a uniform cell grid of
// conservative CSR triangle lists (gennbv_amd/env/mesh_scene.py builds them once with torch).
//
//   k_render_camera   one lane per env: c2w from (x, y, z, pitch, yaw), fp64 trig rounded to fp32
//                     (synthetic.camera_to_world's convention; roll is ignored like there)
//   k_render_depth    one wave per 8x8 pixel tile: ray d = R * Kinv * (u, v, 1) (ray parameter == depth),
//                     3-D DDA over the env's cells, watertight ray/triangle test (Woop, Benthin, Wald 2013),
//                     closest hit with t > 1e-3, analytic ground plane z = 0 as synthetic.render_depth
//
// The camera matrix and the per-pixel trace live in raytrace.h: viewcover.hip runs the same code on candidate poses.
//
// No atomics: each lane owns its pixel, so the output is deterministic.  The per-pixel path is fp32 only.  The DDA
// axes and the ray's dominant-axis permutation are selects, not arrays, so nothing is runtime-indexed per lane.
#include "common.h"
#include "raytrace.h"
#include "scene_cells.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kTile = 8;        // 8 x 8 pixels = one wave
constexpr int kWavesPerBlock = 4;

struct Kinv9 {
    float m[9];
};

__global__ __launch_bounds__(64) void k_render_camera(const float *__restrict__ poses, int64_t poses_row_stride, int n,
                                                      float *__restrict__ c2w)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    camera_of_pose(poses + (size_t)e * poses_row_stride, c2w + (size_t)e * 16);
}

__global__ __launch_bounds__(kTile * kTile * kWavesPerBlock) void k_render_depth(
    GnbvMeshScene sc, const float *__restrict__ c2w, Kinv9 ki, int h, int w, int tiles_x, int tiles_per_env,
    float *__restrict__ depth_raw, float *__restrict__ seg_raw, uint32_t *__restrict__ rgba)
{
    const int e = blockIdx.y;
    const int tile = blockIdx.x * kWavesPerBlock + (int)(threadIdx.x >> 6);
    if (tile >= tiles_per_env) return;  // whole wave
    const int lane = threadIdx.x & 63;
    const int u = (tile % tiles_x) * kTile + (lane & 7);
    const int v = (tile / tiles_x) * kTile + (lane >> 3);
    if (u >= w || v >= h) return;

    // ---- the trace (raytrace.h: shared with viewcover.hip, one expression sequence for both)
    float best;
    int obj;
    trace_pixel(sc, e, c2w + (size_t)e * 16, ki.m, (float)u, (float)v, best, obj);

    const size_t pix = ((size_t)e * h + v) * w + u;
    depth_raw[pix] = best == INFINITY ? -INFINITY : -best;
    seg_raw[pix] = obj > 0 ? 255.f : 0.f;
    if (rgba != nullptr) {
        // synthetic.render_depth's shading of object `which` 
        uint32_t r = 90, g = 120, bl = 70;
        if (obj > 0) {
            const uint32_t shade = (uint32_t)(obj % 200) * 29u % 200u + 40u;  // == obj * 29 % 200 + 40 without overflow
            r = shade;
            g = 255u - shade;
            bl = shade / 2u + 60u;
        }
        rgba[pix] = r | (g << 8) | (bl << 16) | (255u << 24);
    }
}

}  // namespace

GNBV_API int gnbv_render_depth(const GnbvMeshScene *scene, const float *poses, int64_t poses_row_stride, const float *inv_intri,
                               int h, int w, float *c2w_out, float *depth_raw, float *seg_raw, uint8_t *rgba, void *stream)
{
    GNBV_CHECK_ARG(scene != nullptr && inv_intri != nullptr && poses != nullptr && c2w_out != nullptr);
    GNBV_CHECK_ARG(depth_raw != nullptr && seg_raw != nullptr);
    const GnbvMeshScene sc = *scene;
    GNBV_CHECK_ARG(scene_ok(sc) && sc.n <= 65535 && h > 0 && w > 0 && poses_row_stride >= 6);
    GNBV_CHECK_ARG(rgba == nullptr || ((uintptr_t)rgba & 3) == 0);
    hipStream_t st = gnbv_stream(stream);
    k_render_camera<<<(sc.n + 63) / 64, 64, 0, st>>>(poses, poses_row_stride, sc.n, c2w_out);
    Kinv9 ki;
    for (int i = 0; i < 9; ++i) ki.m[i] = inv_intri[i];
    const int tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    const int tiles = tiles_x * tiles_y;
    dim3 grid((tiles + kWavesPerBlock - 1) / kWavesPerBlock, sc.n);
    k_render_depth<<<grid, kTile * kTile * kWavesPerBlock, 0, st>>>(sc, c2w_out, ki, h, w, tiles_x, tiles, depth_raw, seg_raw,
                                                                    reinterpret_cast<uint32_t *>(rgba));
    return gnbv_launch_status();
}

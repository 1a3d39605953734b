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
// No atomics: each lane owns its pixel, so the output is deterministic.  The per-pixel path is fp32 only.  The DDA
// axes and the ray's dominant-axis permutation are selects, not arrays, so nothing is runtime-indexed per lane.
#include "common.h"
#include "../../include/gennbv_hip.h"

namespace {

constexpr float kTMin = 1e-3f;  // synthetic.render_depth's near limit (object and ground)
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
    const float *p = poses + (size_t)e * poses_row_stride;
    const double pitch = (double)p[4], yaw = (double)p[5];
    const double cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
    // columns right, down = fwd x right, fwd; the products in torch.cross's order (-ffp-contract=off: no fused multiply-add)
    const double fx = cp * cy, fy = cp * sy, fz = -sp;
    const double rx = sy, ry = -cy, rz = 0.0;
    const double dx = fy * rz - fz * ry, dy = fz * rx - fx * rz, dz = fx * ry - fy * rx;
    float *m = c2w + (size_t)e * 16;
    m[0] = (float)rx; m[1] = (float)dx; m[2] = (float)fx; m[3] = p[0];
    m[4] = (float)ry; m[5] = (float)dy; m[6] = (float)fy; m[7] = p[1];
    m[8] = (float)rz; m[9] = (float)dz; m[10] = (float)fz; m[11] = p[2];
    m[12] = 0.f; m[13] = 0.f; m[14] = 0.f; m[15] = 1.f;
}

__device__ __forceinline__ float pick3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

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

    // ---- the ray (fp32, fixed operation order: the test oracle rebuilds the same bits)
    const float *m = c2w + (size_t)e * 16;
    const float fu = (float)u, fv = (float)v;
    const float cx = ki.m[0] * fu + ki.m[1] * fv + ki.m[2];
    const float cy = ki.m[3] * fu + ki.m[4] * fv + ki.m[5];
    const float cz = ki.m[6] * fu + ki.m[7] * fv + ki.m[8];
    const float dxw = m[0] * cx + m[1] * cy + m[2] * cz;
    const float dyw = m[4] * cx + m[5] * cy + m[6] * cz;
    const float dzw = m[8] * cx + m[9] * cy + m[10] * cz;
    const float ox = m[3], oy = m[7], oz = m[11];

    // ---- ground plane z = 0, exactly as synthetic.render_depth
    float best = INFINITY;
    if (dzw < -1e-6f) {
        const float tg = -oz / dzw;
        if (tg > kTMin) best = tg;
    }
    int obj = 0;

    const int rx = sc.cell_res[e * 3 + 0], ry = sc.cell_res[e * 3 + 1], rz = sc.cell_res[e * 3 + 2];
    if (rx > 0) {
        const float lx = sc.cell_lo[e * 3 + 0], ly = sc.cell_lo[e * 3 + 1], lz = sc.cell_lo[e * 3 + 2];
        const float sx = sc.cell_size[e * 3 + 0], sy = sc.cell_size[e * 3 + 1], sz = sc.cell_size[e * 3 + 2];
        const int base = sc.cell_base[e];
        // slab test against the grid's box
        const float ix_ = 1.0f / dxw, iy_ = 1.0f / dyw, iz_ = 1.0f / dzw;  // +-inf for an axis-parallel ray
        const float ax0 = (lx - ox) * ix_, ax1 = (lx + (float)rx * sx - ox) * ix_;
        const float ay0 = (ly - oy) * iy_, ay1 = (ly + (float)ry * sy - oy) * iy_;
        const float az0 = (lz - oz) * iz_, az1 = (lz + (float)rz * sz - oz) * iz_;
        // (an axis-parallel ray outside the slab gives +-inf on both sides; inside it gives (-inf, +inf) or NaN for 0 * inf,
        // fminf / fmaxf drop the NaN)
        const float t_in = fmaxf(fmaxf(fminf(ax0, ax1), fminf(ay0, ay1)), fmaxf(fminf(az0, az1), kTMin));
        const float t_out = fminf(fminf(fmaxf(ax0, ax1), fmaxf(ay0, ay1)), fmaxf(az0, az1));
        if (t_in <= t_out && t_in < best) {
            // dominant-axis permutation of the watertight test: kz = argmax |d|, (kx, ky) keep the winding
            const float adx = fabsf(dxw), ady = fabsf(dyw), adz = fabsf(dzw);
            const int kz = (adx > ady) ? (adx > adz ? 0 : 2) : (ady > adz ? 1 : 2);
            int kx = kz == 2 ? 0 : kz + 1;
            int ky = kx == 2 ? 0 : kx + 1;
            const float dkz = pick3(dxw, dyw, dzw, kz);
            if (dkz < 0.f) {
                const int t = kx;
                kx = ky;
                ky = t;
            }
            const float shx = pick3(dxw, dyw, dzw, kx) / dkz, shy = pick3(dxw, dyw, dzw, ky) / dkz, shz = 1.0f / dkz;

            // DDA start cell: the entry point, clamped into the grid
            const float px = ox + dxw * t_in, py = oy + dyw * t_in, pz = oz + dzw * t_in;
            int cxi = min(max((int)floorf((px - lx) / sx), 0), rx - 1);
            int cyi = min(max((int)floorf((py - ly) / sy), 0), ry - 1);
            int czi = min(max((int)floorf((pz - lz) / sz), 0), rz - 1);
            const int stx = dxw > 0.f ? 1 : -1, sty = dyw > 0.f ? 1 : -1, stz = dzw > 0.f ? 1 : -1;
            const float tdx = dxw != 0.f ? sx / adx : INFINITY, tdy = dyw != 0.f ? sy / ady : INFINITY, tdz = dzw != 0.f ? sz / adz : INFINITY;
            float tmx = dxw != 0.f ? (lx + (float)(cxi + (stx > 0)) * sx - ox) * ix_ : INFINITY;
            float tmy = dyw != 0.f ? (ly + (float)(cyi + (sty > 0)) * sy - oy) * iy_ : INFINITY;
            float tmz = dzw != 0.f ? (lz + (float)(czi + (stz > 0)) * sz - oz) * iz_ : INFINITY;
            const int max_cells = rx + ry + rz;  // a ray crosses at most this many cells
            for (int it = 0; it < max_cells; ++it) {
                const int cell = base + cxi + rx * (cyi + ry * czi);
                const int b = sc.cell_start[cell], end = sc.cell_start[cell + 1];
                for (int k = b; k < end; ++k) {
                    const int tri = sc.cell_tris[k];
                    const float *q = sc.tris + (size_t)tri * 9;
                    const float Ax0 = q[0] - ox, Ay0 = q[1] - oy, Az0 = q[2] - oz;
                    const float Bx0 = q[3] - ox, By0 = q[4] - oy, Bz0 = q[5] - oz;
                    const float Cx0 = q[6] - ox, Cy0 = q[7] - oy, Cz0 = q[8] - oz;
                    const float Akz = pick3(Ax0, Ay0, Az0, kz), Bkz = pick3(Bx0, By0, Bz0, kz), Ckz = pick3(Cx0, Cy0, Cz0, kz);
                    const float Ax = pick3(Ax0, Ay0, Az0, kx) - shx * Akz, Ay = pick3(Ax0, Ay0, Az0, ky) - shy * Akz;
                    const float Bx = pick3(Bx0, By0, Bz0, kx) - shx * Bkz, By = pick3(Bx0, By0, Bz0, ky) - shy * Bkz;
                    const float Cx = pick3(Cx0, Cy0, Cz0, kx) - shx * Ckz, Cy = pick3(Cx0, Cy0, Cz0, ky) - shy * Ckz;
                    // edge functions: a shared edge gives exact negatives in its two triangles, and 0 counts as inside,
                    // so a ray through a shared edge or vertex hits at least one of the triangles (no cracks)
                    const float U = Cx * By - Cy * Bx;
                    const float V = Ax * Cy - Ay * Cx;
                    const float W = Bx * Ay - By * Ax;
                    if ((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f)) continue;
                    const float det = U + V + W;
                    if (det == 0.f) continue;
                    const float T = U * (shz * Akz) + V * (shz * Bkz) + W * (shz * Ckz);
                    const float t = T / det;
                    if (t > kTMin && t < best) {
                        best = t;
                        obj = sc.tri_obj[tri];
                    }
                }
                // the closest hit so far lies before this cell's exit: no later cell can hold a closer one
                const float t_exit = fminf(tmx, fminf(tmy, tmz));
                if (best <= t_exit || t_exit > t_out) break;
                if (tmx <= tmy && tmx <= tmz) {
                    cxi += stx;
                    tmx += tdx;
                    if (cxi < 0 || cxi >= rx) break;
                } else if (tmy <= tmz) {
                    cyi += sty;
                    tmy += tdy;
                    if (cyi < 0 || cyi >= ry) break;
                } else {
                    czi += stz;
                    tmz += tdz;
                    if (czi < 0 || czi >= rz) break;
                }
            }
        }
    }

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
    GNBV_CHECK_ARG(sc.n > 0 && sc.n <= 65535 && h > 0 && w > 0 && poses_row_stride >= 6);
    GNBV_CHECK_ARG(sc.cell_lo != nullptr && sc.cell_size != nullptr && sc.cell_res != nullptr && sc.cell_base != nullptr);
    GNBV_CHECK_ARG(sc.cell_start != nullptr);  // tris / tri_obj / cell_tris may be NULL when no env has a triangle
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

// raytrace.h -- the per-pixel trace of the closed-loop camera, shared by the renderer (render.hip) and the view
// coverage kernel (viewcover.hip): the camera matrix of a pose and the closest hit of one pixel's ray against an env's
// triangles and the ground plane.  Both users are built with -ffp-contract=off -fno-fast-math, so the one expression
// sequence below gives the same bits in both kernels; nothing here may be restated elsewhere.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/gennbv_hip.h"

constexpr float kTraceTMin = 1e-3f;  // synthetic.render_depth's near limit (object and ground)

// the camera matrix of pose q = (x, y, z, roll, pitch, yaw): fp64 trig rounded to fp32, roll ignored
// (synthetic.camera_to_world's convention)
__device__ __forceinline__ void camera_of_pose(const float *q, float *m)
{
    const double pitch = (double)q[4], yaw = (double)q[5];
    const double cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
    // columns right, down = fwd x right, fwd; the products in torch.cross's order (-ffp-contract=off: no fused multiply-add)
    const double fx = cp * cy, fy = cp * sy, fz = -sp;
    const double rx = sy, ry = -cy, rz = 0.0;
    const double dx = fy * rz - fz * ry, dy = fz * rx - fx * rz, dz = fx * ry - fy * rx;
    m[0] = (float)rx; m[1] = (float)dx; m[2] = (float)fx; m[3] = q[0];
    m[4] = (float)ry; m[5] = (float)dy; m[6] = (float)fy; m[7] = q[1];
    m[8] = (float)rz; m[9] = (float)dz; m[10] = (float)fz; m[11] = q[2];
    m[12] = 0.f; m[13] = 0.f; m[14] = 0.f; m[15] = 1.f;
}

__device__ __forceinline__ float trace_pick3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// The ray of pixel (fu, fv) of env e's camera m (c2w, row-major [4,4]; ki = the inverse intrinsics, row-major [3,3]):
// d = R * Kinv * (u, v, 1) (ray parameter == depth), 3-D DDA over the env's cells, watertight ray/triangle test (Woop,
// Benthin, Wald 2013), closest hit with t > kTraceTMin, analytic ground plane z = 0 as synthetic.render_depth.
// best = the closest t (INFINITY on a miss), obj = the hit triangle's object id (0: ground or miss).  fp32 only, fixed
// operation order: the test oracle rebuilds the same bits.  The DDA axes and the ray's dominant-axis permutation are
// selects, not arrays, so nothing is runtime-indexed per lane.
__device__ __forceinline__ void trace_pixel(const GnbvMeshScene &sc, int e, const float *m, const float (&ki)[9], float fu, float fv,
                                            float &best_out, int &obj_out)
{
    // ---- the ray
    const float cx = ki[0] * fu + ki[1] * fv + ki[2];
    const float cy = ki[3] * fu + ki[4] * fv + ki[5];
    const float cz = ki[6] * fu + ki[7] * fv + ki[8];
    const float dxw = m[0] * cx + m[1] * cy + m[2] * cz;
    const float dyw = m[4] * cx + m[5] * cy + m[6] * cz;
    const float dzw = m[8] * cx + m[9] * cy + m[10] * cz;
    const float ox = m[3], oy = m[7], oz = m[11];

    // ---- ground plane z = 0, exactly as synthetic.render_depth
    float best = INFINITY;
    if (dzw < -1e-6f) {
        const float tg = -oz / dzw;
        if (tg > kTraceTMin) best = tg;
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
        const float t_in = fmaxf(fmaxf(fminf(ax0, ax1), fminf(ay0, ay1)), fmaxf(fminf(az0, az1), kTraceTMin));
        const float t_out = fminf(fminf(fmaxf(ax0, ax1), fmaxf(ay0, ay1)), fmaxf(az0, az1));
        if (t_in <= t_out && t_in < best) {
            // dominant-axis permutation of the watertight test: kz = argmax |d|, (kx, ky) keep the winding
            const float adx = fabsf(dxw), ady = fabsf(dyw), adz = fabsf(dzw);
            const int kz = (adx > ady) ? (adx > adz ? 0 : 2) : (ady > adz ? 1 : 2);
            int kx = kz == 2 ? 0 : kz + 1;
            int ky = kx == 2 ? 0 : kx + 1;
            const float dkz = trace_pick3(dxw, dyw, dzw, kz);
            if (dkz < 0.f) {
                const int t = kx;
                kx = ky;
                ky = t;
            }
            const float shx = trace_pick3(dxw, dyw, dzw, kx) / dkz, shy = trace_pick3(dxw, dyw, dzw, ky) / dkz, shz = 1.0f / dkz;

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
                    const float Akz = trace_pick3(Ax0, Ay0, Az0, kz), Bkz = trace_pick3(Bx0, By0, Bz0, kz), Ckz = trace_pick3(Cx0, Cy0, Cz0, kz);
                    const float Ax = trace_pick3(Ax0, Ay0, Az0, kx) - shx * Akz, Ay = trace_pick3(Ax0, Ay0, Az0, ky) - shy * Akz;
                    const float Bx = trace_pick3(Bx0, By0, Bz0, kx) - shx * Bkz, By = trace_pick3(Bx0, By0, Bz0, ky) - shy * Bkz;
                    const float Cx = trace_pick3(Cx0, Cy0, Cz0, kx) - shx * Ckz, Cy = trace_pick3(Cx0, Cy0, Cz0, ky) - shy * Ckz;
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
                    if (t > kTraceTMin && t < best) {
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
    best_out = best;
    obj_out = obj;
}

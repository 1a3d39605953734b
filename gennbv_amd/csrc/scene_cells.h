// scene_cells.h -- the cell grid of a GnbvMeshScene env (per-env triangle lists in CSR form) and how a wave walks it,
// shared by the body test (collide.hip) and the swept flight (sweep.hip); the host check of a scene's pointers, shared by
// every entry point that takes one.  The users are built with -ffp-contract=off -fno-fast-math, so the one expression
// sequence below gives the same bits in all of them; nothing here may be restated elsewhere.  (raytrace.h reads the
// same grid in fp32, bit for bit as the render oracle: a different contract.)
#pragma once

#include "common.h"
#include "../../include/gennbv_hip.h"

// host: the part of a scene every entry point needs.  tris / tri_obj / cell_tris may be NULL when no env has a triangle.
static inline bool scene_ok(const GnbvMeshScene &sc)
{
    return sc.n > 0 && sc.cell_lo != nullptr && sc.cell_size != nullptr && sc.cell_res != nullptr && sc.cell_base != nullptr &&
           sc.cell_start != nullptr;
}

// ---- fp64 vector algebra of the exact triangle tests
struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 v3(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator*(V3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// ---- the grid of one env
struct EnvCells {  // per-env constants, loaded once
    int res[3], base;  // cells per axis (x fastest; 0,0,0 = an env without triangles), global index of the first cell
    double lo[3], size[3];
};

__device__ __forceinline__ EnvCells load_env_cells(const GnbvMeshScene &sc, int e)
{
    EnvCells c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c.res[k] = sc.cell_res[e * 3 + k];
        c.lo[k] = (double)sc.cell_lo[e * 3 + k];
        c.size[k] = (double)sc.cell_size[e * 3 + k];
    }
    c.base = sc.cell_base[e];
    return c;
}

struct CellRange {  // the cells c0[k] .. c1[k] per axis; c1 < c0 on an axis: none
    int c0[3], c1[3];
};
__device__ __forceinline__ CellRange no_cells() { return CellRange{{0, 0, 0}, {-1, -1, -1}}; }

// The cells the box [lo, hi] overlaps, clamped to the grid (the cell lists are a conservative superset: a triangle that
// touches the box is listed in one of them); false, and r without meaning, when the box misses the grid or the env has
// no triangles.  A 1e-6-cell margin: a point on a cell boundary may count in either neighbour.  (When it returns true
// f1 >= 0 and f0 <= res - 1, so voxelize.hip's range, which clamps c0 from below and c1 from above alone, is this one.)
__device__ __forceinline__ bool cell_range(const EnvCells &cells, const double (&lo)[3], const double (&hi)[3], CellRange &r)
{
    bool any = cells.res[0] > 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double top = (double)(cells.res[k] - 1);
        const double f0 = floor((lo[k] - cells.lo[k]) / cells.size[k] - 1e-6), f1 = floor((hi[k] - cells.lo[k]) / cells.size[k] + 1e-6);
        any = any && f1 >= 0.0 && f0 <= top;
        r.c0[k] = (int)fmin(fmax(f0, 0.0), top);
        r.c1[k] = (int)fmax(fmin(f1, top), 0.0);
    }
    return any;
}

// triangle q (9 floats): its AABB meets the closed box [blo, bhi]
__device__ __forceinline__ bool tri_aabb_meets(const float *q, const double (&blo)[3], const double (&bhi)[3])
{
    bool near = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double tmin = fmin(fmin((double)q[d], (double)q[3 + d]), (double)q[6 + d]);
        const double tmax = fmax(fmax((double)q[d], (double)q[3 + d]), (double)q[6 + d]);
        near = near && tmax >= blo[d] && tmin <= bhi[d];
    }
    return near;
}

// One wave: does test(q) hold for a triangle q (9 floats) listed in a cell of `range` that is not a cell of `prev`
// (no_cells(): every cell of `range`)?  The same value in every lane.  Up to 64 cells at a time: lane j reads cell j's list
// bounds, one wave scan makes the lists one flat range the lanes stride over.  A triangle listed in several cells is
// tested more than once: the results are ORed, and the whole wave leaves at the first hit.  `range` and `prev` must be
// wave-uniform: the trip counts then are, so every lane reaches every shuffle.
template <typename Test>
__device__ __forceinline__ bool wave_any_listed_tri(const GnbvMeshScene &sc, const EnvCells &cells, const CellRange &range,
                                                    const CellRange &prev, Test &&test)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int rx = cells.res[0], ry = cells.res[1];
    const int nx = range.c1[0] - range.c0[0] + 1, ny = range.c1[1] - range.c0[1] + 1, nz = range.c1[2] - range.c0[2] + 1;
    const int ncell = nx * ny * nz;
    for (int j0 = 0; j0 < ncell; j0 += kWave) {
        const int j = j0 + lane;
        int start = 0, cnt = 0;
        if (j < ncell) {
            const int kx = range.c0[0] + j % nx, ky = range.c0[1] + (j / nx) % ny, kz = range.c0[2] + j / (nx * ny);
            const bool seen = kx >= prev.c0[0] && kx <= prev.c1[0] && ky >= prev.c0[1] && ky <= prev.c1[1] && kz >= prev.c0[2] &&
                              kz <= prev.c1[2];
            if (!seen) {
                const int cell = cells.base + kx + rx * (ky + ry * kz);
                start = sc.cell_start[cell];
                cnt = sc.cell_start[cell + 1] - start;
            }
        }
        const int incl = wave_inclusive_scan(cnt);
        const int off = start - (incl - cnt);  // entry of flat index i in this lane's cell = off + i
        const int total = __shfl(incl, kWave - 1, kWave);
        for (int i0 = 0; i0 < total; i0 += kWave) {
            const int i = i0 + lane;
            // the lane whose cell holds flat entry i: the number of lanes with incl <= i (6 fixed steps)
            int pos = 0;
#pragma unroll
            for (int s = kWave / 2; s > 0; s >>= 1)
                if (__shfl(incl, pos + s - 1, kWave) <= i) pos += s;
            const int k = __shfl(off, pos, kWave) + i;
            bool hit = false;
            if (i < total) hit = test(sc.tris + (size_t)sc.cell_tris[k] * 9);
            if (__any(hit)) return true;
        }
    }
    return false;
}

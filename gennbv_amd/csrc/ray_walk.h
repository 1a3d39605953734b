// ray_walk.h -- the reference's integer Bresenham (voxel.hip bresenham_walk) restricted to the steps whose voxel lies in the grid,
// and the unclamped voxel of a pose.  Shared by the view gain (viewgain.hip) and the frontier viewpoints (frontview.hip): one
// closed form, one walk; nothing here may be restated elsewhere.
//
// The walk does not start at the source: the range of steps i in [0, da] whose voxel lies in the grid comes from the closed form
// of the Bresenham minors, nb(i) = floor((2 db i + da) / (2 da)) (exact on the dominant axis, widened by one step on the minors
// and guarded by a bounds test in the loop), so a source 1 000 voxels away costs at most G steps.
#pragma once

#include "common.h"
#include "voxel_frame.h"

constexpr float kCoordClamp = 16777216.0f;  // voxel coordinates saturate at +-2^24: the 64-bit closed form stays exact

// unclamped pose_to_idx of one axis (k_pose_to_idx): floor((p - (range_min - 0.5 v)) / v), IEEE division
__device__ __forceinline__ int axis_to_idx(float p, float range_min, float v)
{
    const float fl = floorf(__fdiv_rn(__fsub_rn(p, frame_min(range_min, v)), v));
    if (!(fl == fl)) return 0;
    return (int)fminf(fmaxf(fl, -kCoordClamp), kCoordClamp);
}

// floor(num / den), den > 0, |num| < 2^52: fp64 quotient + remainder fix-up
__device__ __forceinline__ long long floor_div(long long num, long long den)
{
    long long q = (long long)floor((double)num / (double)den);
    const long long r = num - q * den;
    if (r < 0) --q;
    else if (r >= den) ++q;
    return q;
}

// the same in 32 bits, den > 0 (make_slab_walk's near rays)
__device__ __forceinline__ int floor_div(int num, int den)
{
    const int q = num / den;
    return q - (num - q * den < 0 ? 1 : 0);
}

// steps [lo, hi] of a minor axis (start p0, direction s, extent d; the dominant extent is da > 0) whose coordinate
// p0 + s nb(i) may lie in [b0, b1]: one step wider than the exact range on both sides.  T: long long, or int where the
// products fit (make_slab_walk)
template <typename T>
__device__ __forceinline__ void minor_range(int p0, int s, int d, int da, int b0, int b1, T &lo, T &hi)
{
    const T mlo = s > 0 ? (T)b0 - p0 : (T)p0 - b1;  // nb(i) must reach mlo ...
    const T mhi = s > 0 ? (T)b1 - p0 : (T)p0 - b0;  // ... and not pass mhi
    if (mhi < 0 || (mlo > 0 && d == 0)) {
        hi = -1;
        return;
    }
    if (d == 0) return;
    // first i with nb(i) >= m (m >= 1): ceil((2 da m - da) / (2 d))
    if (mlo > 0) lo = max(lo, floor_div((T)2 * da * mlo - da + (T)2 * d - 1, (T)2 * d) - 1);
    hi = min(hi, floor_div((T)2 * da * (mhi + 1) - da + (T)2 * d - 1, (T)2 * d));
}

struct RayWalk {  // the walk of one ray restricted to the steps [ilo, ihi]
    int n;        // steps to take (0: the ray never meets the grid)
    int i0;       // the first of them, counted from the source
    int pb, pc, p1, p2, lin;
    int sb, sc, two_da, two_db, two_dc, la, lb, lc;  // la, lb, lc: signed linear-index strides of the three axes
};

__device__ __forceinline__ RayWalk make_walk(int x0, int y0, int z0, int x1, int y1, int z1, int g)
{
    RayWalk r;
    r.n = 0;
    const int dx = abs(x1 - x0), dy = abs(y1 - y0), dz = abs(z1 - z0);
    const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1, sz = z0 < z1 ? 1 : -1;
    const int dm = max(max(dx, dy), dz);
    // dominant axis a, minors (b, c) in the reference's order (voxel.hip bresenham_walk); st*: linear stride of the axis
    int pa, pb, pc, da, db, dc, sa, sb, sc, sta, stb, stc;
    const int gg = g * g;
    if (dm == dx)      { pa = x0; pb = y0; pc = z0; da = dx; db = dy; dc = dz; sa = sx; sb = sy; sc = sz; sta = gg; stb = g; stc = 1; }
    else if (dm == dy) { pa = y0; pb = x0; pc = z0; da = dy; db = dx; dc = dz; sa = sy; sb = sx; sc = sz; sta = g; stb = gg; stc = 1; }
    else               { pa = z0; pb = x0; pc = y0; da = dz; db = dx; dc = dy; sa = sz; sb = sx; sc = sy; sta = 1; stb = gg; stc = g; }
    // dominant axis: pa + sa i in [0, g), i in [0, da] -- exact
    long long lo = sa > 0 ? -(long long)pa : (long long)pa - (g - 1);
    long long hi = sa > 0 ? (long long)(g - 1) - pa : (long long)pa;
    lo = max(lo, 0LL);
    hi = min(hi, (long long)da);
    if (da > 0) {
        minor_range(pb, sb, db, da, 0, g - 1, lo, hi);
        if (hi >= lo) minor_range(pc, sc, dc, da, 0, g - 1, lo, hi);
    }
    if (hi < lo) return r;
    long long nb = 0, nc = 0;
    if (da > 0 && lo > 0) {
        nb = floor_div(2LL * db * lo + da, 2LL * da);
        nc = floor_div(2LL * dc * lo + da, 2LL * da);
    }
    r.n = (int)(hi - lo + 1);  // <= g + 2
    r.i0 = (int)lo;
    pa += sa * (int)lo;
    r.pb = pb + sb * (int)nb;
    r.pc = pc + sc * (int)nc;
    // the decision variables in front of step lo -> lo + 1
    r.p1 = (int)(2LL * db * (lo + 1) - da - 2LL * da * nb);
    r.p2 = (int)(2LL * dc * (lo + 1) - da - 2LL * da * nc);
    r.lin = pa * sta + r.pb * stb + r.pc * stc;
    r.sb = sb; r.sc = sc;
    r.two_da = 2 * da; r.two_db = 2 * db; r.two_dc = 2 * dc;
    r.la = sa * sta; r.lb = sb * stb; r.lc = sc * stc;
    return r;
}

// visit(lin, i) for every in-grid voxel of the walk, in order (i: the step, counted from r.i0); visit returns true to stop.
// Returns whether it stopped.
template <typename Visit>
__device__ __forceinline__ bool run_walk(RayWalk r, int g, Visit &&visit)
{
    const unsigned ug = (unsigned)g;
    for (int i = 0; i < r.n; ++i) {
        if ((unsigned)r.pb < ug && (unsigned)r.pc < ug) {
            if (visit(r.lin, i)) return true;
        }
        if (r.p1 >= 0) { r.pb += r.sb; r.lin += r.lb; r.p1 -= r.two_da; }
        if (r.p2 >= 0) { r.pc += r.sc; r.lin += r.lc; r.p2 -= r.two_da; }
        r.lin += r.la;
        r.p1 += r.two_db;
        r.p2 += r.two_dc;
    }
    return false;
}

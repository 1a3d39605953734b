// ray_walk.h -- the reference's integer Bresenham (voxel.hip bresenham_walk) restricted to a range of its steps, and the unclamped
// voxel of a pose.  Shared by the view gain (viewgain.hip) and the frontier viewpoints (frontview.hip); nothing here may be
// restated elsewhere.  Each piece exists once:
//
//   walk_axes    the dominant axis and the two minors in the reference's order, with extents, signs and linear strides;
//   the range    of steps i in [0, da] to take, one per caller.  make_walk: the steps whose voxel lies in the grid, from the
//                closed form of the Bresenham minors, nb(i) = floor((2 db i + da) / (2 da)) -- exact on the dominant axis,
//                widened by one step on the minors (minor_range) and guarded by a test in the loop, so a source 1 000 voxels away
//                costs at most G steps.  slab_cut: recorded steps [first, first + count) cut to the x-planes [X0, X1), exact if
//                x is dominant, minor_range if not;
//   walk_at<T>   coordinates, decision variables and linear index in front of the range's first step, in long long or int;
//   walk_steps   the one step loop, with the caller's "inside" test and visitor.  run_walk is it with the pb, pc test.
//
// The integer part compiles for the host too (tests/ray_walk_host.hip runs it on a CPU); axis_to_idx is device-only.
#pragma once

#include <stdlib.h>

#include "common.h"
#include "voxel_frame.h"

#define RW_FN __host__ __device__ __forceinline__

constexpr float kCoordClamp = 16777216.0f;  // voxel coordinates saturate at +-2^24: the 64-bit closed form stays exact

// unclamped pose_to_idx of one axis (k_pose_to_idx): floor((p - (range_min - 0.5 v)) / v), IEEE division
__device__ __forceinline__ int axis_to_idx(float p, float range_min, float v)
{
    const float fl = floorf(__fdiv_rn(__fsub_rn(p, frame_min(range_min, v)), v));
    if (!(fl == fl)) return 0;
    return (int)fminf(fmaxf(fl, -kCoordClamp), kCoordClamp);
}

template <typename T> RW_FN T rw_min(T a, T b) { return a < b ? a : b; }
template <typename T> RW_FN T rw_max(T a, T b) { return a > b ? a : b; }

// floor(num / den), den > 0, |num| < 2^52: fp64 quotient + remainder fix-up
RW_FN long long floor_div(long long num, long long den)
{
    long long q = (long long)floor((double)num / (double)den);
    const long long r = num - q * den;
    if (r < 0) --q;
    else if (r >= den) ++q;
    return q;
}

// the same in 32 bits, den > 0 (make_slab_cut's near rays)
RW_FN int floor_div(int num, int den)
{
    const int q = num / den;
    return q - (num - q * den < 0 ? 1 : 0);
}

// steps [lo, hi] of a minor axis (start p0, direction s, extent d; the dominant extent is da > 0) whose coordinate
// p0 + s nb(i) may lie in [b0, b1]: one step wider than the exact range on both sides.  T: long long, or int where the
// products fit (make_slab_cut)
template <typename T>
RW_FN void minor_range(int p0, int s, int d, int da, int b0, int b1, T &lo, T &hi)
{
    const T mlo = s > 0 ? (T)b0 - p0 : (T)p0 - b1;  // nb(i) must reach mlo ...
    const T mhi = s > 0 ? (T)b1 - p0 : (T)p0 - b0;  // ... and not pass mhi
    if (mhi < 0 || (mlo > 0 && d == 0)) {
        hi = -1;
        return;
    }
    if (d == 0) return;
    // first i with nb(i) >= m (m >= 1): ceil((2 da m - da) / (2 d))
    if (mlo > 0) lo = rw_max(lo, floor_div((T)2 * da * mlo - da + (T)2 * d - 1, (T)2 * d) - 1);
    hi = rw_min(hi, floor_div((T)2 * da * (mhi + 1) - da + (T)2 * d - 1, (T)2 * d));
}

// dominant axis a, minors (b, c) in the reference's order (voxel.hip bresenham_walk); st*: linear stride of the axis
struct WalkAxes {
    int pa, pb, pc, da, db, dc, sa, sb, sc, sta, stb, stc;
    bool x_dominant;
};

RW_FN WalkAxes walk_axes(int x0, int y0, int z0, int x1, int y1, int z1, int g)
{
    const int dx = abs(x1 - x0), dy = abs(y1 - y0), dz = abs(z1 - z0);
    const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1, sz = z0 < z1 ? 1 : -1;
    const int dm = rw_max(rw_max(dx, dy), dz), gg = g * g;
    const bool xd = dm == dx, yd = !xd && dm == dy, zd = !xd && !yd;
    WalkAxes a;
    a.x_dominant = xd;
    a.pa = xd ? x0 : (yd ? y0 : z0); a.da = xd ? dx : (yd ? dy : dz); a.sa = xd ? sx : (yd ? sy : sz); a.sta = xd ? gg : (yd ? g : 1);
    a.pb = xd ? y0 : x0;             a.db = xd ? dy : dx;             a.sb = xd ? sy : sx;             a.stb = xd ? g : gg;
    a.pc = zd ? y0 : z0;             a.dc = zd ? dy : dz;             a.sc = zd ? sy : sz;             a.stc = zd ? g : 1;
    return a;
}

struct RayWalk {  // the walk of one ray restricted to the steps [lo, hi]
    int n;        // steps to take (0: none)
    int i0;       // the first of them, counted from the source
    int pb, pc, p1, p2, lin;
    int sb, sc, two_da, two_db, two_dc, la, lb, lc;  // la, lb, lc: signed linear-index strides of the three axes
};

// the walk over the steps [lo, hi] (none if hi < lo), in front of step lo -> lo + 1: the closed-form jump, then the reference's
// decision variables.  T: long long, or int where the products fit
template <typename T>
RW_FN RayWalk walk_at(const WalkAxes &a, T lo, T hi)
{
    RayWalk r;
    r.n = 0;
    if (hi < lo) return r;
    T nb = 0, nc = 0;
    if (a.da > 0 && lo > 0) {
        nb = floor_div((T)2 * a.db * lo + a.da, (T)2 * a.da);
        nc = floor_div((T)2 * a.dc * lo + a.da, (T)2 * a.da);
    }
    r.n = (int)(hi - lo + 1);
    r.i0 = (int)lo;
    r.pb = a.pb + a.sb * (int)nb;
    r.pc = a.pc + a.sc * (int)nc;
    r.p1 = (int)((T)2 * a.db * (lo + 1) - a.da - (T)2 * a.da * nb);
    r.p2 = (int)((T)2 * a.dc * (lo + 1) - a.da - (T)2 * a.da * nc);
    r.lin = (a.pa + a.sa * (int)lo) * a.sta + r.pb * a.stb + r.pc * a.stc;
    r.sb = a.sb; r.sc = a.sc;
    r.two_da = 2 * a.da; r.two_db = 2 * a.db; r.two_dc = 2 * a.dc;
    r.la = a.sa * a.sta; r.lb = a.sb * a.stb; r.lc = a.sc * a.stc;
    return r;
}

// visit(lin, i) for every step of the walk that inside(walk) accepts, in order (i: the step, counted from r.i0); visit returns
// true to stop.  Returns whether it stopped.
template <typename Inside, typename Visit>
RW_FN bool walk_steps(RayWalk r, Inside &&inside, Visit &&visit)
{
    for (int i = 0; i < r.n; ++i) {
        if (inside(r)) {
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

// the steps of the ray (x0, y0, z0) -> (x1, y1, z1) whose voxel may lie in the grid; n <= g + 2
RW_FN RayWalk make_walk(int x0, int y0, int z0, int x1, int y1, int z1, int g)
{
    const WalkAxes a = walk_axes(x0, y0, z0, x1, y1, z1, g);
    // dominant axis: pa + sa i in [0, g), i in [0, da] -- exact
    long long lo = rw_max(a.sa > 0 ? -(long long)a.pa : (long long)a.pa - (g - 1), 0LL);
    long long hi = rw_min(a.sa > 0 ? (long long)(g - 1) - a.pa : (long long)a.pa, (long long)a.da);
    if (a.da > 0) {
        minor_range(a.pb, a.sb, a.db, a.da, 0, g - 1, lo, hi);
        if (hi >= lo) minor_range(a.pc, a.sc, a.dc, a.da, 0, g - 1, lo, hi);
    }
    return walk_at(a, lo, hi);
}

// walk_steps over the in-grid voxels: the minors' widened range is guarded here
template <typename Visit>
RW_FN bool run_walk(const RayWalk &r, int g, Visit &&visit)
{
    const unsigned ug = (unsigned)g;
    return walk_steps(r, [ug](const RayWalk &w) { return (unsigned)w.pb < ug && (unsigned)w.pc < ug; }, visit);
}

// The recorded in-grid steps [first, first + count) of the ray, cut to the slab of x-planes [X0, X1); lin is the index inside the
// slab, (x - X0) g^2 + y g + z, and the caller's inside test is (unsigned)lin < (X1 - X0) g^2 (y and z need none: every recorded
// step is in the grid).  int for rays of fewer than 2^14 steps: a recorded ray meets the grid, so |x0| <= da + g, the steps are
// <= da, and every product stays under 2^30.
template <typename T>
RW_FN RayWalk slab_cut(const WalkAxes &a, int g, int first, int count, int X0, int X1)
{
    T lo = first, hi = (T)first + count - 1;
    if (a.x_dominant) {  // x0 + sx i in [X0, X1 - 1], exact
        lo = rw_max(lo, a.sa > 0 ? (T)X0 - a.pa : (T)a.pa - (X1 - 1));
        hi = rw_min(hi, a.sa > 0 ? (T)(X1 - 1) - a.pa : (T)a.pa - X0);
    } else {             // x is the first minor (da > 0 here)
        minor_range<T>(a.pb, a.sb, a.db, a.da, X0, X1 - 1, lo, hi);
    }
    RayWalk r = walk_at<T>(a, lo, hi);
    if (r.n > 0) r.lin -= X0 * g * g;
    return r;
}

RW_FN RayWalk make_slab_cut(int x0, int y0, int z0, int x1, int y1, int z1, int g, int first, int count, int X0, int X1)
{
    const WalkAxes a = walk_axes(x0, y0, z0, x1, y1, z1, g);
    return a.da < (1 << 14) ? slab_cut<int>(a, g, first, count, X0, X1) : slab_cut<long long>(a, g, first, count, X0, X1);
}

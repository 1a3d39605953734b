// seg_box.h -- is the closed box [lo, hi] within R of the segment a -> b?  The exact predicate of gnbv_sweep_tri (sweepmap.hip),
// fp64, closed form, no iteration; host and device, so that a CPU build can be tested against brute force.
//
// D^2(s) = sum_a g_a(s)^2, g_a(s) = max(lo_a - x_a(s), 0, x_a(s) - hi_a), x(s) = a + s (b - a), is convex and piecewise quadratic
// in s with at most six breakpoints, where a coordinate crosses a face.  Its minimum over [0, 1] is at an end, at a breakpoint or
// at the vertex of one piece's quadratic (clamped to the piece).  Every candidate s is EVALUATED through g itself -- the value
// at any s is an upper bound of the minimum, so an inexact vertex can only miss by its own rounding, never report a touch that
// is not there -- and the ends are evaluated at a and b themselves: a zero-length segment is the ball test of
// gnbv_flight_blocked_tri, (gx^2 + gy^2) + gz^2 <= R^2, bit for bit.
#pragma once

#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ double seg_box_gap2_at(const double *p, const double *lo, const double *hi)
{
    const double gx = fmax(fmax(lo[0] - p[0], 0.0), p[0] - hi[0]);
    const double gy = fmax(fmax(lo[1] - p[1], 0.0), p[1] - hi[1]);
    const double gz = fmax(fmax(lo[2] - p[2], 0.0), p[2] - hi[2]);
    return (gx * gx + gy * gy) + gz * gz;
}

__host__ __device__ __forceinline__ double seg_box_gap2(const double *a, const double *d, const double *lo, const double *hi, double s)
{
    const double p[3] = {a[0] + s * d[0], a[1] + s * d[1], a[2] + s * d[2]};
    return seg_box_gap2_at(p, lo, hi);
}

#define GNBV_SEG_BOX_CSWAP(i, j)          \
    do {                                  \
        const double lo_ = fmin(t##i, t##j); \
        t##j = fmax(t##i, t##j);          \
        t##i = lo_;                       \
    } while (0)

// a, b the ends, d = b - a; r2 = R^2
__host__ __device__ __forceinline__ bool seg_box_within(const double *a, const double *b, const double *d, const double *lo,
                                                        const double *hi, double r2)
{
    if (seg_box_gap2_at(a, lo, hi) <= r2 || seg_box_gap2_at(b, lo, hi) <= r2) return true;
    // the breakpoints, clamped to [0, 1] (an axis the segment does not move on has none; a NaN clamps to 0)
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0, t5 = 0.0;
    if (d[0] != 0.0) {
        t0 = fmin(fmax((lo[0] - a[0]) / d[0], 0.0), 1.0);
        t1 = fmin(fmax((hi[0] - a[0]) / d[0], 0.0), 1.0);
    }
    if (d[1] != 0.0) {
        t2 = fmin(fmax((lo[1] - a[1]) / d[1], 0.0), 1.0);
        t3 = fmin(fmax((hi[1] - a[1]) / d[1], 0.0), 1.0);
    }
    if (d[2] != 0.0) {
        t4 = fmin(fmax((lo[2] - a[2]) / d[2], 0.0), 1.0);
        t5 = fmin(fmax((hi[2] - a[2]) / d[2], 0.0), 1.0);
    }
    // sorted by a 12-comparator network: registers only
    GNBV_SEG_BOX_CSWAP(0, 5); GNBV_SEG_BOX_CSWAP(1, 3); GNBV_SEG_BOX_CSWAP(2, 4);
    GNBV_SEG_BOX_CSWAP(1, 2); GNBV_SEG_BOX_CSWAP(3, 4);
    GNBV_SEG_BOX_CSWAP(0, 3); GNBV_SEG_BOX_CSWAP(2, 5);
    GNBV_SEG_BOX_CSWAP(0, 1); GNBV_SEG_BOX_CSWAP(2, 3); GNBV_SEG_BOX_CSWAP(4, 5);
    GNBV_SEG_BOX_CSWAP(1, 2); GNBV_SEG_BOX_CSWAP(3, 4);
    const double pts[8] = {0.0, t0, t1, t2, t3, t4, t5, 1.0};
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double p = pts[i], q = pts[i + 1];
        if (i > 0 && seg_box_gap2(a, d, lo, hi, p) <= r2) return true;  // a breakpoint
        if (!(q > p)) continue;
        // the piece's quadratic: the terms that are active at its middle, sum (c_a + s d_a)^2
        const double mid = 0.5 * (p + q);
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double x = a[ax] + mid * d[ax];
            if (x < lo[ax]) {
                num += (a[ax] - lo[ax]) * d[ax];
                den += d[ax] * d[ax];
            } else if (x > hi[ax]) {
                num += (a[ax] - hi[ax]) * d[ax];
                den += d[ax] * d[ax];
            }
        }
        if (den > 0.0) {
            const double s = fmin(fmax(-num / den, p), q);
            if (seg_box_gap2(a, d, lo, hi, s) <= r2) return true;
        }
    }
    return false;
}

#undef GNBV_SEG_BOX_CSWAP

// sensor.hip -- the depth sensor model of the closed-loop camera on MI355X: range limits, edge and random dropouts, range
// noise and disparity quantisation between gnbv_render_depth and everything that reads a frame.
//
// include/gennbv_hip.h gnbv_depth_sensor has the exact rule (DESIGN.md "Depth sensor model").  The result of a pixel is a pure
// function of (the input frame, seed, frame[e], e, v, u): Philox4x32-10 keyed by the seed and counted by the pixel, every fp32
// operation an explicit _rn intrinsic in the header's order (the library is built with -ffp-contract=off -fno-fast-math).
//
//   k_depth_sensor<R, kVec>   one workgroup of 256 lanes per 16 x 64 tile of an env's image; lane l owns the four pixels
//     (row l / 16, columns 4 (l % 16) .. + 3).  blockIdx.y strides over the envs.
//       kVec: w, both env strides and all four frame pointers are multiples of 16 bytes, so a lane's four pixels are in the image
//         together and move as one 16-byte load per input and one 16-byte store per output; otherwise four guarded dword accesses.
//       R > 0 (edge_radius): every lane turns its depths into a code -- t for a RET pixel, NaN for any other -- and writes them
//         to the tile's LDS image; the R-wide ring around the tile is coded from dword loads; after one barrier a lane reads the
//         (2R + 1) x (4 + 2R) strip under its four windows with two ds_read_b128 per row and tests it in registers:
//         !(|t_q - t_p| <= thr) is true for a non-RET q (NaN) and for a step above thr alike.  Neighbours outside the image are
//         skipped by their coordinates, so the LDS cells that stand for them are never written nor looked at.
//       R == 0: no LDS, no barrier.
// Traffic: 16 B per pixel (two loads, two stores); the ring adds (16 + 2R)(64 + 2R) / 1024 - 1 = 16 % (R = 1) or 33 % (R = 2)
// of depth re-reads, which come from L2.  Measured, the kernel is bound by Philox and the per-pixel arithmetic on frames that are
// mostly returns, not by that traffic.  No atomics, no workspace, every output element of every env's h w block
// stored once.
#include "common.h"
#include "../../include/gennbv_hip.h"

#include <cmath>

namespace {

constexpr int kSensTileW = 64, kSensTileH = 16, kSensLanes = 256;
constexpr int kSensPitch = kSensTileW + 8;  // floats per LDS row: >= 64 + 2 R, and a multiple of 4 so that the strips are 16-byte aligned

struct SensorParams {
    int n, h, w, tiles_x;
    const float *depth_in;
    const uint32_t *seg_in;
    int64_t in_stride;
    float *depth_out;
    uint32_t *seg_out;
    int64_t out_stride;
    const int32_t *frame;
    uint32_t key0, key1;
    float min_range, max_range, edge_abs, edge_rel;
    uint32_t edge_drop, drop;
    float sigma0, sigma1, sigma2;
    const float *gauss_lut;
    float quant;
};

struct Philox4 { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ bool sensor_drops(uint32_t threshold, uint32_t word)
{
    return threshold == 0xFFFFFFFFu || word < threshold;  // (threshold 0: no word is below it)
}

// t of a RET pixel, NaN of any other: the LDS code, and the class test of the pixel itself
__device__ __forceinline__ float sensor_code(float r, float min_range, float max_range)
{
    const float t = -r;
    return (t >= min_range && t <= max_range) ? t : __builtin_nanf("");
}

// steps 1 and 3 to 6 of the rule for one in-image pixel; `edge` is step 2's verdict (false with edge_radius 0)
__device__ __forceinline__ void sensor_pixel(const SensorParams &a, float r, bool edge, uint32_t pix, uint32_t e, uint32_t fr, uint32_t seg,
                                             float &d_out, uint32_t &s_out)
{
    const float t = -r;
    s_out = 0u;
    if (!(t >= a.min_range && t <= a.max_range)) {
        d_out = t > a.max_range ? -INFINITY : GNBV_DEPTH_NO_RETURN;  // MISS (t = +inf) and FAR : VOID
        return;
    }
    const Philox4 rnd = philox4x32_10(pix, e, fr, 0u, a.key0, a.key1);
    const bool dropped = (edge && sensor_drops(a.edge_drop, rnd.w[0])) || sensor_drops(a.drop, rnd.w[1]);
    const float z = a.gauss_lut != nullptr ? a.gauss_lut[rnd.w[2] >> 20] : 0.0f;
    const float sigma = __fadd_rn(__fadd_rn(a.sigma0, __fmul_rn(a.sigma1, t)), __fmul_rn(a.sigma2, __fmul_rn(t, t)));
    const float t1 = __fadd_rn(t, __fmul_rn(sigma, z));
    float t2 = t1;
    if (a.quant > 0.0f) t2 = __fdiv_rn(a.quant, rintf(__fdiv_rn(a.quant, t1)));
    if (dropped || !(t2 >= a.min_range)) {
        d_out = GNBV_DEPTH_NO_RETURN;
    } else if (t2 > a.max_range) {
        d_out = -INFINITY;
    } else {
        d_out = -t2;
        s_out = seg;
    }
}

template <int R, bool kVec>
__global__ __launch_bounds__(kSensLanes) void k_depth_sensor(SensorParams a)
{
    __shared__ __attribute__((aligned(16))) float tile[R > 0 ? (kSensTileH + 2 * R) * kSensPitch : 4];

    const int tid = threadIdx.x, row = tid >> 4, col4 = (tid & 15) << 2;
    const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const unsigned x0 = (unsigned)tx * kSensTileW, y0 = (unsigned)ty * kSensTileH;
    const unsigned h = (unsigned)a.h, w = (unsigned)a.w;
    const unsigned v = y0 + row, u0 = x0 + col4;
    const size_t off = (size_t)v * w + u0;  // the lane's first pixel within the env's block (used only where it is in the image)
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k] = v < h && u0 + k < w;

    for (int e = blockIdx.y; e < a.n; e += gridDim.y) {
        const float *din = a.depth_in + (size_t)e * a.in_stride;
        const uint32_t *sin = a.seg_in + (size_t)e * a.in_stride;
        float r[4];
        uint32_t s[4];
        if (kVec) {
            float4 d4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uint4 s4 = make_uint4(0u, 0u, 0u, 0u);
            if (in[0]) {  // w % 4 == 0: the four pixels are in the image together
                d4 = *reinterpret_cast<const float4 *>(din + off);
                s4 = *reinterpret_cast<const uint4 *>(sin + off);
            }
            r[0] = d4.x, r[1] = d4.y, r[2] = d4.z, r[3] = d4.w;
            s[0] = s4.x, s[1] = s4.y, s[2] = s4.z, s[3] = s4.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r[k] = in[k] ? din[off + k] : 0.0f;
                s[k] = in[k] ? sin[off + k] : 0u;
            }
        }

        bool edge[4] = {false, false, false, false};
        if (R > 0) {
            constexpr int kBand = R * (kSensTileW + 2 * R);  // the ring's top (or bottom) rows, corners included
            constexpr int kSide = kSensTileH * R;            // its left (or right) columns beside the tile
            // LDS cell (ly, lx) stands for image pixel (y0 - R + ly, x0 - R + lx)
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[(R + row) * kSensPitch + R + col4 + k] = sensor_code(r[k], a.min_range, a.max_range);
            for (int i = tid; i < 2 * kBand + 2 * kSide; i += kSensLanes) {
                int ly, lx;
                if (i < 2 * kBand) {
                    const int b = i >= kBand ? 1 : 0, j = i - b * kBand;
                    ly = j / (kSensTileW + 2 * R) + b * (R + kSensTileH);
                    lx = j % (kSensTileW + 2 * R);
                } else {
                    const int q = i - 2 * kBand, b = q >= kSide ? 1 : 0, j = q - b * kSide;
                    ly = R + j / R;
                    lx = j % R + b * (R + kSensTileW);
                }
                const unsigned gy = y0 + (unsigned)ly - R, gx = x0 + (unsigned)lx - R;  // wraps above h, w where it is left of / above 0
                if (gy < h && gx < w) tile[ly * kSensPitch + lx] = sensor_code(din[(size_t)gy * w + gx], a.min_range, a.max_range);
            }
            __syncthreads();
            float win[2 * R + 1][8];
#pragma unroll
            for (int dy = 0; dy <= 2 * R; ++dy) {
                const float4 *p = reinterpret_cast<const float4 *>(&tile[(row + dy) * kSensPitch + col4]);
                const float4 lo = p[0], hi = p[1];  // (columns past 63 + 2 R are in the pitch, never written, never used: dx <= 2 R)
                win[dy][0] = lo.x, win[dy][1] = lo.y, win[dy][2] = lo.z, win[dy][3] = lo.w;
                win[dy][4] = hi.x, win[dy][5] = hi.y, win[dy][6] = hi.z, win[dy][7] = hi.w;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float tp = -r[k];
                const float thr = __fadd_rn(a.edge_abs, __fmul_rn(a.edge_rel, tp));
                bool any = false;
#pragma unroll
                for (int dy = 0; dy <= 2 * R; ++dy) {
#pragma unroll
                    for (int dx = 0; dx <= 2 * R; ++dx) {
                        if (dy == R && dx == R) continue;
                        const bool inside = v + (unsigned)dy - R < h && u0 + (unsigned)(k + dx) - R < w;
                        // a non-RET neighbour is NaN: the comparison is false, as for a step above thr
                        any |= inside && !(fabsf(__fsub_rn(win[dy][k + dx], tp)) <= thr);
                    }
                }
                edge[k] = any;
            }
        }

        const uint32_t fr = (uint32_t)a.frame[e];
        float d_out[4];
        uint32_t s_out[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d_out[k] = 0.0f, s_out[k] = 0u;
            if (in[k]) sensor_pixel(a, r[k], edge[k], (uint32_t)(off + k), (uint32_t)e, fr, s[k], d_out[k], s_out[k]);
        }
        float *dout = a.depth_out + (size_t)e * a.out_stride;
        uint32_t *sout = a.seg_out + (size_t)e * a.out_stride;
        if (kVec) {
            if (in[0]) {
                *reinterpret_cast<float4 *>(dout + off) = make_float4(d_out[0], d_out[1], d_out[2], d_out[3]);
                *reinterpret_cast<uint4 *>(sout + off) = make_uint4(s_out[0], s_out[1], s_out[2], s_out[3]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (in[k]) {
                    dout[off + k] = d_out[k];
                    sout[off + k] = s_out[k];
                }
            }
        }
        if (R > 0) __syncthreads();  // every strip is in registers before the next env's codes land in the tile
    }
}

template <int R>
void launch_sensor(const SensorParams &a, bool vec, dim3 grid, hipStream_t stream)
{
    if (vec)
        hipLaunchKernelGGL((k_depth_sensor<R, true>), grid, dim3(kSensLanes), 0, stream, a);
    else
        hipLaunchKernelGGL((k_depth_sensor<R, false>), grid, dim3(kSensLanes), 0, stream, a);
}

bool sens_ok(float x) { return std::isfinite(x) && x >= 0.0f; }

struct Span { uintptr_t lo, hi; };

bool spans_meet(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

GNBV_API int gnbv_depth_sensor(const GnbvDepthSensor *args, void *stream)
{
    GNBV_CHECK_ARG(args != nullptr);
    const GnbvDepthSensor g = *args;
    GNBV_CHECK_ARG(g.n >= 1 && g.h >= 1 && g.w >= 1);
    const int64_t hw = (int64_t)g.h * g.w;
    GNBV_CHECK_ARG(hw <= 0xFFFFFFFFll);
    GNBV_CHECK_ARG(g.in_env_stride >= hw && g.out_env_stride >= hw);
    GNBV_CHECK_ARG(g.in_env_stride <= INT64_MAX / 8 / g.n && g.out_env_stride <= INT64_MAX / 8 / g.n);  // the spans below fit 64 bits
    GNBV_CHECK_ARG(g.depth_in != nullptr && g.seg_in != nullptr && g.depth_out != nullptr && g.seg_out != nullptr && g.frame != nullptr);
    GNBV_CHECK_ARG(std::isfinite(g.min_range) && std::isfinite(g.max_range) && g.min_range > 0.0f && g.min_range <= g.max_range);
    GNBV_CHECK_ARG(g.edge_radius >= 0 && g.edge_radius <= 2 && sens_ok(g.edge_abs) && sens_ok(g.edge_rel));
    GNBV_CHECK_ARG(sens_ok(g.sigma0) && sens_ok(g.sigma1) && sens_ok(g.sigma2) && sens_ok(g.quant));
    GNBV_CHECK_ARG(g.gauss_lut != nullptr || (g.sigma0 == 0.0f && g.sigma1 == 0.0f && g.sigma2 == 0.0f));
    // the stencil reads neighbours: no output span may meet an input span, nor the other output span
    const auto span = [&](const float *base, int64_t stride) {
        const uintptr_t lo = (uintptr_t)base;
        return Span{lo, lo + 4 * (uintptr_t)((int64_t)(g.n - 1) * stride + hw)};
    };
    const Span di = span(g.depth_in, g.in_env_stride), si = span(g.seg_in, g.in_env_stride);
    const Span dout = span(g.depth_out, g.out_env_stride), sout = span(g.seg_out, g.out_env_stride);
    GNBV_CHECK_ARG(!spans_meet(dout, di) && !spans_meet(dout, si) && !spans_meet(sout, di) && !spans_meet(sout, si) && !spans_meet(dout, sout));

    SensorParams a;
    a.n = g.n, a.h = g.h, a.w = g.w;
    a.tiles_x = (int)(((int64_t)g.w + kSensTileW - 1) / kSensTileW);
    a.depth_in = g.depth_in;
    a.seg_in = reinterpret_cast<const uint32_t *>(g.seg_in);
    a.in_stride = g.in_env_stride;
    a.depth_out = g.depth_out;
    a.seg_out = reinterpret_cast<uint32_t *>(g.seg_out);
    a.out_stride = g.out_env_stride;
    a.frame = g.frame;
    a.key0 = (uint32_t)(g.seed & 0xFFFFFFFFull), a.key1 = (uint32_t)(g.seed >> 32);
    a.min_range = g.min_range, a.max_range = g.max_range, a.edge_abs = g.edge_abs, a.edge_rel = g.edge_rel;
    a.edge_drop = g.edge_drop, a.drop = g.drop;
    a.sigma0 = g.sigma0, a.sigma1 = g.sigma1, a.sigma2 = g.sigma2;
    a.gauss_lut = g.gauss_lut;
    a.quant = g.quant;
    const int64_t tiles = (int64_t)a.tiles_x * (((int64_t)g.h + kSensTileH - 1) / kSensTileH);  // <= 2^28 + 2^26: h w < 2^32
    const bool vec = g.w % 4 == 0 && g.in_env_stride % 4 == 0 && g.out_env_stride % 4 == 0 &&
                     (((uintptr_t)g.depth_in | (uintptr_t)g.seg_in | (uintptr_t)g.depth_out | (uintptr_t)g.seg_out) & 15) == 0;
    const dim3 grid((unsigned)tiles, (unsigned)(g.n < 65535 ? g.n : 65535));
    const hipStream_t s = gnbv_stream(stream);
    switch (g.edge_radius) {
    case 0: launch_sensor<0>(a, vec, grid, s); break;
    case 1: launch_sensor<1>(a, vec, grid, s); break;
    default: launch_sensor<2>(a, vec, grid, s); break;
    }
    return gnbv_launch_status();
}

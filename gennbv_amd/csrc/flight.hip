// flight.hip -- collision-free flight between views on MI355X: the shortest 26-connected route over the flight lattice.
//
// sweep.hip answers whether the STRAIGHT flight between two poses is free.  This file answers whether ANY flight is, and how
// long the shortest one over the lattice is.  The lattice (gennbv_amd/env/flight.py) has nx * ny * nz = M nodes, node id
// c = (k ny + j) nx + i, the same for every env; bit c of blocked[e] says that the inflated sphere at node c is not free in env
// e (MeshScene.flight_blocked).  Two nodes that differ by at most one step on every axis are joined by an edge when both are
// free; the edge costs cost[|dx| | |dy| << 1 | |dz| << 2] millimetres (integers, computed once on the host), so every
// distance is an integer sum, the answer does not depend on the order of relaxation and tests compare every u32 exactly.
//
//   k_flight_field<kLds>   one workgroup of 1024 lanes per env; lane t owns nodes t, t + 1024, ...  The table d[] lives in LDS
//     (kLds: 4 M bytes after a 16-byte header; the whole 160 KiB of a CU holds 40956 nodes) or in field_out itself (global).
//       d[c] = kInf for a blocked node (never relaxed, never read as a distance), kFree for a free node nobody has reached,
//       0 for the source; then in-place (Gauss-Seidel) sweeps d[c] = min(d[c], d[n] + cost) over the 26 neighbours, the node
//       order reversed every other sweep, until a whole sweep changes nothing.
//     Only c's owner writes d[c]; neighbours are read while their owners may be writing them.  Every value ever stored is the
//     length of a real route (or kFree) and values only fall, so a torn order costs sweeps, never correctness: a sweep in
//     which nothing changed read, after the barrier before it, the final values, and a fixed point of the Bellman equations
//     with d[source] = 0 and positive costs is unique.  Reads and writes are whole dwords (relaxed atomics of workgroup scope:
//     in global memory the loads must not be served from a stale register or line across the barrier).
//     Exit: every lane reads the SAME barrier-published flag (three flags in rotation: set in sweep s, read after the barrier
//     of sweep s, cleared by lane 0 after the barrier of sweep s + 1 for sweep s + 3), so the whole workgroup leaves on
//     the same sweep; the sweep count is capped at M (Bellman-Ford needs fewer), a capped env sets status_out[e] = 1.
//     At the end kFree becomes kInf.
//     kW (gnbv_flight_field_w): entering a node whose `costly` bit is set costs penalty_mm more, whichever neighbour it is entered
//       from, so the bit belongs to the node relaxed, not to the 26 neighbours read: d[c] = min(d[c], min_n(d[n] + cost) + pen(c)).
//       In LDS a lane owns at most ceil(40956 / 1024) = 40 nodes and keeps their bits in one 64-bit register for all sweeps; in
//       global memory it reads the word of the node it relaxes.  The argument above is untouched: every stored value is still
//       the cost of a real route, values only fall, and M (max cost + penalty) < kFree keeps every sum inside 32 bits.
//   k_flight_query   one lane per (env, target): the field at the target's nearest node.
//   k_flight_path<kW>  one lane per env: the walk from the target's node down the field to the source (kW: the penalty of the
//     node walked from is part of the equation).
#include <cmath>

#include "common.h"
#include "map_bits.h"  // lattice_ok: the one lattice check, shared with the kernels that place the lattice on the map
#include "../../include/gennbv_hip.h"

namespace {

constexpr int kFieldLanes = 1024;
constexpr uint32_t kInf = 0xFFFFFFFFu;   // blocked, unreachable, no node
constexpr uint32_t kFree = 0xFFFFFFFEu;  // inside k_flight_field only: free, not reached yet
constexpr int kLdsHeader = 16;           // the three exit flags; keeps the table 16-byte aligned
constexpr int kLdsBytes = 160 * 1024;
constexpr int kLdsMaxNodes = (kLdsBytes - kLdsHeader) / 4;

struct Lattice {
    int nx, ny, nz;
    double lo[3], h[3];
    uint32_t cost[8];
};

// the nearest node of a pose: per axis clamp(floor((p - lo) / h + 0.5), 0, n - 1) in fp64; -1 for a non-finite coordinate
__device__ __forceinline__ int nearest_node(const Lattice &lat, const float *__restrict__ p)
{
    const int n[3] = {lat.nx, lat.ny, lat.nz};
    int idx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double v = (double)p[a];
        if (!isfinite(v)) return -1;
        double f = 0.0;
        if (n[a] > 1) f = fmin(fmax(floor((v - lat.lo[a]) / lat.h[a] + 0.5), 0.0), (double)(n[a] - 1));
        idx[a] = (int)f;
    }
    return (idx[2] * lat.ny + idx[1]) * lat.nx + idx[0];
}

__device__ __forceinline__ uint32_t ld(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

template <bool kLds, bool kW>
__global__ __launch_bounds__(kFieldLanes) void k_flight_field(const uint32_t *__restrict__ blocked, int words, Lattice lat,
                                                              const float *__restrict__ poses, int64_t pose_stride,
                                                              uint32_t *__restrict__ field_out, int32_t *__restrict__ status_out,
                                                              const uint32_t *__restrict__ costly, uint32_t penalty)
{
    extern __shared__ __attribute__((aligned(16))) char flight_lds[];
    int *flags = reinterpret_cast<int *>(flight_lds);
    const int e = blockIdx.x, tid = threadIdx.x;
    const int nx = lat.nx, ny = lat.ny, nz = lat.nz, m = nx * ny * nz;
    const uint32_t *bits = blocked + (size_t)e * words;
    uint32_t *out = field_out + (size_t)e * m;
    uint32_t *d = kLds ? reinterpret_cast<uint32_t *>(flight_lds + kLdsHeader) : out;

    // ---- the source (the same value in every lane: the branch below is uniform over the workgroup)
    const int src = nearest_node(lat, poses + (size_t)e * pose_stride);
    const bool src_ok = src >= 0 && ((bits[src >> 5] >> (src & 31)) & 1u) == 0;
    if (!src_ok) {
        for (int c = tid; c < m; c += kFieldLanes) out[c] = kInf;
        if (tid == 0) status_out[e] = 0;
        return;
    }
    if (tid < 3) flags[tid] = 0;
    for (int c = tid; c < m; c += kFieldLanes) st(d + c, ((bits[c >> 5] >> (c & 31)) & 1u) ? kInf : (c == src ? 0u : kFree));
    __syncthreads();

    // ---- sweeps
    const int per_lane = (m + kFieldLanes - 1) / kFieldLanes;
    const int plane = nx * ny;
    const uint32_t *pen_bits = kW ? costly + (size_t)e * words : nullptr;
    unsigned long long mine = 0ull;  // kW && kLds: bit q = the costly bit of this lane's node q * 1024 + tid (per_lane <= 40)
    if (kW && kLds)
        for (int q = 0; q < per_lane; ++q) {
            const int c = q * kFieldLanes + tid;
            if (c < m) mine |= (unsigned long long)((pen_bits[c >> 5] >> (c & 31)) & 1u) << q;
        }
    int sweep = 0, more = 1;
    while (more != 0 && sweep < m) {  // `more` and `sweep` are the same in every lane
        bool changed = false;
        for (int q = 0; q < per_lane; ++q) {  // chunk q is about one z slab: up the lattice in even sweeps, down in odd ones
            const int chunk = (sweep & 1) ? per_lane - 1 - q : q;
            const int c = chunk * kFieldLanes + tid;
            if (c >= m) continue;
            const int i = c % nx, j = (c / nx) % ny, k = c / plane;
            const uint32_t own = ld(d + c);
            if (own == kInf || own == 0u) continue;  // blocked, or the source
            // branch-free, so that the 26 loads go out back to back: a neighbour outside the lattice reads the node itself and
            // is not used.  (All three loops unrolled: offsets, cost index and the in-bounds flags become constants / registers.)
            const bool okx[3] = {i > 0, true, i < nx - 1}, oky[3] = {j > 0, true, j < ny - 1}, okz[3] = {k > 0, true, k < nz - 1};
            uint32_t dn[27];  // all loads first, then the minimum: the loads of one node are in flight together
#pragma unroll
            for (int q3 = 0; q3 < 27; ++q3) {
                const int dx = q3 % 3 - 1, dy = (q3 / 3) % 3 - 1, dz = q3 / 9 - 1;
                if (q3 == 13) continue;
                const bool in = okx[dx + 1] && oky[dy + 1] && okz[dz + 1];
                dn[q3] = ld(d + (in ? c + dz * plane + dy * nx + dx : c));
            }
            uint32_t pen = 0u;
            if (kW) pen = ((kLds ? (uint32_t)(mine >> chunk) : pen_bits[c >> 5] >> (c & 31)) & 1u) ? penalty : 0u;
            uint32_t best = own;
#pragma unroll
            for (int q3 = 0; q3 < 27; ++q3) {
                const int dx = q3 % 3 - 1, dy = (q3 / 3) % 3 - 1, dz = q3 / 9 - 1;
                if (q3 == 13) continue;
                const bool in = okx[dx + 1] && oky[dy + 1] && okz[dz + 1];
                const uint32_t cand = dn[q3] + lat.cost[(dx != 0) | ((dy != 0) << 1) | ((dz != 0) << 2)] + pen;
                best = (in && dn[q3] < kFree && cand < best) ? cand : best;  // (>= kFree: blocked or not reached)
            }
            if (best < own) {
                st(d + c, best);
                changed = true;
            }
        }
        const int slot = sweep % 3;
        if (changed) flags[slot] = 1;
        __syncthreads();
        more = flags[slot];
        if (tid == 0) flags[(slot + 2) % 3] = 0;  // last read after the barrier of sweep - 1, next set in sweep + 2
        ++sweep;
    }

    // ---- kFree -> kInf (the barrier that ended the last sweep has published every store)
    for (int c = tid; c < m; c += kFieldLanes) {
        const uint32_t v = ld(d + c);
        if (kLds || v == kFree) out[c] = v == kFree ? kInf : v;
    }
    if (tid == 0) status_out[e] = more != 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_flight_query(const uint32_t *__restrict__ field, Lattice lat, const float *__restrict__ targets, int n,
                                                      int k, int64_t row_stride, uint32_t *__restrict__ cost_out)
{
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= (int64_t)n * k) return;
    const int e = (int)(item / k);
    const int node = nearest_node(lat, targets + (size_t)item * row_stride);
    const size_t m = (size_t)lat.nx * lat.ny * lat.nz;
    cost_out[item] = node < 0 ? kInf : field[(size_t)e * m + node];
}

template <bool kW>
__global__ __launch_bounds__(kWave) void k_flight_path(const uint32_t *__restrict__ field, Lattice lat, const float *__restrict__ targets, int n,
                                                       int64_t row_stride, int32_t *__restrict__ nodes_out, int max_len,
                                                       int32_t *__restrict__ len_out, const uint32_t *__restrict__ costly, int words,
                                                       uint32_t penalty)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int nx = lat.nx, ny = lat.ny, nz = lat.nz, plane = nx * ny, m = plane * nz;
    const uint32_t *d = field + (size_t)e * m;
    int32_t *nodes = nodes_out + (size_t)e * max_len;
    int cur = nearest_node(lat, targets + (size_t)e * row_stride);
    if (cur < 0 || d[cur] == kInf) {
        len_out[e] = 0;
        return;
    }
    int count = 0;
    uint32_t dc = d[cur];
    for (;;) {
        if (count < max_len) nodes[count] = cur;
        ++count;
        if (dc == 0u || count > m) break;  // the source (count > m: a table that is no field; cannot happen after k_flight_field)
        const int i = cur % nx, j = (cur / nx) % ny, k = cur / plane;
        int next = -1;
        uint32_t dnext = 0;
        uint32_t pen = 0u;  // of the node walked from, once per node
        if (kW) pen = ((costly[(size_t)e * words + (cur >> 5)] >> (cur & 31)) & 1u) ? penalty : 0u;
        for (int dz = -1; dz <= 1 && next < 0; ++dz) {
            if ((unsigned)(k + dz) >= (unsigned)nz) continue;
            for (int dy = -1; dy <= 1 && next < 0; ++dy) {
                if ((unsigned)(j + dy) >= (unsigned)ny) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    if ((unsigned)(i + dx) >= (unsigned)nx || (dx | dy | dz) == 0) continue;
                    const int nb = cur + dz * plane + dy * nx + dx;
                    const uint32_t dn = d[nb];
                    const uint32_t step = lat.cost[(dx != 0) | ((dy != 0) << 1) | ((dz != 0) << 2)];
                    if (dn < dc && (kW ? (uint64_t)dn + step + pen == (uint64_t)dc : dn + step == dc)) {
                        next = nb;
                        dnext = dn;
                        break;
                    }
                }
            }
        }
        if (next < 0) {  // no predecessor: not a field either
            count = 0;
            break;
        }
        cur = next;
        dc = dnext;
    }
    len_out[e] = dc != 0u ? 0 : (count <= max_len ? count : -count);
}

// a lattice that passes lattice_ok (map_bits.h: shared with the kernels that place the lattice on the map), positive edge costs
// whose sum over a route through every node -- with `penalty` added at every node entered -- stays below kFree
bool make_lattice(int nx, int ny, int nz, const uint32_t *cost, const double *lo, const double *h, Lattice *out, uint32_t penalty = 0)
{
    if (cost == nullptr || lo == nullptr || h == nullptr) return false;
    if (!lattice_ok(nx, ny, nz, lo, h)) return false;
    const int n[3] = {nx, ny, nz};
    uint32_t cmax = 0;
    for (int a = 0; a < 3; ++a) {
        out->lo[a] = lo[a];
        out->h[a] = h[a];
    }
    for (int b = 0; b < 8; ++b) {
        bool used = b != 0;
        for (int a = 0; a < 3; ++a)
            if (((b >> a) & 1) && n[a] == 1) used = false;
        if (used && cost[b] == 0) return false;
        if (used && cost[b] > cmax) cmax = cost[b];
        out->cost[b] = cost[b];
    }
    const uint64_t m = (uint64_t)nx * ny * nz;
    if (m > 0x7fffffffull || m * ((uint64_t)cmax + penalty) >= (uint64_t)kFree) return false;
    out->nx = nx;
    out->ny = ny;
    out->nz = nz;
    return true;
}

template <bool kW>
int launch_field(const uint32_t *blocked, int n, int nx, int ny, int nz, const uint32_t *cost, const float *poses, int64_t poses_row_stride,
                 const double *lo, const double *h, uint32_t *field_out, int32_t *status_out, const uint32_t *costly, uint32_t penalty,
                 int mode, void *stream)
{
    GNBV_CHECK_ARG(blocked != nullptr && poses != nullptr && field_out != nullptr && status_out != nullptr && (!kW || costly != nullptr));
    GNBV_CHECK_ARG(n >= 1 && poses_row_stride >= 3 && mode >= 0 && mode <= 2);
    Lattice lat;
    GNBV_CHECK_ARG(make_lattice(nx, ny, nz, cost, lo, h, &lat, penalty));
    const int m = nx * ny * nz, words = (m + 31) / 32;
    const bool fits = m <= kLdsMaxNodes;
    GNBV_CHECK_ARG(mode != 1 || fits);
    if (mode == 1 || (mode == 0 && fits)) {
        const size_t lds = (size_t)kLdsHeader + 4 * (size_t)m;
        static size_t lds_allowed = 64 * 1024;  // what a launch may ask for without the attribute (one per instantiation)
        if (lds > lds_allowed) {
            const hipError_t err = hipFuncSetAttribute((const void *)k_flight_field<true, kW>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
            if (err != hipSuccess) return (int)err;
            lds_allowed = kLdsBytes;
        }
        hipLaunchKernelGGL((k_flight_field<true, kW>), dim3(n), dim3(kFieldLanes), lds, gnbv_stream(stream), blocked, words, lat, poses,
                           poses_row_stride, field_out, status_out, costly, penalty);
    } else {
        hipLaunchKernelGGL((k_flight_field<false, kW>), dim3(n), dim3(kFieldLanes), kLdsHeader, gnbv_stream(stream), blocked, words, lat, poses,
                           poses_row_stride, field_out, status_out, costly, penalty);
    }
    return gnbv_launch_status();
}

}  // namespace

GNBV_API int gnbv_flight_lds_max_nodes(void) { return kLdsMaxNodes; }

GNBV_API int gnbv_flight_field(const uint32_t *blocked, int n, int nx, int ny, int nz, const uint32_t *cost, const float *poses,
                               int64_t poses_row_stride, const double *lo, const double *h, uint32_t *field_out, int32_t *status_out,
                               int mode, void *stream)
{
    return launch_field<false>(blocked, n, nx, ny, nz, cost, poses, poses_row_stride, lo, h, field_out, status_out, nullptr, 0u, mode, stream);
}

GNBV_API int gnbv_flight_field_w(const uint32_t *blocked, const uint32_t *costly, uint32_t penalty_mm, int n, int nx, int ny, int nz,
                                 const uint32_t *cost, const float *poses, int64_t poses_row_stride, const double *lo, const double *h,
                                 uint32_t *field_out, int32_t *status_out, int mode, void *stream)
{
    return launch_field<true>(blocked, n, nx, ny, nz, cost, poses, poses_row_stride, lo, h, field_out, status_out, costly, penalty_mm, mode,
                              stream);
}

GNBV_API int gnbv_flight_query(const uint32_t *field, int n, int nx, int ny, int nz, const double *lo, const double *h, const float *targets,
                               int k, int64_t targets_row_stride, uint32_t *cost_mm_out, void *stream)
{
    GNBV_CHECK_ARG(field != nullptr && targets != nullptr && cost_mm_out != nullptr);
    GNBV_CHECK_ARG(n >= 1 && k >= 1 && (int64_t)n * k <= 0x7fffffff && targets_row_stride >= 3);
    const uint32_t ones[8] = {1, 1, 1, 1, 1, 1, 1, 1};  // (the query reads no cost)
    Lattice lat;
    GNBV_CHECK_ARG(make_lattice(nx, ny, nz, ones, lo, h, &lat));
    const int blocks = (int)(((int64_t)n * k + 255) / 256);
    hipLaunchKernelGGL(k_flight_query, dim3(blocks), dim3(256), 0, gnbv_stream(stream), field, lat, targets, n, k, targets_row_stride,
                       cost_mm_out);
    return gnbv_launch_status();
}

GNBV_API int gnbv_flight_path(const uint32_t *field, int n, int nx, int ny, int nz, const uint32_t *cost, const double *lo, const double *h,
                              const float *targets, int64_t targets_row_stride, int32_t *nodes_out, int max_len, int32_t *len_out,
                              void *stream)
{
    GNBV_CHECK_ARG(field != nullptr && targets != nullptr && nodes_out != nullptr && len_out != nullptr);
    GNBV_CHECK_ARG(n >= 1 && max_len >= 1 && targets_row_stride >= 3);
    Lattice lat;
    GNBV_CHECK_ARG(make_lattice(nx, ny, nz, cost, lo, h, &lat));
    hipLaunchKernelGGL(k_flight_path<false>, dim3((n + kWave - 1) / kWave), dim3(kWave), 0, gnbv_stream(stream), field, lat, targets, n,
                       targets_row_stride, nodes_out, max_len, len_out, nullptr, 0, 0u);
    return gnbv_launch_status();
}

GNBV_API int gnbv_flight_path_w(const uint32_t *field, const uint32_t *costly, uint32_t penalty_mm, int n, int nx, int ny, int nz,
                                const uint32_t *cost, const double *lo, const double *h, const float *targets, int64_t targets_row_stride,
                                int32_t *nodes_out, int max_len, int32_t *len_out, void *stream)
{
    GNBV_CHECK_ARG(field != nullptr && costly != nullptr && targets != nullptr && nodes_out != nullptr && len_out != nullptr);
    GNBV_CHECK_ARG(n >= 1 && max_len >= 1 && targets_row_stride >= 3);
    Lattice lat;
    GNBV_CHECK_ARG(make_lattice(nx, ny, nz, cost, lo, h, &lat, penalty_mm));
    hipLaunchKernelGGL(k_flight_path<true>, dim3((n + kWave - 1) / kWave), dim3(kWave), 0, gnbv_stream(stream), field, lat, targets, n,
                       targets_row_stride, nodes_out, max_len, len_out, costly, (nx * ny * nz + 31) / 32, penalty_mm);
    return gnbv_launch_status();
}

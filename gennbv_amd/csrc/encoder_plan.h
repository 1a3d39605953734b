// encoder_plan.h -- the launch plan of the encoder grid branch (encoder.hip), as plain host C++17 without any HIP include: the
// launch constants host and kernels share, the geometry helpers, the GENNBV_* switches (read from the environment here and
// nowhere else in the encoder), the path predicates forward and backward share (enc_paths), which kernel variant every stage runs
// on what grid (enc_forward_plan / enc_backward_plan), and the workspace layout in numbers (enc_ws_layout).  encoder.hip's host
// side only carries a plan out; tests/encoder_plan_dump.cpp compiles this header alone with a host compiler and prints plans, so
// the CPU suite checks the decisions the library makes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

// ---- launch constants ----
constexpr int kC = 16;          // channels of both conv layers
constexpr int kTaps = 27;
constexpr int kEncThreads = 256;
constexpr int kEncWaves = kEncThreads / 64;
constexpr int kBigThreads = 1024;  // conv2 fwd / dgrad: 16 waves share one 27 KiB weight image -> 32 waves per CU
// Workgroup = 12 waves (three per SIMD, <= 168 VGPRs each): room for the third slab buffer; 4 planes x 15 rows = 60 tiles = 5 per wave.
constexpr int kFwdThreads = 768;
constexpr int kAcThreads = 512, kAcRow = 3 * 256;
constexpr int kPlanesPerGroup = 4;
constexpr int kE1 = 512 + kC;             // conv1 weight-gradient partial row: [32 taps][16], bias [16]
constexpr int kE1F = 512 + 2 * kC;        // the fused one: T1 [32 taps][16], S1, S2 [16]
constexpr int kE2 = kTaps * 256 + kC;     // conv2 weight-gradient partial row
constexpr int kReduceSlices = 64;
// bn_state = [2][4][16] floats (scale, shift, mean, rstd per layer) + kAcRow ints: the minibatch total of the input
// autocorrelation, written by the forward whenever it computed BN1's statistics from it (EncPaths::analytic) and read
// back by the backward instead of gathering the rows again
constexpr int kBnStateFloats = 2 * 4 * kC;
constexpr int kLds64K = 64 * 1024;        // dynamic LDS a launch may ask for without the opt-in
namespace split {
constexpr int kNP = 4;                    // output planes per workgroup of the split conv2 kernels
}
namespace dsplit {
constexpr int kPairs = 4;                 // plane pairs per workgroup of the fused data-gradient kernels
}
// the split weight images' slots in the workspace, in bytes (encoder.hip ties them to conv_split.h's image sizes)
constexpr size_t kW2SplitImgBytes = 14 * 2 * 64 * 16, kW2SplitDgradSlotBytes = 2048 * 16;

// ---- geometry ----
static inline int out_size(int g) { return (g - 3) / 2 + 1; }
static inline size_t y1_elems(int batch, int O1) { return (size_t)batch * O1 * O1 * 2 * ((O1 + 1) / 2) * kC; }
static inline int sample_plane_grid(int B, int O) { return ((B + 7) / 8) * 8 * O; }
static inline int sample_plane_group_grid(int B, int O, int PZ) { return ((B + 7) / 8) * 8 * ((O + PZ - 1) / PZ); }
// Planes per workgroup of the fp32 conv2 forward kernel: the smallest of 1, 2, 4 whose grid is at most 512 workgroups (two
// per CU: one round), four beyond that.  At the reference's 20^3 (O2 = 4, 128 samples) four planes were ONE workgroup per sample whose
// waves walked two tiles one after the other in a launch that is nothing but latency:
// forward 128 -> 512 workgroups: 14.3 -> 11.7 us.  (The data gradient does NOT gain: see enc_backward_plan.)
static inline int planes_per_group(int B, int O)
{
    for (int pz = 1; pz < kPlanesPerGroup; pz <<= 1)
        if (sample_plane_group_grid(B, O, pz) <= 512) return pz;
    return kPlanesPerGroup;
}
static inline int autocorr_planes(int grid)
{
    const int p = (kLds64K / (grid * grid) - 1) / 2;
    return p < 1 ? 1 : (p > 4 ? 4 : p);
}
// stage 1 of the deterministic fp64 reduction: partial [P][E] -> tmp [slices][E]; the consumer (a *_finish kernel) adds the
// <= 64 slices in order
static inline int reduce_slices(int P)
{
    const int slices = P / 32;  // ~32 partial rows per workgroup
    return slices < 1 ? 1 : (slices > kReduceSlices ? kReduceSlices : slices);
}
// its float4 kernel: rows of whole float4 from a 16-byte aligned address (every region of enc_ws_layout with kE1, kE1F and kE2 is)
static inline bool enc_reduce_vec4(uintptr_t partial, int E) { return E % 4 == 0 && (partial & 15) == 0; }
namespace splitx {
static inline int items(int B, int O2, int XT) { return ((B + 7) / 8) * 8 * ((O2 + split::kNP - 1) / split::kNP) * XT; }
}
namespace dsplitx {
static inline int items(int B, int NA, int XT) { return ((B + 7) / 8) * 8 * ((NA + dsplit::kPairs - 1) / dsplit::kPairs) * XT; }
}
static inline int imin(int a, int b) { return a < b ? a : b; }

// ---- the switches: GENNBV_* environment variables, read on every call (tests flip them between calls of one process) ----
struct EncSwitches {
    bool conv_split;     // GENNBV_CONV_SPLIT: the split-f16 conv2 kernels (conv_split.h, conv_splitx.h)
    int splitx;          // GENNBV_SPLITX: -1 unset, 0 no x-tiled kernels, 1 the G = 64 class runs them too (tests)
    int splitx_maxwg;    // GENNBV_SPLITX_MAXWG: most workgroups of the x-tiled backward kernels (each walks items block, block + grid, ...);
                         // lowered so that small test shapes exercise the several-items-per-workgroup path
    int conv_maxwg;      // GENNBV_CONV_MAXWG: most workgroups of the G = 64 split kernels that walk several items (k_conv2_wgrad_split_dma,
                         // k_conv12_fwd_split): 256 = one per CU, i.e. two items per workgroup at the bench's minibatch; 512 restores one
                         // item per workgroup (bit-identity tests against the register-staged kernel, A/B runs)
    bool wgrad_dma;      // GENNBV_WGRAD_DMA: k_conv2_wgrad_split_dma, bit-identical to the register-staged k_conv2_wgrad_split
    bool fused_bwd;      // GENNBV_FUSED_BWD: conv2 data gradient fused with the conv1 weight gradient
    bool conv1_split;    // GENNBV_CONV1_SPLIT: k_conv1_fwd_split
    bool fused_train, fused_eval;  // GENNBV_FUSED_TRAIN / _EVAL: conv1 + BN1 + ReLU + conv2 in one launch
    bool analytic_bn1;   // GENNBV_ANALYTIC_BN1: BN1's batch statistics from the input autocorrelation
};
static inline bool enc_env_on(const char *name)  // "off" = the first character is '0'
{
    const char *e = getenv(name);
    return !(e && e[0] == '0');
}
static inline int enc_env_maxwg(const char *name, int dflt)  // 8..512, rounded down to a multiple of 8
{
    const char *e = getenv(name);
    const int v = e ? atoi(e) : 0;
    return v >= 8 && v <= 512 ? (v & ~7) : dflt;
}
static inline EncSwitches enc_switches_from_env()
{
    EncSwitches s;
    const char *sx = getenv("GENNBV_SPLITX");
    s.conv_split = enc_env_on("GENNBV_CONV_SPLIT");
    s.splitx = !sx ? -1 : sx[0] == '0' ? 0 : sx[0] == '1' ? 1 : -1;
    s.splitx_maxwg = enc_env_maxwg("GENNBV_SPLITX_MAXWG", 512);
    s.conv_maxwg = enc_env_maxwg("GENNBV_CONV_MAXWG", 256);
    s.wgrad_dma = enc_env_on("GENNBV_WGRAD_DMA");
    s.fused_bwd = enc_env_on("GENNBV_FUSED_BWD");
    s.conv1_split = enc_env_on("GENNBV_CONV1_SPLIT");
    s.fused_train = enc_env_on("GENNBV_FUSED_TRAIN");
    s.fused_eval = enc_env_on("GENNBV_FUSED_EVAL");
    s.analytic_bn1 = enc_env_on("GENNBV_ANALYTIC_BN1");
    return s;
}

// ---- what the decisions depend on besides the switches ----
struct EncFacts {
    int batch, grid;
    bool training;                       // (a backward belongs to a training forward: true)
    bool obs;                            // obs_grid: fp32 observation rows
    int obs_addr15, obs_stride4;         // its address & 15, row_stride % 4
    bool i8;                             // GnbvEncoderParams.grid_i8: the grid as int8 rows
    int i8_addr15, i8_stride16;          // its address & 15, grid_i8_row_stride % 16
    bool autocorr, autocorr_total, autocorr_global;
    bool force_fp32;
    bool dp;                             // world > 1 with sync_sum and sync_buf: BatchNorm over the replicas' global minibatch
    bool eval_prepared, features;
};

// ---- the predicates forward, backward and eval_prepare share: they must agree on what the layer-1 buffer and bn_state hold ----
struct EncPaths {
    bool split;        // conv2 kernels on the f16 matrix pipe with split (hi + lo) operands, staged through LDS (conv_split.h): fp32 y1 in
                       // the default x-parity layout, 16 voxel slots per half row (G = 64)
    bool splitx;       // the same arithmetic for rows wider than 16 voxel slots per x parity (conv_splitx.h: x tiles of 16 outputs, 17-voxel
                       // ring rows): the G = 128 class (O1 = 63, O2 = 31); GENNBV_SPLITX=1 also routes the G = 64 class through them
    bool fused_bwd;    // conv2 data gradient fused with the conv1 weight gradient (dz1' never stored): the grid as aligned int8 rows
    bool i8_staged;    // conv1 stages aligned int8 rows through a fp32 LDS slab
    bool analytic;     // BN1 batch statistics from the stored input autocorrelation rows (k_bn1_analytic: 6 us, independent of conv1)
                       // instead of partial sums in conv1 + a 12 us reduction behind it
    bool fused_eval;   // inference at G = 64: conv1 + BN1 + ReLU + conv2 in one kernel, no layer-1 buffer at all; y1 is left untouched
    bool fused_train;  // training with BN1's statistics known beforehand: the same launch, which also stores y1 for the backward
    bool saved_total;  // the forward leaves the minibatch's autocorrelation total in bn_state and the fused backward reads it there
};
static inline EncPaths enc_paths(const EncFacts &f, const EncSwitches &s)
{
    const int G = f.grid, O1 = out_size(G), O2 = out_size(O1), XH = (O1 + 1) / 2;
    const bool f16 = s.conv_split && !f.force_fp32;
    const bool i8_rows = f.i8 && G % 16 == 0 && f.i8_stride16 == 0 && f.i8_addr15 == 0;
    const bool ac_fits = 3 * G * G <= kLds64K;  // k_input_autocorr's three planes
    EncPaths p;
    p.split = f16 && XH == 16 && O2 <= 15;
    p.splitx = f16 && O2 >= 1 && s.splitx != 0 && ((XH > 16 && XH <= 32 && O2 <= 32) || (XH == 16 && O2 <= 15 && s.splitx == 1));
    p.fused_bwd = s.fused_bwd && i8_rows && ac_fits;
    p.i8_staged = i8_rows && (size_t)3 * (2 * O1 + 1) * G * sizeof(float) <= (size_t)kLds64K && 2 * O1 + 1 <= G;
    p.analytic = f.training && f.autocorr && p.i8_staged && ac_fits && s.analytic_bn1;
    p.fused_eval = !f.training && p.split && p.i8_staged && G == 64 && s.fused_eval;
    p.fused_train = p.analytic && p.split && G == 64 && s.conv1_split && s.fused_train;
    p.saved_total = p.fused_bwd && p.analytic;
    return p;
}

enum class EncRefusal {
    NONE,
    DP_NEEDS_GLOBAL_AUTOCORR,  // hipErrorInvalidValue: data-parallel BatchNorm runs on the analytic + fused path only (GnbvEncoderParams.world)
    NOT_APPLICABLE,            // GNBV_ERR_NOT_APPLICABLE: gnbv_encoder_eval_prepare where the forward is not the one-launch inference
};

// ---- forward ----
enum class Bn1 { PREPARED, PREPARE, ANALYTIC, REDUCE, FINALIZE };  // fused eval: the caller's eval_prepare / the same launches here
enum class Conv1 {
    FUSED,        // k_conv12_fwd_split<training>: conv2 rides along
    SPLIT,        // k_conv1_fwd_split (no partial sums: BN1 is analytic or in eval mode)
    LDS_I8,       // k_conv1_fwd_lds<int8>: compact int8 copy of the tri-class grid, a quarter of the input bytes
    LDS_F32,      // k_conv1_fwd_lds<float>
    LDS_I8_SLAB,  // k_conv1_fwd_lds<int8, true>: int8 rows, fp32 slab too large (G = 128): int8 slab
    DIRECT_I8,    // k_conv1_fwd<int8>: compact rows at a size the staged kernels do not take
    DIRECT_F32,   // k_conv1_fwd
};
enum class Conv2 { FUSED, SPLITX, SPLIT, FP32 };
enum class Bn2 { NONE, DP, REDUCE, FINALIZE };

struct EncForwardPlan {
    EncRefusal refusal;
    EncPaths paths;
    int O1, O2, P2;
    Bn1 bn1;
    int bn1_grid;        // k_bn1_analytic: 9 workgroups where it also writes the weight images (fused_train), else 1
    bool have_total;     // ... from the caller's minibatch total: no gather (GnbvEncoderParams.autocorr_total)
    Conv1 conv1;
    int c1_grid;
    size_t c1_lds;
    bool c1_part;        // conv1 writes BN1 partial sums: one row of bn_part per workgroup
    int split_img;       // conv1 writes the f16 weight images in passing: only where a split kernel reads them
    int nitems;          // FUSED: a workgroup walks items block, block + grid, ... on one continuous ring
    Conv2 conv2;
    int g2;              // conv2's workgroups = BN2 partial rows (FUSED: one per ITEM, whatever the grid)
    int XT, pz2;
    Bn2 bn2;
    int feat_grid;       // k_bn_relu_apply, 0: no features (the consumer folds BN2 + ReLU into its operand load)
};

static inline EncForwardPlan enc_forward_plan(const EncFacts &f, const EncSwitches &s)
{
    EncForwardPlan p = {};
    const EncPaths &t = p.paths = enc_paths(f, s);
    const int B = f.batch, G = f.grid, O1 = p.O1 = out_size(G), O2 = p.O2 = out_size(O1);
    p.P2 = O2 * O2 * O2;
    const bool dp = f.training && f.dp;
    if (dp && !(t.saved_total && f.autocorr_global)) p.refusal = EncRefusal::DP_NEEDS_GLOBAL_AUTOCORR;
    p.bn1 = t.fused_eval ? (f.eval_prepared ? Bn1::PREPARED : Bn1::PREPARE) : t.analytic ? Bn1::ANALYTIC : f.training ? Bn1::REDUCE : Bn1::FINALIZE;
    p.bn1_grid = t.fused_train ? 9 : 1;
    p.have_total = f.autocorr_total && !dp;
    p.c1_part = f.training && !t.analytic;
    p.split_img = (t.split || t.splitx) ? 1 : 0;
    p.c1_grid = sample_plane_grid(B, O1);
    const size_t slab = (size_t)3 * (2 * O1 + 1) * G * sizeof(float);
    const bool rows_fit = 2 * O1 + 1 <= G;
    if (t.fused_eval || t.fused_train) {
        p.conv1 = Conv1::FUSED;
        p.nitems = sample_plane_group_grid(B, O2, split::kNP);
        p.c1_grid = imin(p.nitems, s.conv_maxwg);
    } else if (t.i8_staged && !p.c1_part && G == 64 && t.split && s.conv1_split) {
        p.conv1 = Conv1::SPLIT;
    } else if (t.i8_staged) {
        p.conv1 = Conv1::LDS_I8, p.c1_lds = slab;
    } else if (f.obs && G % 4 == 0 && f.obs_stride4 == 0 && f.obs_addr15 == 0 && slab <= (size_t)kLds64K && rows_fit) {
        p.conv1 = Conv1::LDS_F32, p.c1_lds = slab;
    } else if (f.i8 && G % 16 == 0 && f.i8_stride16 == 0 && f.i8_addr15 == 0 && slab / 4 <= (size_t)kLds64K && rows_fit) {
        p.conv1 = Conv1::LDS_I8_SLAB, p.c1_lds = slab / 4;
    } else {
        p.conv1 = f.obs ? Conv1::DIRECT_F32 : Conv1::DIRECT_I8;
    }
    // conv2 (BN1 + ReLU on load; + BN2 statistics).  Its weight images were written by the conv1 kernel in passing.
    p.pz2 = planes_per_group(B, O2);
    p.XT = (O2 + 15) / 16;
    if (p.conv1 == Conv1::FUSED)
        p.conv2 = Conv2::FUSED, p.g2 = p.nitems;
    else if (t.splitx)
        p.conv2 = Conv2::SPLITX, p.g2 = splitx::items(B, O2, p.XT);
    else if (t.split)
        p.conv2 = Conv2::SPLIT, p.g2 = sample_plane_group_grid(B, O2, split::kNP);
    else
        p.conv2 = Conv2::FP32, p.g2 = sample_plane_group_grid(B, O2, p.pz2);
    p.bn2 = dp ? Bn2::DP : f.training ? Bn2::REDUCE : (t.fused_eval && f.eval_prepared) ? Bn2::NONE : Bn2::FINALIZE;
    // BN2 + ReLU -> flat features [B, 16*P2]: 256 elements per workgroup, grid-stride beyond 4096 workgroups
    const int64_t fg = ((int64_t)B * kC * p.P2 + 255) / 256;
    p.feat_grid = !f.features ? 0 : fg > 4096 ? 4096 : (int)fg;
    return p;
}

// gnbv_encoder_eval_prepare applies where the inference forward of the same facts is the one-launch kernel
static inline EncRefusal enc_eval_prepare_refusal(const EncFacts &f, const EncSwitches &s)
{
    return enc_paths(f, s).fused_eval ? EncRefusal::NONE : EncRefusal::NOT_APPLICABLE;
}

// ---- backward ----
enum class Wgrad2 { SPLITX_LOOP, SPLITX, SPLIT_DMA, SPLIT, FP32 };
enum class Dgrad { FUSED_SPLITX_LOOP, FUSED_SPLITX, FUSED_SPLIT, FUSED_FP32, PLAIN };  // FUSED_*: + the conv1 weight gradient
enum class Wgrad1 { FUSED, LDS_I8, LDS_F32, DIRECT_I8, DIRECT_F32 };                   // k_conv1_wgrad_lds<NR, NI> / k_conv1_wgrad

struct EncBackwardPlan {
    EncRefusal refusal;
    EncPaths paths;
    int O1, O2, P2;
    bool autocorr_launch;  // the minibatch total of the input autocorrelation is computed here: no per-row results, no saved total
    int ac_planes, ac_grid;
    size_t ac_lds;
    int bn2_apply_grid;
    Wgrad2 wgrad2;
    int wg_blocks;         // its workgroups = partial rows of kE2 floats in wg_part
    int wg_nitems, XT;
    int wg_slices;
    Dgrad dgrad;
    int gd;                // its workgroups = partial rows (FUSED_*: kE1F floats in wg1_part; PLAIN: BN rows in bn_part)
    int pzd, dg_nitems, dg_XT;
    Wgrad1 wgrad1;
    int NR, NI;            // 16-byte requests per lane and row of y1 / of the input
    int wg1_blocks;        // its workgroups = partial rows of kE1 floats in wg1_part
    size_t c1w_lds;
    int wg1_slices;        // stage-1 slices of wg1_part's rows (FUSED: of gd rows)
};

static inline EncBackwardPlan enc_backward_plan(const EncFacts &f, const EncSwitches &s)
{
    EncBackwardPlan p = {};
    const EncPaths &t = p.paths = enc_paths(f, s);
    const int B = f.batch, G = f.grid, O1 = p.O1 = out_size(G), O2 = p.O2 = out_size(O1), NA = (O1 + 1) / 2;
    p.P2 = O2 * O2 * O2;
    if (f.dp && !(t.saved_total && f.autocorr_global)) p.refusal = EncRefusal::DP_NEEDS_GLOBAL_AUTOCORR;
    p.autocorr_launch = t.fused_bwd && !t.saved_total && !f.autocorr;
    p.ac_planes = autocorr_planes(G);
    p.ac_grid = sample_plane_group_grid(B, O1, p.ac_planes);
    p.ac_lds = (size_t)(2 * p.ac_planes + 1) * G * G;
    p.bn2_apply_grid = B * ((p.P2 + 63) / 64);
    // ---- conv2 weight gradient ----
    p.XT = (O2 + 15) / 16;
    if (t.splitx) {
        p.wg_nitems = splitx::items(B, O2, p.XT);
        // one item per workgroup while the partial buffer holds a row per item (2 048 rows of kE2: the whole of wg_part); else
        // workgroups walk items (<= 512 rows)
        const bool loop = p.wg_nitems > 2048 || s.splitx_maxwg < 512;
        p.wgrad2 = loop ? Wgrad2::SPLITX_LOOP : Wgrad2::SPLITX;
        p.wg_blocks = loop ? imin(p.wg_nitems, s.splitx_maxwg) : p.wg_nitems;
    } else if (t.split) {
        p.wg_nitems = sample_plane_group_grid(B, O2, split::kNP);
        p.wgrad2 = s.wgrad_dma ? Wgrad2::SPLIT_DMA : Wgrad2::SPLIT;
        p.wg_blocks = s.wgrad_dma ? imin(p.wg_nitems, s.conv_maxwg) : p.wg_nitems;  // (one workgroup per CU by default)
    } else {
        // the fp32 kernel: FOUR rows per wave where there are fewer rows than 512 workgroups x 4 waves x 4 -- at the reference's 20^3 one
        // row per wave made the launch its epilogue, 512 workgroup-level reductions and 14 MB of partial rows for 2 048 rows of four
        // outputs: 128 workgroups -2.9 us per minibatch, 64: -1.4; profiles/r06_ab_train_g20_wgrad_blocks*.json
        const int blocks = (B * O2 * O2 + 4 * kEncWaves - 1) / (4 * kEncWaves);
        p.wgrad2 = Wgrad2::FP32;
        p.wg_blocks = blocks > 512 ? 512 : ((blocks + 7) & ~7);
    }
    p.wg_slices = reduce_slices(p.wg_blocks);
    // ---- conv2 data gradient (+ ReLU1 mask, BN1 backward sums) ----
    // The data gradient keeps four plane pairs per workgroup at every size: with two -- 384 workgroups at 20^3 -- or one -- 640 -- it
    // took 20-21 us instead of 16: every workgroup starts by copying the 27 KiB weight image, and that prologue is what these launches
    // are made of.  What does help is BALANCE at the same number of workgroups: the plane pairs of a sample in ceil(NA / 4) groups of
    // equal size -- at 20^3 (NA = 5) groups of 3 + 2 instead of 4 + 1: 15 super-tiles on a workgroup's 16 waves instead of 20, one
    // round: -2.2 us per minibatch (five in one group: +3.5; profiles/r06_ab_train_g20_dgrad_pz.json).  NA = 16, 32 stay at four.
    const int ngd = (NA + kPlanesPerGroup - 1) / kPlanesPerGroup;
    p.pzd = t.fused_bwd ? kPlanesPerGroup : (NA + ngd - 1) / ngd;
    p.gd = sample_plane_group_grid(B, NA, p.pzd);
    p.dg_XT = (NA + 15) / 16;
    if (!t.fused_bwd) {
        p.dgrad = Dgrad::PLAIN;
    } else if (t.splitx) {
        p.dg_nitems = dsplitx::items(B, NA, p.dg_XT);
        // one item per workgroup while wg1_part -- 1 536 rows of kE2 floats -- holds a row of kE1F floats per item; else T1 / S1 / S2
        // are kept across a workgroup's items: <= 512 partial rows
        const bool loop = (size_t)p.dg_nitems * kE1F > (size_t)1536 * kE2 || s.splitx_maxwg < 512;
        p.dgrad = loop ? Dgrad::FUSED_SPLITX_LOOP : Dgrad::FUSED_SPLITX;
        p.gd = loop ? imin(p.dg_nitems, s.splitx_maxwg) : p.dg_nitems;
    } else {
        p.dgrad = t.split ? Dgrad::FUSED_SPLIT : Dgrad::FUSED_FP32;
    }
    // ---- conv1 weight gradient (BN1 backward fused) ----
    if (t.fused_bwd) {
        p.wgrad1 = Wgrad1::FUSED;
        p.wg1_slices = reduce_slices(p.gd);
        return p;
    }
    // five rows per wave below the cap, for the same reason as the conv2 weight gradient above: 20^3, 2 048 -> 520 workgroups -6.7 us
    // per minibatch, 256: -4.2, 128: +4.3.  VGPR-light: 32 waves per CU hide the load latency
    const int blocks1 = (B * O1 * O1 + 5 * kEncWaves - 1) / (5 * kEncWaves);
    p.wg1_blocks = blocks1 > 2048 ? 2048 : ((blocks1 + 7) & ~7);
    p.wg1_slices = reduce_slices(p.wg1_blocks);
    const size_t lds = (size_t)kEncWaves * (2 * NA * kC + 9 * G) * sizeof(float);
    const int nr = (2 * NA * kC + 255) / 256, ni = (9 * G + 255) / 256;
    if (f.i8 && G % 16 == 0 && 9 * G <= 1024 && f.i8_stride16 == 0 && f.i8_addr15 == 0 && lds <= (size_t)kLds64K && nr <= 4) {
        p.wgrad1 = Wgrad1::LDS_I8, p.c1w_lds = lds;
        p.NR = nr <= 1 ? 1 : nr <= 2 ? 2 : 4, p.NI = 1;
    } else if (f.obs && G % 4 == 0 && f.obs_stride4 == 0 && f.obs_addr15 == 0 && lds <= (size_t)kLds64K && nr <= 4 && ni <= 5) {
        p.wgrad1 = Wgrad1::LDS_F32, p.c1w_lds = lds;
        if (nr <= 1 && ni <= 1) p.NR = 1, p.NI = 1;
        else if (nr <= 1 && ni <= 2) p.NR = 1, p.NI = 2;
        else if (nr <= 2 && ni <= 3) p.NR = 2, p.NI = 3;
        else p.NR = 4, p.NI = 5;
    } else {
        p.wgrad1 = f.obs ? Wgrad1::DIRECT_F32 : Wgrad1::DIRECT_I8;
    }
    return p;
}

// ---- workspace layout, in bytes from the (256-byte aligned) workspace ----
struct EncWsLayout {
    size_t bn_part, bn_part_bytes;  // BN partial rows of the largest producer (conv1 fwd / conv2 dgrad: B*O1 workgroups x 4 waves x 32 floats)
    size_t wg_part, wg_part_bytes;  // weight-gradient partials: 2 048 rows of kE2 floats
    size_t wg1_part;                // OVERLAPS wg_part from its row 512: the conv1 weight gradient's partials (fused: kE1F floats per row)
    size_t red;                     // fp64 reduction scratch, 8 192 doubles, 256-byte aligned; its named slots:
    size_t S2, S1;                  //   BN2 / BN1 backward sums [2][16] doubles
    size_t Rac;                     //   the autocorrelation total computed by the backward, kAcRow ints
    size_t dy2_absmax;              //   max |dy2| (bit patterns, 64 slots x 128 bytes): the gradient scale of the split kernels
    size_t tmp, tmp_bytes;          // stage-1 slices: 64 rows of kE2 doubles
    size_t tmp1;                    // OVERLAPS tmp from its row 32: the slices of the conv1 weight gradient
    size_t w2img, w2img_dgrad;      // fp32 conv2 weight images: forward, data gradient (6 912 floats each)
    size_t w2split, w2split_dgrad;  // split f16 weight images: forward, data gradient
    size_t w2split_bounds;          // the data-gradient image's |W2| bounds
    size_t total;
};
// The two overlaps, both kept apart by stream order (every launch of a call is on the caller's stream):
//  * wg_part / wg1_part: k_conv2_wgrad_splitx<false> may fill all 2 048 rows of wg_part; its stage-1 reduction has read them before the
//    data gradient (fused) or k_conv1_wgrad* writes wg1_part.
//  * tmp / tmp1: the stage-1 slices of the conv2 weight gradient (up to 64 rows) are consumed by k_conv2_wgrad_finish before the
//    conv1 weight gradient's stage 1 writes tmp1.
struct EncWsOverlap {
    const char *a, *a_launch, *b, *b_launch;
};
constexpr EncWsOverlap kEncWsOverlaps[] = {{"wg_part", "conv2_wgrad", "wg1_part", "conv1_wgrad"},
                                           {"tmp", "conv2_wgrad_reduce", "tmp1", "conv1_wgrad_reduce"}};

static inline EncWsLayout enc_ws_layout(int batch, int grid)
{
    EncWsLayout l = {};
    if (batch <= 0 || grid < 7) return l;
    l.bn_part_bytes = (size_t)(batch + 8) * out_size(grid) * kEncWaves * 2 * kC * sizeof(float);
    l.wg_part = l.bn_part + l.bn_part_bytes;
    l.wg_part_bytes = (size_t)2048 * kE2 * sizeof(float);
    l.wg1_part = l.wg_part + (size_t)512 * kE2 * sizeof(float);
    l.red = (l.wg_part + l.wg_part_bytes + 255) & ~(size_t)255;
    l.S2 = l.red + 128 * sizeof(double);
    l.S1 = l.red + 192 * sizeof(double);
    l.Rac = l.red + 1024 * sizeof(double);
    l.dy2_absmax = l.red + 2048 * sizeof(double);
    l.tmp = l.red + 8192 * sizeof(double);
    l.tmp_bytes = (size_t)kReduceSlices * kE2 * sizeof(double);
    l.tmp1 = l.tmp + (size_t)32 * kE2 * sizeof(double);
    l.w2img = l.tmp + l.tmp_bytes;
    l.w2img_dgrad = l.w2img + kTaps * 256 * sizeof(float);
    l.w2split = l.w2img + 2 * kTaps * 256 * sizeof(float);
    l.w2split_dgrad = l.w2split + kW2SplitImgBytes;
    l.w2split_bounds = l.w2split_dgrad + kW2SplitDgradSlotBytes;
    // (the slack behind the images covers the alignment of `red` and the data-gradient image's longer slot)
    l.total = l.bn_part_bytes + l.wg_part_bytes + 8192 * sizeof(double) + l.tmp_bytes + 2 * kTaps * 256 * sizeof(float) + 2 * kW2SplitImgBytes +
              1024 /*the |W2| bounds*/ + 8192 + 4096;
    return l;
}

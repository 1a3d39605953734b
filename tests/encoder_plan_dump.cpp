// Prints what csrc/encoder_plan.h decides.  Reads tuples from stdin -- 16 facts "batch grid training obs obs_addr15 obs_stride4 i8
// i8_addr15 i8_stride16 autocorr autocorr_total autocorr_global force_fp32 dp eval_prepared features", then the ten GENNBV_* knobs
// in kKnobs' order as the strings the environment would hold ("-": unset) -- sets the environment accordingly, reads the switches
// the way the library does, and writes one JSON object per tuple: the switches, the paths, both plans, the workspace layout.
// Host C++ only; tests/test_encoder_plan_cpu.py compiles and runs it.
#include "../gennbv_amd/csrc/encoder_plan.h"

#include <stdio.h>
#include <string.h>

static const char *const kKnobs[10] = {"GENNBV_CONV_SPLIT", "GENNBV_SPLITX", "GENNBV_SPLITX_MAXWG", "GENNBV_WGRAD_DMA", "GENNBV_CONV_MAXWG",
                                       "GENNBV_FUSED_BWD", "GENNBV_CONV1_SPLIT", "GENNBV_FUSED_TRAIN", "GENNBV_FUSED_EVAL", "GENNBV_ANALYTIC_BN1"};
static const char *const kRefusal[] = {"none", "dp", "not_applicable"};

int main()
{
    static const char *const kBn1[] = {"prepared", "prepare", "analytic", "reduce", "finalize"};
    static const char *const kConv1[] = {"fused", "split", "lds_i8", "lds_f32", "lds_i8_slab", "direct_i8", "direct_f32"};
    static const char *const kConv2[] = {"fused", "splitx", "split", "fp32"};
    static const char *const kBn2[] = {"none", "dp", "reduce", "finalize"};
    static const char *const kWgrad2[] = {"splitx_loop", "splitx", "split_dma", "split", "fp32"};
    static const char *const kDgrad[] = {"fused_splitx_loop", "fused_splitx", "fused_split", "fused_fp32", "plain"};
    static const char *const kWgrad1[] = {"fused", "lds_i8", "lds_f32", "direct_i8", "direct_f32"};
    int v[16];
    char knob[10][32];
    for (;;) {
        for (int i = 0; i < 16; ++i)
            if (scanf("%d", &v[i]) != 1) return i == 0 ? 0 : 1;
        for (int i = 0; i < 10; ++i) {
            if (scanf("%31s", knob[i]) != 1) return 1;
            if (strcmp(knob[i], "-") == 0) unsetenv(kKnobs[i]);
            else setenv(kKnobs[i], knob[i], 1);
        }
        EncFacts f = {};
        f.batch = v[0], f.grid = v[1], f.training = v[2], f.obs = v[3], f.obs_addr15 = v[4], f.obs_stride4 = v[5], f.i8 = v[6], f.i8_addr15 = v[7];
        f.i8_stride16 = v[8], f.autocorr = v[9], f.autocorr_total = v[10], f.autocorr_global = v[11], f.force_fp32 = v[12], f.dp = v[13];
        f.eval_prepared = v[14], f.features = v[15];
        const EncSwitches s = enc_switches_from_env();
        const EncPaths t = enc_paths(f, s);
        const EncForwardPlan fw = enc_forward_plan(f, s);
        EncFacts fb = f;
        fb.training = true;  // (a backward follows a training forward of the same inputs)
        const EncBackwardPlan bw = enc_backward_plan(fb, s);
        const EncWsLayout l = enc_ws_layout(f.batch, f.grid);
        printf("{\"switches\": {\"conv_split\": %d, \"splitx\": %d, \"splitx_maxwg\": %d, \"conv_maxwg\": %d, \"wgrad_dma\": %d, \"fused_bwd\": %d, "
               "\"conv1_split\": %d, \"fused_train\": %d, \"fused_eval\": %d, \"analytic_bn1\": %d}, ",
               s.conv_split, s.splitx, s.splitx_maxwg, s.conv_maxwg, s.wgrad_dma, s.fused_bwd, s.conv1_split, s.fused_train, s.fused_eval, s.analytic_bn1);
        printf("\"paths\": {\"split\": %d, \"splitx\": %d, \"fused_bwd\": %d, \"i8_staged\": %d, \"analytic\": %d, \"fused_eval\": %d, \"fused_train\": %d, "
               "\"saved_total\": %d}, \"eval_prepare\": \"%s\", ",
               t.split, t.splitx, t.fused_bwd, t.i8_staged, t.analytic, t.fused_eval, t.fused_train, t.saved_total,
               kRefusal[(int)enc_eval_prepare_refusal(f, s)]);
        printf("\"fwd\": {\"refusal\": \"%s\", \"split\": %d, \"splitx\": %d, \"fused_bwd\": %d, \"saved_total\": %d, \"O1\": %d, \"O2\": %d, \"P2\": %d, "
               "\"bn1\": \"%s\", \"bn1_grid\": %d, \"have_total\": %d, \"conv1\": \"%s\", \"c1_grid\": %d, \"c1_lds\": %zu, \"c1_part\": %d, "
               "\"split_img\": %d, \"nitems\": %d, \"conv2\": \"%s\", \"g2\": %d, \"XT\": %d, \"pz2\": %d, \"bn2\": \"%s\", \"feat_grid\": %d}, ",
               kRefusal[(int)fw.refusal], fw.paths.split, fw.paths.splitx, fw.paths.fused_bwd, fw.paths.saved_total, fw.O1, fw.O2, fw.P2,
               kBn1[(int)fw.bn1], fw.bn1_grid, fw.have_total, kConv1[(int)fw.conv1], fw.c1_grid, fw.c1_lds, fw.c1_part, fw.split_img, fw.nitems,
               kConv2[(int)fw.conv2], fw.g2, fw.XT, fw.pz2, kBn2[(int)fw.bn2], fw.feat_grid);
        printf("\"bwd\": {\"refusal\": \"%s\", \"split\": %d, \"splitx\": %d, \"fused_bwd\": %d, \"saved_total\": %d, \"autocorr_launch\": %d, "
               "\"ac_planes\": %d, \"ac_grid\": %d, \"ac_lds\": %zu, \"bn2_apply_grid\": %d, \"wgrad2\": \"%s\", \"wg_blocks\": %d, \"wg_nitems\": %d, "
               "\"XT\": %d, \"wg_slices\": %d, \"dgrad\": \"%s\", \"gd\": %d, \"pzd\": %d, \"dg_nitems\": %d, \"dg_XT\": %d, \"wgrad1\": \"%s\", "
               "\"NR\": %d, \"NI\": %d, \"wg1_blocks\": %d, \"c1w_lds\": %zu, \"wg1_slices\": %d}, ",
               kRefusal[(int)bw.refusal], bw.paths.split, bw.paths.splitx, bw.paths.fused_bwd, bw.paths.saved_total, bw.autocorr_launch, bw.ac_planes,
               bw.ac_grid, bw.ac_lds, bw.bn2_apply_grid, kWgrad2[(int)bw.wgrad2], bw.wg_blocks, bw.wg_nitems, bw.XT, bw.wg_slices, kDgrad[(int)bw.dgrad],
               bw.gd, bw.pzd, bw.dg_nitems, bw.dg_XT, kWgrad1[(int)bw.wgrad1], bw.NR, bw.NI, bw.wg1_blocks, bw.c1w_lds, bw.wg1_slices);
        printf("\"ws\": {\"bn_part\": %zu, \"bn_part_bytes\": %zu, \"wg_part\": %zu, \"wg_part_bytes\": %zu, \"wg1_part\": %zu, \"red\": %zu, \"S2\": %zu, "
               "\"S1\": %zu, \"Rac\": %zu, \"dy2_absmax\": %zu, \"tmp\": %zu, \"tmp_bytes\": %zu, \"tmp1\": %zu, \"w2img\": %zu, \"w2img_dgrad\": %zu, "
               "\"w2split\": %zu, \"w2split_dgrad\": %zu, \"w2split_bounds\": %zu, \"total\": %zu, \"overlaps\": [",
               l.bn_part, l.bn_part_bytes, l.wg_part, l.wg_part_bytes, l.wg1_part, l.red, l.S2, l.S1, l.Rac, l.dy2_absmax, l.tmp, l.tmp_bytes, l.tmp1,
               l.w2img, l.w2img_dgrad, l.w2split, l.w2split_dgrad, l.w2split_bounds, l.total);
        for (size_t i = 0; i < sizeof(kEncWsOverlaps) / sizeof(kEncWsOverlaps[0]); ++i)
            printf("%s[\"%s\", \"%s\", \"%s\", \"%s\"]", i ? ", " : "", kEncWsOverlaps[i].a, kEncWsOverlaps[i].a_launch, kEncWsOverlaps[i].b,
                   kEncWsOverlaps[i].b_launch);
        printf("]}}\n");
    }
}

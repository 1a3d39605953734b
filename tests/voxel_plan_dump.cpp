// Prints the launch plan csrc/voxel_plan.h makes: reads "n g h w has_lists large slab_override" tuples from stdin (large: -1, 0 or
// 1) and writes one JSON object per tuple.  Host C++ only; tests/test_voxel_abi_regimes_cpu.py compiles and runs it.
#include "../gennbv_amd/csrc/voxel_plan.h"

#include <stdio.h>

int main()
{
    static const char *const kRegime[] = {"list", "large", "round1"};
    int n, g, h, w, has_lists, large, slab_override;
    while (scanf("%d %d %d %d %d %d %d", &n, &g, &h, &w, &has_lists, &large, &slab_override) == 7) {
        const VoxelMaskPlan p = voxel_mask_plan(n, g, h, w, has_lists != 0, large, slab_override);
        printf("{\"regime\": \"%s\", \"words\": %d, \"env_groups\": %d, \"fchunks\": %d, \"chunks\": %d, \"splits\": %d, ",
               kRegime[(int)p.regime], p.words, p.env_groups, p.fchunks, p.chunks, p.splits);
        printf("\"hit_windows\": %d, \"path_windows\": %d, \"hit_nw\": %d, \"path_nw\": %d, ", p.hit_windows, p.path_windows, p.hit_nw,
               p.path_nw);
        printf("\"list_lds\": %zu, \"ray_list_lds\": %zu, \"hit_lds\": %zu, \"path_lds\": %zu, ", p.list_lds, p.ray_list_lds, p.hit_lds,
               p.path_lds);
        printf("\"slab_align\": %d, \"slab_planes\": %d, \"slabs\": %d, \"slab_slices\": %d, \"slab_lds\": %zu, ", p.slab_align,
               p.slab_planes, p.slabs, p.slab_slices, p.slab_lds);
        printf("\"hit_grid\": %d, \"ray_grid\": %d, \"zero_offset\": %zu, \"zero_bytes\": %zu, \"zero_coverage\": %d, ", p.hit_grid,
               p.ray_grid, p.zero_offset, p.zero_bytes, (int)p.zero_coverage);
        printf("\"ws_bytes\": %zu, \"ws_bytes_hw\": %zu, \"ray_count_ints\": %zu, \"ray_list_cap\": %lld}\n", voxel_workspace_bytes(n, g),
               voxel_workspace_bytes_hw(n, g, h, w), ray_count_ints(n), (long long)ray_list_cap(g, h, w));
    }
    return 0;
}

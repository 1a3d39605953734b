// The integer walk of gennbv_amd/csrc/ray_walk.h compiled for the host: the ray record of k_vg_fate and the slab cut of k_vg_slab
// (viewgain.hip) with the header's own make_walk, run_walk, make_slab_cut and walk_steps.  tests/test_ray_walk_host_cpu.py
// compiles and runs it.
//
// stdin, one ray per line:  g height x0 y0 z0 x1 y1 z1 occ      (occ: linear index of the one occupied voxel, -1 for none)
// stdout per ray:           R first count blocked xa xb          the record, as k_vg_fate packs it
//                           S X0 lin lin ...                     per slab [X0, X0 + height) that marks a voxel: the grid-linear
//                                                                indices in the order visited
#include <cstdio>

#include "ray_walk.h"

int main()
{
    int g, height, x0, y0, z0, x1, y1, z1, occ;
    while (scanf("%d %d %d %d %d %d %d %d %d", &g, &height, &x0, &y0, &z0, &x1, &y1, &z1, &occ) == 9) {
        const int gg = g * g;
        // ---- k_vg_fate
        const RayWalk rw = make_walk(x0, y0, z0, x1, y1, z1, g);
        int first = 0, last = -1, lin_first = 0, lin_last = 0;
        bool blocked = false;
        if (rw.n > 0)
            blocked = run_walk(rw, g, [&](int lin, int i) {
                if (lin == occ) return true;
                if (last < 0) { first = i; lin_first = lin; }
                last = i; lin_last = lin;
                return false;
            });
        const int count = last < 0 ? 0 : last - first + 1;
        const int xf = lin_first / gg, xl = lin_last / gg, xa = xf < xl ? xf : xl, xb = xf < xl ? xl : xf;
        const int rec_first = rw.n > 0 ? rw.i0 + first : 0;
        printf("R %d %d %d %d %d\n", rec_first, count, blocked ? 1 : 0, xa, xb);
        // ---- k_vg_slab, every slab in turn
        for (int X0 = 0; X0 < g; X0 += height) {
            const int X1 = X0 + height < g ? X0 + height : g;
            if (count == 0 || xb < X0 || xa >= X1) continue;
            const unsigned svox = (unsigned)((X1 - X0) * gg);
            const RayWalk w = make_slab_cut(x0, y0, z0, x1, y1, z1, g, rec_first, count, X0, X1);
            bool any = false;
            walk_steps(w, [svox](const RayWalk &s) { return (unsigned)s.lin < svox; }, [&](int lin, int) {
                if (!any) printf("S %d", X0);
                any = true;
                printf(" %d", lin + X0 * gg);
                return false;
            });
            if (any) printf("\n");
        }
    }
    return 0;
}

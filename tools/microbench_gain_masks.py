"""Microbenchmark of the view gain that keeps its masks (gnbv_view_gain_masks; gnbv_view_gain_slab_masks above 64^3) beside the
view gain it extends, and of the set-cover plan on the masks (ViewGainMasks.plan, one gnbv_cover_greedy launch).

    python tools/microbench_gain_masks.py [--repeats 7] [--iters 5] [--cases ...] [--parent-lib PATH] [--chunk 0] [--envs128 64]
                                          [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call.
Cases (N, G, camera, stride, K), each on all-unknown grids and on mid-episode grids (10 closed-loop steps of random lattice poses):

  g64_k8      256, 64^3, 240x320, 4, 8
  g64_k32     256, 64^3, 240x320, 4, 32
  g20_k32     8, 20^3, 240x320, 4, 32
  g128_k8     64, 128^3, 240x320, 4, 8      (not in the default list: --cases g128_k8,g128_k32; --envs128 changes the 64.  A row
  g128_k32    64, 128^3, 240x320, 4, 32      is 256 KiB: 64 envs x 32 x both masks = 1 GiB, 512 envs = 8 GiB per operator, and three
                                             masks operators are alive at a time.)  Above 64^3 the operators are make_view_gain's
                                             and make_view_gain_masks': gnbv_view_gain_slab and gnbv_view_gain_slab_masks; a parent
                                             build without the latter times gnbv_view_gain_slab only.

Rows per grid: gnbv_view_gain of this build; the same call on the library at --parent-lib (another build of the same ABI, e.g. the
parent commit's: _lib.activate), on the same grids and poses; gnbv_view_gain_masks with both masks, the hit mask only, the unknown
mask only.  Beside every masks row: the bytes the call stores more than gnbv_view_gain (n k words 4 per mask), its extra time over
this build's gnbv_view_gain, and the store rate the two imply.  Then, for horizon 1, 3 and 5: `plan(horizon)` on the hit mask and
on the unknown mask, `plan_weighted(horizon, weights)` on both (one gnbv_cover_greedy_w launch; --weights, default 1,4), the sum
of the two single-mask plans it is set against, and -- with --parent-lib -- the two single-mask plans of that build on the same
masks, then the A/B of tools/microbench_cover_greedy.py (`ab`: this build, that build, that build again, alternated in one call,
both builds on this build's masks after asserting equal masks and outputs) for `plan("hit")`, `plan("unknown")` and, where that
build has gnbv_cover_greedy_w, `plan_weighted`.  With --parent-lib the kernel calls themselves get the same A/B, after the same
assertion: `view_gain_ab` (gnbv_view_gain, or gnbv_view_gain_slab above 64^3) and `masks_both_ab`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gennbv_amd import _lib  # noqa: E402
from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.eval.baselines import LatticeCandidates  # noqa: E402
from gennbv_amd.ops.gain_masks import make_view_gain_masks  # noqa: E402
from gennbv_amd.ops.view_gain import MAX_GRID, make_view_gain  # noqa: E402
from tools.microbench_cover_greedy import ab  # noqa: E402
from tools.microbench_render import time_calls  # noqa: E402
from tools.microbench_view_gain import mid_episode_grid, stats  # noqa: E402

DEV = "cuda:0"


def masks_case(name, n, g, h, w, stride, k, args):
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    lc = LatticeCandidates(cfg, k, seed=3)
    poses = lc.poses(lc.sample(n)).to(DEV)
    grids = {"all_unknown": torch.zeros(n, g ** 3, dtype=torch.int8, device=DEV), "mid_episode": mid_episode_grid(cfg, n, scene)}
    kw = dict(stride=stride, device=DEV, chunk=args.chunk)
    ops = {"view_gain": make_view_gain(n, k, cfg, scene.range_gt, scene.voxel_size, **kw)}
    if args.parent_lib:
        _lib.activate(args.parent_lib)  # an operator keeps the library that was active when it was built
        ops["view_gain_parent"] = make_view_gain(n, k, cfg, scene.range_gt, scene.voxel_size, **kw)
        if g <= MAX_GRID or hasattr(_lib.load(), "gnbv_view_gain_slab_masks"):
            ops["masks_both_parent"] = make_view_gain_masks(n, k, cfg, scene.range_gt, scene.voxel_size, **kw)
        _lib.activate()
    ops["masks_both"] = make_view_gain_masks(n, k, cfg, scene.range_gt, scene.voxel_size, **kw)
    ops["masks_hit"] = make_view_gain_masks(n, k, cfg, scene.range_gt, scene.voxel_size, unknown=False, **kw)
    ops["masks_unknown"] = make_view_gain_masks(n, k, cfg, scene.range_gt, scene.voxel_size, hit=False, **kw)
    words = ops["masks_both"].words
    mask_bytes = n * k * words * 4
    weights = tuple(int(w) for w in args.weights.split(","))
    out = {"case": name, "weights": weights, "envs": n, "grid": g, "h": h, "w": w, "stride": stride, "k": k, "chunk": args.chunk, "words": words,
           "mask_bytes": mask_bytes}
    for gname, tri in grids.items():
        want = ops["view_gain"](tri, poses).clone()
        for oname, op in ops.items():
            assert torch.equal(op(tri, poses), want), oname
            out[f"{gname}_{oname}"] = stats(time_calls(lambda: op(tri, poses), args.iters, args.repeats))
        for oname in ("view_gain", "masks_both"):  # the kernel calls themselves, this build against that build
            if oname + "_parent" in ops:
                mine, par = ops[oname], ops[oname + "_parent"]
                if oname == "masks_both":
                    assert torch.equal(mine.unknown_bits, par.unknown_bits) and torch.equal(mine.hit_bits, par.hit_bits)
                ab(out, f"{gname}_{oname}", [lambda: mine(tri, poses)] + [lambda: par(tri, poses)] * 2, args.iters, args.repeats)
        base = out[f"{gname}_view_gain"]["us_median"]
        for oname, masks in (("masks_both", 2), ("masks_hit", 1), ("masks_unknown", 1)):
            row = out[f"{gname}_{oname}"]
            row["extra_bytes"] = masks * mask_bytes
            row["extra_us"] = row["us_median"] - base
            row["implied_GB_per_s"] = masks * mask_bytes / row["extra_us"] * 1e-3 if row["extra_us"] > 0 else None
        both = ops["masks_both"]
        both(tri, poses)
        plans = {"": both}
        if "masks_both_parent" in ops:
            plans["_parent"] = ops["masks_both_parent"]
            plans["_parent"](tri, poses)
        for horizon in (1, 3, 5):
            for tag, op in plans.items():
                out[f"{gname}_plan_{horizon}{tag}"] = stats(time_calls(lambda: op.plan(horizon, which="hit"), args.iters, args.repeats))
                out[f"{gname}_plan_unknown_{horizon}{tag}"] = stats(time_calls(lambda: op.plan(horizon, which="unknown"), args.iters, args.repeats))
            row = stats(time_calls(lambda: both.plan_weighted(horizon, weights=weights), args.iters, args.repeats))
            row["hit_plus_unknown_us"] = out[f"{gname}_plan_{horizon}"]["us_median"] + out[f"{gname}_plan_unknown_{horizon}"]["us_median"]
            out[f"{gname}_plan_weighted_{horizon}"] = row
        if "_parent" in plans:
            par = plans["_parent"]
            own = par.unknown_bits, par.hit_bits  # the same masks for both libraries: where two rows lie changes a two-plane read
            assert torch.equal(own[0], both.unknown_bits) and torch.equal(own[1], both.hit_bits)
            par.unknown_bits, par.hit_bits = both.unknown_bits, both.hit_bits
            calls = {"plan": lambda op, t: op.plan(t, which="hit"), "plan_unknown": lambda op, t: op.plan(t, which="unknown")}
            if hasattr(par.lib, "gnbv_cover_greedy_w"):
                calls["plan_weighted"] = lambda op, t: (lambda c, g, cov: (c, g, *cov))(*op.plan_weighted(t, weights=weights))
            for horizon in (1, 3, 5):
                for cname, call in calls.items():
                    mine = [t.clone() for t in call(both, horizon)] + [both.gains0.clone()]
                    assert all(torch.equal(x, y) for x, y in zip(mine, [*call(par, horizon), par.gains0])), (cname, horizon)
                    ab(out, f"{gname}_{cname}_{horizon}", [lambda: call(both, horizon)] + [lambda: call(par, horizon)] * 2, args.iters, args.repeats)
            par.unknown_bits, par.hit_bits = own
        out[gname + "_mean_plan5_weighted_plane_gain"] = both.plane_gain.float().mean(dim=0).tolist()
        out[gname + "_mean_gain"] = want.float().mean(dim=(0, 1)).tolist()
        out[gname + "_mean_plan5_gain"] = both.plan(5, which="hit")[1].float().mean(dim=0).tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cases", default="g64_k8,g64_k32,g20_k32")
    ap.add_argument("--parent-lib", default=None, help="another build of libgennbv_hip.so (the same ABI) to time gnbv_view_gain on")
    ap.add_argument("--weights", default="1,4", help="w_unknown,w_hit of the weighted plan")
    ap.add_argument("--chunk", type=int, default=0, help="candidates per workgroup (0 = chosen)")
    ap.add_argument("--envs128", type=int, default=64, help="envs of the 128^3 cases")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_gain_masks needs a GPU")
    table = {"g64_k8": (256, 64, 240, 320, 4, 8), "g64_k32": (256, 64, 240, 320, 4, 32), "g20_k32": (8, 20, 240, 320, 4, 32),
             "g128_k8": (args.envs128, 128, 240, 320, 4, 8), "g128_k32": (args.envs128, 128, 240, 320, 4, 32)}
    results = []
    for c in args.cases.split(","):
        if c not in table:
            raise SystemExit("unknown case " + c)
        r = masks_case(c, *table[c], args)
        print(json.dumps(r), flush=True)
        results.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Microbenchmark of the view pool: building the masks (gnbv_view_cover_masks) and deciding on them (gnbv_cover_greedy).

    python tools/microbench_cover_greedy.py [--envs 256] [--grid 64] [--pool 256] [--repeats 7] [--iters 2] [--parts build,select,plan]
                                            [--parent-lib PATH] [--out FILE.json]

The protocol of tools/microbench_view_cover.py: device events around `iters` back-to-back calls, after warm-up, `repeats` times,
the alternatives of one part alternated repeat by repeat in one process; reported: median / min / max us per call.  Box scenes
(make_scenes), 240 x 320 camera, stride 1, look-at-scene lattice poses.

  build    ViewPool(...) for `pool` views per env (masks, union, staging copies; 1 call per repeat), beside the same candidate
           count through ViewCover.__call__ in batches of 64 (the trace with three integers per candidate instead of a mask row)
  select   one decision over the pool against a mid-episode covered set (the covered set of plan(5)): exhaustive (every mask
           read: bytes = N P vwords 4 + N vwords 4, against the 8 TB/s roof), with carried bounds (the bounds left by the
           decision before, restored before each call), and beside them the one-step oracle's decision on the same state:
           ViewCover (K = 32) + choose
  plan     plan(20) from the empty set, lazy against exhaustive

--parent-lib PATH (another build of libgennbv_hip.so with the same ABI, e.g. the parent commit's: _lib.activate) adds an A/B of
gnbv_cover_greedy to `select` and `plan`: per row, three series alternated repeat by repeat in one alternate(...) call -- this
build, the library at PATH on the same masks, and that library a second time -- after asserting that both libraries give the same
outputs.  `noise_floor_us` is the larger of the gap between the two PATH medians and the wider min-max of the two; `within_noise`
says whether this build's median exceeds the first PATH median by no more than that.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gennbv_amd import _lib  # noqa: E402
from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.state_encoding import OccupancyGridUpdater  # noqa: E402
from gennbv_amd.eval.baselines import LatticeCandidates, choose  # noqa: E402
from gennbv_amd.ops.cover_greedy import CoverGreedy  # noqa: E402
from gennbv_amd.ops.view_cover import ViewCover  # noqa: E402
from gennbv_amd.ops.view_pool import UNKNOWN, ViewPool  # noqa: E402
from tools.microbench_view_cover import alternate, stats  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12


def on_library(pool, lib):
    """`pool`'s masks and contact under another build of the library, with outputs of its own"""
    par = copy.copy(pool)
    par.lib, par._cg = lib, CoverGreedy(lib, pool.device, pool.num_envs, pool.pool_size, pool.words)
    par._gains, par._choice1, par._gain1 = (torch.empty_like(t) for t in (pool._gains, pool._choice1, pool._gain1))
    return par


def ab(res, name, fns, iters, repeats):
    """res[name + "_ab"]: this build / the parent library / the parent library again, alternated in one call"""
    this, par, again = (stats(us) for us in alternate(fns, iters, repeats))
    width = lambda r: r["us_max"] - r["us_min"]
    floor = max(abs(par["us_median"] - again["us_median"]), width(par), width(again))
    over = this["us_median"] - par["us_median"]
    res[name + "_ab"] = {"this": this, "parent": par, "parent_again": again, "noise_floor_us": floor, "over_parent_us": over,
                         "within_noise": over <= floor}
    print(json.dumps({name + "_ab": res[name + "_ab"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--oracle-k", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--parts", default="build,select,plan")
    ap.add_argument("--parent-lib", default=None, help="another build of libgennbv_hip.so (the same ABI) to set gnbv_cover_greedy against")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_cover_greedy needs a GPU")
    n, g, p, h, w = args.envs, args.grid, args.pool, 240, 320
    parts = args.parts.split(",")
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    upd = OccupancyGridUpdater(n, g, h, w, S.inverse_intrinsics(h, w, cfg.horizontal_fov), scene.range_gt, scene.voxel_size, scene.grid_gt,
                               DEV, cfg.depth_sense_dist)
    gt = upd.gt_bits
    lc = LatticeCandidates(cfg, p, seed=3, look_at_scene=True)
    poses = lc.poses(lc.sample(n)).to(DEV)
    res = {"envs": n, "grid": g, "pool": p, "h": h, "w": w}

    def build():
        return ViewPool(mesh, cfg, scene.range_gt, scene.voxel_size, gt, poses)

    pool = build()
    vwords = (((g ** 3 + 31) // 32) + 3) & ~3
    res["mask_bytes"] = pool.masks.numel() * 4
    if "build" in parts:
        kb = min(64, p)
        vc = ViewCover(mesh, cfg, scene.range_gt, scene.voxel_size, kb)
        cols = [poses[:, j:j + kb].contiguous() for j in range(0, p - kb + 1, kb)]

        def counted():
            for c in cols:
                vc(c, gt, None)
        del pool
        torch.cuda.empty_cache()
        b, c = alternate([build, counted], 1, max(3, args.repeats // 2), warmup=1)
        res["build"], res["view_cover_same_candidates"] = stats(b), stats(c)
        res["build_over_view_cover"] = res["build"]["us_median"] / res["view_cover_same_candidates"]["us_median"]
        print(json.dumps({k: res[k] for k in ("build", "view_cover_same_candidates", "build_over_view_cover")}), flush=True)
        pool = build()
    pars = []
    if args.parent_lib:
        pars = [on_library(pool, _lib.activate(args.parent_lib)) for _ in range(2)]
        _lib.activate()
        res["parent_lib"] = os.path.basename(args.parent_lib)
    if "select" in parts:
        cov4 = pool.plan(4)[2].clone()
        cov5 = pool.plan(5)[2].clone()
        ub0 = torch.full((n, p), UNKNOWN, dtype=torch.int32, device=DEV)
        want = tuple(t.clone() for t in pool.select(cov5))
        pool.select(cov4, ub0)  # the bounds a decision leaves for the next one
        ub = ub0.clone()
        assert all(torch.equal(x, y) for x, y in zip(pool.select(cov5, ub), want))
        ko = args.oracle_k
        vco = ViewCover(mesh, cfg, scene.range_gt, scene.voxel_size, ko)
        poses_o = poses[:, :ko].contiguous()

        def carried():
            ub.copy_(ub0)
            pool.select(cov5, ub)

        ex, ca, orc = alternate([lambda: pool.select(cov5), carried, lambda: choose(vco(poses_o, gt, cov5), (1, 0))], args.iters, args.repeats)
        res["select_exhaustive"], res["select_carried_bounds"], res["oracle_decision"] = stats(ex), stats(ca), stats(orc)
        nbytes = n * p * vwords * 4 + n * vwords * 4
        res["select_bytes"] = nbytes
        res["select_fraction_of_hbm_roof"] = nbytes / (res["select_exhaustive"]["us_median"] * 1e-6) / HBM_BYTES_PER_S
        res["oracle_over_select"] = res["oracle_decision"]["us_median"] / res["select_exhaustive"]["us_median"]
        print(json.dumps({k: res[k] for k in ("select_exhaustive", "select_carried_bounds", "oracle_decision", "select_bytes",
                                              "select_fraction_of_hbm_roof", "oracle_over_select")}), flush=True)
        if pars:
            ubs = [ub0.clone() for _ in pars]
            pool.select(cov5)
            for q, u in zip(pars, ubs):
                assert all(torch.equal(x, y) for x, y in zip(q.select(cov5), want)) and torch.equal(q._gains, pool._gains)
                assert all(torch.equal(x, y) for x, y in zip(q.select(cov5, u), want)) and torch.equal(u, ub)

            def carried_on(q, u):
                def f():
                    u.copy_(ub0)
                    q.select(cov5, u)
                return f
            ab(res, "select_exhaustive", [lambda: pool.select(cov5)] + [lambda q=q: q.select(cov5) for q in pars], args.iters, args.repeats)
            ab(res, "select_carried_bounds", [carried] + [carried_on(q, u) for q, u in zip(pars, ubs)], args.iters, args.repeats)
    if "plan" in parts:
        r = args.rounds
        a = tuple(t.clone() for t in pool.plan(r, None, lazy=True))
        assert all(torch.equal(x, y) for x, y in zip(a, pool.plan(r, None, lazy=False)))
        lz, ex = alternate([lambda: pool.plan(r, None, lazy=True), lambda: pool.plan(r, None, lazy=False)], args.iters, args.repeats)
        res["plan_lazy"], res["plan_exhaustive"], res["plan_rounds"] = stats(lz), stats(ex), r
        print(json.dumps({k: res[k] for k in ("plan_rounds", "plan_lazy", "plan_exhaustive")}), flush=True)
        for q in pars:
            for lazy in (True, False):
                assert all(torch.equal(x, y) for x, y in zip(a, q.plan(r, None, lazy=lazy))) and torch.equal(q._gains, pool._gains)
        if pars:
            for name, lazy in (("plan_lazy", True), ("plan_exhaustive", False)):
                ab(res, name, [lambda: pool.plan(r, None, lazy=lazy)] + [lambda q=q: q.plan(r, None, lazy=lazy) for q in pars], args.iters, args.repeats)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Microbenchmark of the view coverage (gnbv_view_cover) beside the composed path it replaces.

    python tools/microbench_view_cover.py [--repeats 7] [--iters 2] [--cases ...] [--chunk 0] [--window 0] [--parent-lib PATH]
                                          [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call.
The fused call and the composed path run in the same process, alternated repeat by repeat, on the same mid-episode state
(5 updates from random look-at-scene poses).  Cases (N, G, camera, stride, K):

  g64_s1     256, 64^3, 240x320, 1, 32   box scenes; fused and composed
  g64_s4     256, 64^3, 240x320, 4, 32   box scenes; fused only (the composed path has no strided form)
  dense_s1   64, 64^3, 240x320, 1, 32    the dense 19 900-triangle scene of tools/microbench_render.py; fused and composed
  g128_s1    128, 128^3, 240x320, 1, 32  box scenes, the windowed kernel; fused and composed

The composed path, per candidate column j: restore the updater's state (scanned bits and probability codes), gnbv_render_depth
at poses[:, j], OccupancyGridUpdater.update, read coverage_count.  Its parts are also timed alone (`render_us`, `update_us`,
`restore_us`: one column each).  Each case checks once that the composed increments equal the fused new_gt.

--parent-lib PATH (another build of libgennbv_hip.so with the same ABI, e.g. the parent commit's: _lib.activate) adds `fused_ab`, the
A/B of tools/microbench_cover_greedy.py (`ab`: this build, that build, that build again, alternated in one call) for the ViewCover
call, after asserting that both builds give equal outputs.

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/microbench_view_cover.py` run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gennbv_amd import _lib  # noqa: E402
from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.state_encoding import OccupancyGridUpdater  # noqa: E402
from gennbv_amd.eval.baselines import LatticeCandidates  # noqa: E402
from gennbv_amd.ops.view_cover import ViewCover  # noqa: E402
from tools.microbench_render import dense_mesh, time_calls  # noqa: E402

DEV = "cuda:0"


def stats(us):
    med = float(np.median(us))
    return {"us_median": med, "us_min": float(min(us)), "us_max": float(max(us))}


def alternate(fns, iters, repeats, warmup=2):
    """time_calls' protocol for several callables, alternated repeat by repeat -> one list of us per callable"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[i].append(a.elapsed_time(b) * 1e3 / iters)
    return out


def cover_case(name, mesh, scene, n, g, h, w, stride, k, args, composed=True):
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    lc = LatticeCandidates(cfg, k, seed=3, look_at_scene=True)
    poses = lc.poses(lc.sample(n)).to(DEV)
    kinv = S.inverse_intrinsics(h, w, cfg.horizontal_fov)
    upd = OccupancyGridUpdater(n, g, h, w, kinv, scene.range_gt, scene.voxel_size, scene.grid_gt, DEV, cfg.depth_sense_dist,
                               max_steps_between_resets=101)
    feed = RenderFeed(mesh, cfg, with_rgba=False)
    warm = LatticeCandidates(cfg, 5, seed=9, look_at_scene=True)
    for p in warm.poses(warm.sample(n)).to(DEV).unbind(1):  # the mid-episode state
        p = p.contiguous()
        d, s, _, c2w = feed.render(p)
        upd.update(d, s, c2w, p)
    scanned0, count0 = upd.scanned_bits.clone(), upd.coverage_count.clone()
    code0 = upd.prob_code.clone() if upd.coded else upd._prob_f32.clone()
    cols = [poses[:, j].contiguous() for j in range(k)]
    inc = torch.empty(n, k, dtype=torch.int32, device=DEV)
    vc = ViewCover(mesh, cfg, scene.range_gt, scene.voxel_size, k, stride=stride, chunk=args.chunk, window=args.window)

    def restore():
        upd.scanned_bits.copy_(scanned0)
        (upd.prob_code if upd.coded else upd._prob_f32).copy_(code0)

    def composed_call():
        for j in range(k):
            restore()
            d, s, _, c2w = feed.render(cols[j])
            upd.update(d, s, c2w, cols[j])
            torch.sub(upd.coverage_count, count0, out=inc[:, j])
        restore()

    def fused_call():
        vc(poses, upd.gt_bits, scanned0)

    out = {"case": name, "envs": n, "grid": g, "h": h, "w": w, "stride": stride, "k": k, "chunk": args.chunk, "window": args.window,
           "triangles_per_env": mesh.num_triangles // n}
    if composed:
        composed_call()
        out["equal_to_composed"] = bool(torch.equal(vc(poses, upd.gt_bits, scanned0)[..., 0], inc))
        f, c = alternate([fused_call, composed_call], args.iters, args.repeats)
        out["fused"], out["composed"] = stats(f), stats(c)
        out["ratio_composed_over_fused"] = out["composed"]["us_median"] / out["fused"]["us_median"]
        d, s, _, c2w = feed.render(cols[0])
        out["render_us"] = stats(time_calls(lambda: feed.render(cols[0]), args.iters * 4, args.repeats))
        out["update_us"] = stats(time_calls(lambda: upd.update(d, s, c2w, cols[0]), args.iters * 4, args.repeats))
        out["restore_us"] = stats(time_calls(restore, args.iters * 4, args.repeats))
        restore()
    else:
        out["fused"] = stats(alternate([fused_call], args.iters, args.repeats)[0])
    if args.parent_lib:
        from tools.microbench_cover_greedy import ab  # (that module imports this one)
        _lib.activate(args.parent_lib)  # an operator keeps the library that was active when it was built
        par = ViewCover(mesh, cfg, scene.range_gt, scene.voxel_size, k, stride=stride, chunk=args.chunk, window=args.window)
        _lib.activate()
        assert torch.equal(par(poses, upd.gt_bits, scanned0), vc(poses, upd.gt_bits, scanned0))
        ab(out, "fused", [fused_call] + [lambda: par(poses, upd.gt_bits, scanned0)] * 2, args.iters, args.repeats)
    out["mean_cover"] = vc(poses, upd.gt_bits, scanned0).float().mean(dim=(0, 1)).tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--cases", default="g64_s1,g64_s4,dense_s1,g128_s1")
    ap.add_argument("--chunk", type=int, default=0, help="candidates per workgroup (0 = chosen)")
    ap.add_argument("--window", type=int, default=0, help="bit-set words per workgroup (0 = chosen)")
    ap.add_argument("--parent-lib", default=None, help="another build of libgennbv_hip.so (the same ABI) to set the ViewCover call against")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_view_cover needs a GPU")
    results = []
    for c in args.cases.split(","):
        if c in ("g64_s1", "g64_s4", "g128_s1"):
            n, g, stride = (128, 128, 1) if c == "g128_s1" else (256, 64, 4 if c == "g64_s4" else 1)
            scene = S.make_scenes(n, g, seed=1)
            r = cover_case(c, MeshScene.from_boxes(scene, device=DEV), scene, n, g, 240, 320, stride, 32, args, composed=stride == 1)
        elif c == "dense_s1":
            n, g = 64, 64
            mesh = dense_mesh(n)
            scene = mesh.ground_truth(g, torch.tensor([[6.5, -6.5, 6.5, -6.5, 9.0, 0.0]] * n))
            r = cover_case(c, mesh, scene, n, g, 240, 320, 1, 32, args)
        else:
            raise SystemExit("unknown case " + c)
        print(json.dumps(r), flush=True)
        results.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

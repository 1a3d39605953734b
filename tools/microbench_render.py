"""Microbenchmark of the closed-loop renderer (gnbv_render_depth) and of the closed-loop env step.

    python tools/microbench_render.py [--repeats 7] [--iters 20] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call,
Mrays/s at the median, and the share of the output-store floor (12 B per pixel with rgba: depth, seg, rgba at 8 TB/s
HBM peak) the median reaches.  Cases:

  boxes_240x320    256 envs x 240x320, make_scenes box scenes (<= 96 triangles per env)
  boxes_400x400    256 envs x 400x400, 20^3 scenes (the reference default camera)
  dense_240x320    256 envs x 240x320, two UV spheres + boxes per env (~20 k triangles: the cell grid at work)
  env_step         closed-loop vs open-loop ReplayFeedEnv.step at 256 x 240x320 x 64^3, alternated in one process

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/microbench_render.py` run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.config import TaskConfig, baseline_config  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene, sphere_triangles  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E spec


def time_calls(fn, iters, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def summary(us, n, h, w):
    med = float(np.median(us))
    rays = n * h * w
    return {"us_median": med, "us_min": float(min(us)), "us_max": float(max(us)), "spread_pct": 100.0 * (max(us) - min(us)) / med,
            "mrays_per_s": rays / med, "store_floor_frac": (12.0 * rays / HBM_PEAK * 1e6) / med}


def dense_mesh(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    sc = S.make_scenes(n, 16, seed=seed, max_boxes=4)
    boxes = MeshScene.from_boxes(sc)
    tris, ids = [], []
    base_sphere = sphere_triangles((0.0, 0.0, 0.0), 1.0, 70, 72)  # 9 936 triangles
    for e in range(n):
        t, i = boxes.env_triangles(e)
        parts, pid = [t], [i]
        for k in range(2):
            c = torch.cat([(torch.rand(2, generator=g) - 0.5) * 8.0, 2.0 + torch.rand(1, generator=g) * 3.0])
            parts.append(base_sphere * (1.0 + 1.5 * float(torch.rand(1, generator=g))) + c)
            pid.append(torch.full((base_sphere.shape[0],), 10 + k, dtype=torch.int32))
        tris.append(torch.cat(parts))
        ids.append(torch.cat(pid))
    return MeshScene.from_triangles(tris, ids, device=DEV)


def render_case(name, mesh, cfg, args):
    n = mesh.num_envs
    feed = RenderFeed(mesh, cfg)
    poses = S.poses_from_actions(S.sample_actions(n, cfg, torch.Generator().manual_seed(3)), cfg).float().to(DEV)
    us = time_calls(lambda: feed.render(poses), args.iters, args.repeats)
    r = summary(us, n, cfg.camera_height, cfg.camera_width)
    r.update(case=name, envs=n, h=cfg.camera_height, w=cfg.camera_width, triangles_per_env=mesh.num_triangles / n,
             obj_frac=float((feed.seg_raw > 0).float().mean()))
    return r


def env_step_case(args):
    from gennbv_amd.env.replay_feed import ReplayFeed, ReplayFeedEnv
    n = 256
    cfg = baseline_config(1)  # 240x320, 64^3
    scene = S.make_scenes(n, cfg.grid_size, seed=1)
    open_env = ReplayFeedEnv(cfg, scene, ReplayFeed.synthetic(scene, cfg, 4, seed=1), DEV)
    open_env.feed = ReplayFeed(*[None if x is None else x.to(DEV) for x in (open_env.feed.depth_raw, open_env.feed.seg_raw,
                                                                            open_env.feed.rgba, open_env.feed.c2w)])
    closed_env = ReplayFeedEnv(cfg, scene, RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg), DEV)
    gen = torch.Generator().manual_seed(5)
    acts = [S.sample_actions(n, cfg, gen).to(DEV) for _ in range(8)]
    res = {"open": [], "closed": []}
    for env in (open_env, closed_env):
        env.reset()
    k = [0]

    def step(env):
        env.step(acts[k[0] % len(acts)])
        k[0] += 1
    for _ in range(args.repeats):  # alternate the two envs, one timed block each per round
        for name, env in (("open", open_env), ("closed", closed_env)):
            res[name] += time_calls(lambda: step(env), args.iters, 1, warmup=2)
    out = {"case": "env_step", "envs": n, "h": cfg.camera_height, "w": cfg.camera_width, "grid": cfg.grid_size}
    for name, us in res.items():
        med = float(np.median(us))
        out[name] = {"us_median": med, "us_min": float(min(us)), "us_max": float(max(us)),
                     "spread_pct": 100.0 * (max(us) - min(us)) / med}
    out["closed_minus_open_us"] = out["closed"]["us_median"] - out["open"]["us_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="boxes_240x320,boxes_400x400,dense_240x320,env_step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_render needs a GPU")
    cases = args.cases.split(",")
    results = []
    for c in cases:
        if c == "boxes_240x320":
            cfg = baseline_config(1)
            r = render_case(c, MeshScene.from_boxes(S.make_scenes(256, 16, seed=1), device=DEV), cfg, args)
        elif c == "boxes_400x400":
            cfg = TaskConfig()
            r = render_case(c, MeshScene.from_boxes(S.make_scenes(256, 20, seed=1), device=DEV), cfg, args)
        elif c == "dense_240x320":
            r = render_case(c, dense_mesh(256), baseline_config(1), args)
        elif c == "env_step":
            r = env_step_case(args)
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

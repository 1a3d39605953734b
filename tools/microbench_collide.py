"""Microbenchmark of collision termination (gnbv_collide_cylinder) and of the closed-loop env step with and without it.

    python tools/microbench_collide.py [--repeats 7] [--iters 20] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call.
Cases:

  boxes      256 envs, make_scenes box scenes at BASELINE configs[1] geometry (64^3 grid; <= 96 triangles per env),
             cf2x body at random lattice poses
  dense      256 envs, two UV spheres + boxes per env (~20 k triangles: the cell grid at work), the same poses
  batch_k32  the box scenes, 256 x 32 random lattice poses: one collide_candidates call (gnbv_collide_cylinder_batch) against
             the 32 collide calls it replaces, alternated in one process
  env_step   closed-loop ReplayFeedEnv.step at 256 x 240x320 x 64^3, without and with a CollisionBody, alternated in one process

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/microbench_collide.py` run.
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
from gennbv_amd.env.collision import CollisionBody  # noqa: E402
from gennbv_amd.env.config import baseline_config  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from tools.microbench_render import dense_mesh, time_calls  # noqa: E402

DEV = "cuda:0"


def stats(us):
    med = float(np.median(us))
    return {"us_median": med, "us_min": float(min(us)), "us_max": float(max(us)), "spread_pct": 100.0 * (max(us) - min(us)) / med}


def collide_case(name, mesh, cfg, args):
    n = mesh.num_envs
    poses = S.poses_from_actions(S.sample_actions(n, cfg, torch.Generator().manual_seed(3)), cfg).float().to(DEV).contiguous()
    body = CollisionBody()
    out = torch.empty(n, dtype=torch.uint8, device=DEV)
    r = stats(time_calls(lambda: mesh.collide(poses, body, out=out), args.iters, args.repeats))
    code = out.cpu().numpy()
    r.update(case=name, envs=n, triangles_per_env=mesh.num_triangles / n, contact_frac=float((code != 0).mean()))
    return r


def batch_case(args, k=32):
    from gennbv_amd.eval.baselines import LatticeCandidates
    cfg = baseline_config(1)
    n = 256
    mesh = MeshScene.from_boxes(S.make_scenes(n, cfg.grid_size, seed=1), device=DEV)
    lc = LatticeCandidates(cfg, k, seed=3)
    poses = lc.poses(lc.sample(n)).to(DEV)
    body = CollisionBody()
    out_b = torch.empty(n, k, dtype=torch.uint8, device=DEV)
    out_c = torch.empty(k, n, dtype=torch.uint8, device=DEV)

    def columns():
        for j in range(k):
            mesh.collide(poses[:, j], body, out=out_c[j])
    res = {"batched": [], "columns": []}
    for _ in range(args.repeats):
        res["batched"] += time_calls(lambda: mesh.collide_candidates(poses, body, out=out_b), args.iters, 1, warmup=2)
        res["columns"] += time_calls(columns, args.iters, 1, warmup=2)
    r = {"case": "batch_k32", "envs": n, "k": k, "equal": bool(torch.equal(out_b, out_c.t())),
         "contact_frac": float((out_b != 0).float().mean())}
    for name, us in res.items():
        r[name] = stats(us)
    r["columns_over_batched"] = r["columns"]["us_median"] / r["batched"]["us_median"]
    return r


def env_step_case(args):
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    n = 256
    cfg = baseline_config(1)  # 240x320, 64^3
    scene = S.make_scenes(n, cfg.grid_size, seed=1)
    envs = {"closed": ReplayFeedEnv(cfg, scene, RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg), DEV),
            "closed_collide": ReplayFeedEnv(cfg, scene, RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg), DEV,
                                            collision=CollisionBody())}
    gen = torch.Generator().manual_seed(5)
    acts = [S.sample_actions(n, cfg, gen).to(DEV) for _ in range(8)]
    res = {k: [] for k in envs}
    for env in envs.values():
        env.reset()
    k = [0]

    def step(env):
        env.step(acts[k[0] % len(acts)])
        k[0] += 1
    for _ in range(args.repeats):  # alternate the two envs, one timed block each per round
        for name, env in envs.items():
            res[name] += time_calls(lambda: step(env), args.iters, 1, warmup=2)
    out = {"case": "env_step", "envs": n, "h": cfg.camera_height, "w": cfg.camera_width, "grid": cfg.grid_size}
    for name, us in res.items():
        out[name] = stats(us)
    out["collide_minus_plain_us"] = out["closed_collide"]["us_median"] - out["closed"]["us_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="boxes,dense,batch_k32,env_step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_collide needs a GPU")
    results = []
    for c in args.cases.split(","):
        cfg = baseline_config(1)
        if c == "boxes":
            r = collide_case(c, MeshScene.from_boxes(S.make_scenes(256, cfg.grid_size, seed=1), device=DEV), cfg, args)
        elif c == "dense":
            r = collide_case(c, dense_mesh(256), cfg, args)
        elif c == "batch_k32":
            r = batch_case(args)
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

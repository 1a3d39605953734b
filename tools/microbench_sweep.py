"""Microbenchmark of the swept flight path (gnbv_sweep_sphere, MeshScene.sweep_candidates) beside the pose test
(gnbv_collide_cylinder_batch, MeshScene.collide_candidates) at the same N x K, in the same process.

    python tools/microbench_sweep.py [--repeats 7] [--iters 20] [--envs 256] [--k 32] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times, the two kernels alternated; reported:
median / min / max us per launch and sweep / collide.  Cases (N envs x K random lattice candidates each):

  boxes_init    make_scenes box scenes (<= 96 triangles per env), every flight from the init pose (one start per env, broadcast)
  boxes_random  the same scenes, every flight from its own random lattice pose
  dense_init    two UV spheres + boxes per env (~20 k triangles: the cell grid at work), from the init pose
  dense_random  the same mesh, from random lattice poses

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/microbench_sweep.py` run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.collision import CollisionBody  # noqa: E402
from gennbv_amd.env.config import baseline_config  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from tools.microbench_collide import stats  # noqa: E402
from tools.microbench_render import dense_mesh, time_calls  # noqa: E402

DEV = "cuda:0"


def sweep_case(name, mesh, cfg, random_starts, args):
    from gennbv_amd.eval.baselines import LatticeCandidates
    n, k = mesh.num_envs, args.k
    lc = LatticeCandidates(cfg, k, seed=3)
    to = lc.poses(lc.sample(n)).to(DEV).contiguous()
    if random_starts:
        ls = LatticeCandidates(cfg, k, seed=4)
        start = ls.poses(ls.sample(n)).to(DEV).contiguous()
    else:
        start = torch.tensor(cfg.init_pose_buf, dtype=torch.float32, device=DEV).repeat(n, 1)
    body = CollisionBody(sweep=True)
    out_s = torch.empty(n, k, dtype=torch.uint8, device=DEV)
    out_c = torch.empty(n, k, dtype=torch.uint8, device=DEV)
    res = {"sweep": [], "collide": []}
    for _ in range(args.repeats):
        res["sweep"] += time_calls(lambda: mesh.sweep_candidates(start, to, body, out=out_s), args.iters, 1, warmup=2)
        res["collide"] += time_calls(lambda: mesh.collide_candidates(to, body, out=out_c), args.iters, 1, warmup=2)
    length = (to[..., :3] - (start if random_starts else start[:, None])[..., :3]).norm(dim=-1)
    r = {"case": name, "envs": n, "k": k, "triangles_per_env": mesh.num_triangles / n, "cells_per_axis_max": int(mesh.cell_res.max()),
         "mean_flight_m": float(length.mean()), "blocked_frac": float((out_s != 0).float().mean()),
         "contact_frac": float((out_c != 0).float().mean())}
    for key, us in res.items():
        r[key] = stats(us)
    r["sweep_over_collide"] = r["sweep"]["us_median"] / r["collide"]["us_median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--cases", default="boxes_init,boxes_random,dense_init,dense_random")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_sweep needs a GPU")
    cfg = baseline_config(1)
    meshes = {}
    results = []
    for c in args.cases.split(","):
        kind, _, starts = c.partition("_")
        if kind not in ("boxes", "dense") or starts not in ("init", "random"):
            raise SystemExit("unknown case " + c)
        if kind not in meshes:
            meshes.clear()
            torch.cuda.empty_cache()
            meshes[kind] = (MeshScene.from_boxes(S.make_scenes(args.envs, cfg.grid_size, seed=1), device=DEV) if kind == "boxes"
                            else dense_mesh(args.envs))
        r = sweep_case(c, meshes[kind], cfg, starts == "random", args)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Microbenchmark of the surface voxelizer (gnbv_voxelize_surface, MeshScene.ground_truth's kernel).

    python tools/microbench_voxelize.py [--repeats 7] [--iters 10] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call,
the occupied share of the grid, and the share of the output-store floor (4 B per voxel at 8 TB/s HBM peak) the median
reaches.  Cases:

  boxes_g64      256 envs of make_scenes box scenes (<= 96 triangles per env), G = 64
  boxes_g128     the same at G = 128
  dense_g64      256 envs of two UV spheres + boxes (~20 k triangles per env, microbench_render's dense scene), G = 64
  oracle_cpu     the fp64 test oracle (tests/voxelize_oracle.py) on one box env at G = 64, CPU seconds, for context
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from microbench_render import HBM_PEAK, dense_mesh, time_calls  # noqa: E402

DEV = "cuda:0"


def voxelize_case(name, mesh, g, range_gt, args):
    n = mesh.num_envs
    rng, vox = mesh.grid_spec(g, range_gt)
    rng, vox = rng.to(DEV), vox.to(DEV)
    grid = torch.empty(n, g, g, g, dtype=torch.float32, device=DEV)
    us = time_calls(lambda: mesh.voxelize_into(grid, rng, vox), args.iters, args.repeats)
    med = float(np.median(us))
    return {"case": name, "envs": n, "grid": g, "triangles_per_env": mesh.num_triangles / n,
            "us_median": med, "us_min": float(min(us)), "us_max": float(max(us)), "spread_pct": 100.0 * (max(us) - min(us)) / med,
            "occupied_frac": float(grid.mean()), "store_floor_frac": (4.0 * n * g ** 3 / HBM_PEAK * 1e6) / med}


def oracle_case(args):
    from tests import voxelize_oracle as VO
    g = 64
    sc = S.make_scenes(1, g, seed=1)
    tris = MeshScene.from_boxes(sc).env_triangles(0)[0]
    t = VO.tau(sc.range_gt[0].numpy())
    secs = []
    for _ in range(max(1, min(args.repeats, 3))):
        t0 = time.perf_counter()
        VO.separation(tris, sc.range_gt[0].numpy(), sc.voxel_size[0].numpy(), g, reach=2 * t)
        secs.append(time.perf_counter() - t0)
    return {"case": "oracle_cpu", "envs": 1, "grid": g, "triangles_per_env": int(tris.shape[0]),
            "s_median": float(np.median(secs)), "s_min": float(min(secs)), "s_max": float(max(secs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cases", default="boxes_g64,boxes_g128,dense_g64,oracle_cpu")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_voxelize needs a GPU")
    results = []
    for c in args.cases.split(","):
        if c in ("boxes_g64", "boxes_g128"):
            g = 64 if c == "boxes_g64" else 128
            sc = S.make_scenes(256, 16, seed=1)
            r = voxelize_case(c, MeshScene.from_boxes(sc, device=DEV), g, sc.range_gt, args)
        elif c == "dense_g64":
            r = voxelize_case(c, dense_mesh(256), 64, torch.tensor([[8.0, -8.0, 8.0, -8.0, 10.0, 0.0]] * 256), args)
        elif c == "oracle_cpu":
            r = oracle_case(args)
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

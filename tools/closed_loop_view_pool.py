"""Closed-loop table of DESIGN.md "View pool: cached visibility masks and the greedy set-cover planner".

    python tools/closed_loop_view_pool.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--pools 32,256] [--views 512] [--seeds 1,2] [--out FILE.json]

The set-up of tools/closed_loop_view_cover.py (ReplayFeedEvalEnv over RenderFeed(MeshScene.from_boxes(make_scenes(envs, grid,
seed=1))), 60 x 80 camera, `steps`-step episodes, surface and observable ground truth), extended by PoolCoverPolicy at each
pool size, and per pool: the plan ceiling (the covered share of the ground truth after plan(`steps`) from the post-reset scanned
set) and the pool's observable share (union_bits, with the post-reset scanned set, over the ground truth).
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
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv  # noqa: E402
from gennbv_amd.eval.baselines import (GreedyGainPolicy, LatticeCandidates, OracleGainPolicy, PoolCoverPolicy,  # noqa: E402
                                       RandomLatticePolicy)
from tools.closed_loop_view_cover import run  # noqa: E402

DEV = "cuda:0"


def count(bits):
    """int32 [N, words] -> set bits per row"""
    return np.unpackbits(np.ascontiguousarray(bits.cpu().numpy()).view(np.uint8), axis=1).sum(1).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--pools", default="32,256")
    ap.add_argument("--views", type=int, default=512)
    ap.add_argument("--seeds", default="1,2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_view_pool needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    surface = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(surface, device=DEV)
    lc = LatticeCandidates(cfg, args.views, seed=0, look_at_scene=True)
    init = S.poses_from_actions(torch.tensor(cfg.init_action).view(1, 1, 6).expand(n, 1, 6), cfg).float()
    observable = mesh.observable_ground_truth(g, torch.cat([init, lc.poses(lc.sample(n))], 1), cfg, base=surface)
    pools = [int(p) for p in args.pools.split(",")]
    res = {"envs": n, "grid": g, "steps": args.steps, "k": args.k, "pools": pools, "rows": []}
    for gt_name, scene in (("surface", surface), ("observable", observable)):
        for seed in (int(s) for s in args.seeds.split(",")):
            names = ["random", "greedy", "oracle"] + [f"pool{p}" for p in pools]
            for pname in names:
                env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps)
                row = {"gt": gt_name, "seed": seed, "policy": pname}
                if pname == "random":
                    pol = RandomLatticePolicy(cfg, n, seed)
                elif pname == "greedy":
                    pol = GreedyGainPolicy(env, k=args.k, weights=(1, 4), seed=seed)
                elif pname == "oracle":
                    pol = OracleGainPolicy(env, k=args.k, seed=seed)
                else:
                    pol = PoolCoverPolicy(env, pool_size=int(pname[4:]), seed=seed)
                    env.reset()
                    u = env.updater
                    gt_count = count(u.gt_bits)
                    covered = pol.plan(args.steps)[2]
                    row["plan_ceiling"] = float(np.mean(count(covered & u.gt_bits) / gt_count))
                    row["pool_observable_share"] = float(np.mean(count((pol.pool.union_bits() | u.scanned_bits) & u.gt_bits) / gt_count))
                row.update(run(pol, env))
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Closed-loop table of DESIGN.md "View coverage, observable ground truth and the oracle planner".

    python tools/closed_loop_view_cover.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--views 512] [--seeds 1,2] [--out FILE.json]

ReplayFeedEvalEnv over RenderFeed(MeshScene.from_boxes(make_scenes(envs, grid, seed=1))), 60 x 80 camera, `steps`-step
episodes, K candidates per decision: final coverage (mean over envs of coverage_ratio on each env's done step) and mean_AUC
of the random, greedy and one-step-oracle planners, on the surface ground truth and on the observable ground truth built
from `views` look-at-scene lattice views per env (plus the init pose); and the share of the surface voxels that is observable.
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
from gennbv_amd.eval import evaluate_policy_grid_obs  # noqa: E402
from gennbv_amd.eval.baselines import GreedyGainPolicy, LatticeCandidates, OracleGainPolicy, RandomLatticePolicy  # noqa: E402

DEV = "cuda:0"


def run(policy, env):
    n = env.num_envs
    final = {}

    def cb(loc, _):
        i = loc["i"]
        if bool(loc["done"]) and i not in final:
            final[i] = float(env.coverage_ratio[i])
    _, lens, auc, _ = evaluate_policy_grid_obs(policy, env, n_eval_episodes=n, callback=cb)
    return {"final_coverage": float(np.mean([final[i] for i in range(n)])), "mean_AUC": float(auc.mean()),
            "mean_length": float(np.mean(lens))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--views", type=int, default=512)
    ap.add_argument("--seeds", default="1,2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_view_cover needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    surface = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(surface, device=DEV)
    lc = LatticeCandidates(cfg, args.views, seed=0, look_at_scene=True)
    init = S.poses_from_actions(torch.tensor(cfg.init_action).view(1, 1, 6).expand(n, 1, 6), cfg).float()
    views = torch.cat([init, lc.poses(lc.sample(n))], 1)
    observable = mesh.observable_ground_truth(g, views, cfg, base=surface)
    share = (observable.grid_gt.sum(dim=(1, 2, 3)).cpu() / surface.grid_gt.sum(dim=(1, 2, 3))).tolist()
    res = {"envs": n, "grid": g, "steps": args.steps, "k": args.k, "views": args.views, "observable_share_per_env": share,
           "observable_share_mean": float(np.mean(share)), "rows": []}
    print(json.dumps({"observable_share_mean": res["observable_share_mean"], "per_env": share}), flush=True)
    for gt_name, scene in (("surface", surface), ("observable", observable)):
        for seed in (int(s) for s in args.seeds.split(",")):
            for pname in ("random", "greedy", "oracle"):
                env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps)
                pol = {"random": lambda: RandomLatticePolicy(cfg, n, seed),
                       "greedy": lambda: GreedyGainPolicy(env, k=args.k, weights=(1, 4), seed=seed),
                       "oracle": lambda: OracleGainPolicy(env, k=args.k, seed=seed)}[pname]()
                row = {"gt": gt_name, "seed": seed, "policy": pname}
                row.update(run(pol, env))
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Closed-loop table of DESIGN.md "Frontier of the scanned map": uniform against frontier-aimed candidates.

    python tools/closed_loop_frontier.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--seeds 1,2] [--top 8] [--block 4]
                                         [--radius_m 3.0] [--stride 2] [--out FILE.json]

The set-up of the "View gain" closed-loop table: ReplayFeedEvalEnv over RenderFeed(MeshScene.from_boxes(make_scenes(envs, grid,
seed=1))), 60 x 80 camera, `steps`-step episodes, K candidates per decision, weights (1, 4).  Rows, per seed:

  greedy / uniform            GreedyGainPolicy over LatticeCandidates
  greedy / frontier aim       GreedyGainPolicy(candidates=FrontierCandidates(radius_m=None)): the same positions, aimed at the frontier
  greedy / frontier R m       ... radius_m=R: positions moved to within R of the frontier block's centroid too
  map-greedy / ...            the same three under MapGreedyPolicy on an env with CollisionBody(sweep=True) and
                              BeliefFlightField(unknown="free") over the stride-`stride` flight lattice

Columns: final coverage (mean over envs of coverage_ratio on each env's done step), mean_AUC, mean episode length, and the mean
frontier voxel count of the map the planner saw at each decision of the first `steps` steps (a Frontier op of the tool's own).
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
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.flight import FlightLattice  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv  # noqa: E402
from gennbv_amd.eval import evaluate_policy_grid_obs  # noqa: E402
from gennbv_amd.eval.baselines import FrontierCandidates, GreedyGainPolicy, MapGreedyPolicy  # noqa: E402
from gennbv_amd.ops.flight_field import BeliefFlightField  # noqa: E402
from gennbv_amd.ops.frontier import Frontier  # noqa: E402

DEV = "cuda:0"


class CountingPolicy:
    """The wrapped planner, with the frontier count of every observation it is shown kept on the device."""

    def __init__(self, inner, cfg, frontier):
        self.inner, self.cfg, self.frontier, self.counts = inner, cfg, frontier, []

    def __call__(self, obs, deterministic: bool = True):
        cfg = self.cfg
        self.frontier(obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim])
        self.counts.append(self.frontier.count().float().mean())
        return self.inner(obs, deterministic)

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state


def run(policy, env, steps):
    n = env.num_envs
    final = {}

    def cb(loc, _):
        i = loc["i"]
        if bool(loc["done"]) and i not in final:
            final[i] = float(env.coverage_ratio[i])
    _, lens, auc, _ = evaluate_policy_grid_obs(policy, env, n_eval_episodes=n, callback=cb)
    return {"final_coverage": float(np.mean([final[i] for i in range(n)])), "mean_AUC": float(auc.mean()),
            "mean_length": float(np.mean(lens)), "frontier_count_by_step": [round(float(c), 1) for c in policy.counts[:steps]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--seeds", default="1,2")
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--radius_m", type=float, default=3.0)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_frontier needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = CollisionBody(sweep=True)
    lattice = FlightLattice(cfg, stride=args.stride)
    res = {"envs": n, "grid": g, "steps": args.steps, "k": args.k, "top": args.top, "block": args.block, "radius_m": args.radius_m,
           "stride": args.stride, "rows": []}
    sources = ("uniform", "frontier aim", f"frontier {args.radius_m:g} m")
    for seed in (int(s) for s in args.seeds.split(",")):
        for planner in ("greedy", "map-greedy"):
            for source in sources:
                if planner == "greedy":
                    env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps)
                else:
                    flight = BeliefFlightField(n, lattice, body, scene.range_gt, scene.voxel_size, g, unknown="free", device=DEV)
                    env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps, collision=body,
                                            flight=flight)
                cands = None
                if source != "uniform":
                    cands = FrontierCandidates(cfg, args.k, seed, Frontier(n, g, block=args.block, device=DEV), scene.range_gt,
                                               scene.voxel_size, top=args.top, radius_m=None if source.endswith("aim") else args.radius_m)
                cls = GreedyGainPolicy if planner == "greedy" else MapGreedyPolicy
                pol = CountingPolicy(cls(env, k=args.k, weights=(1, 4), seed=seed, candidates=cands), cfg,
                                     Frontier(n, g, block=args.block, device=DEV))
                row = {"seed": seed, "row": f"{planner} / {source}"}
                row.update(run(pol, env, args.steps))
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

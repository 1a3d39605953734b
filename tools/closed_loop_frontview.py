"""Closed-loop table of DESIGN.md "Frontier viewpoints": the nearest-frontier planner beside the map-greedy rows of the frontier table.

    python tools/closed_loop_frontview.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--seeds 1,2] [--top 8] [--block 4]
                                          [--r_min_m 1.0] [--r_max_m 4.0] [--voxel_value_mm 50] [--stride 2] [--carve] [--carve-stride 2]
                                          [--out FILE.json]

The set-up of tools/closed_loop_frontier.py's map-greedy rows: ReplayFeedEvalEnv over RenderFeed(MeshScene.from_boxes(make_scenes(
envs, grid, seed=1))), 60 x 80 camera, `steps`-step episodes, CollisionBody(sweep=True), BeliefFlightField(unknown="free") over the
stride-`stride` flight lattice.  Rows, per seed:

  map-greedy / uniform          MapGreedyPolicy over LatticeCandidates, K candidates, weights (1, 4)
  map-greedy / frontier aim     MapGreedyPolicy(candidates=FrontierCandidates(radius_m=None))
  frontier view / nearest       FrontierViewPolicy(voxel_value_mm=0), fallback = map-greedy / uniform
  frontier view / value V       FrontierViewPolicy(voxel_value_mm=V), the same fallback

Columns: final coverage (mean over envs of coverage_ratio on each env's done step), mean_AUC, mean episode length, the mean of
env.flight_length on the done step (metres flown in the episode), and the share of decisions that fell back (0 for the map-greedy
rows: they have no fallback).  Small samples: reported, not asserted.
`--carve` gives every row's env a CarvedMap (ops/carve.py; `--carve-stride` is its pixel lattice): field, frontier and view gain
then read the observation's grid plus the free space along every camera ray.
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
from gennbv_amd.eval.baselines import FrontierCandidates, FrontierViewPolicy, MapGreedyPolicy  # noqa: E402
from gennbv_amd.ops.carve import CarvedMap  # noqa: E402
from gennbv_amd.ops.flight_field import BeliefFlightField  # noqa: E402
from gennbv_amd.ops.frontier import Frontier  # noqa: E402

DEV = "cuda:0"


class FallbackShare:
    """The wrapped planner, with the share of envs that fell back at every decision kept on the device."""

    def __init__(self, inner):
        self.inner, self.shares = inner, []

    def __call__(self, obs, deterministic: bool = True):
        out = self.inner(obs, deterministic)
        fell = getattr(self.inner, "fell_back", None)
        self.shares.append(torch.zeros((), device=obs.device) if fell is None else fell.float().mean())
        return out

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state


def run(policy, env):
    n = env.num_envs
    final, flown = {}, {}

    def cb(loc, _):
        i = loc["i"]
        if bool(loc["done"]) and i not in final:
            final[i] = float(env.coverage_ratio[i])
            flown[i] = float(env.flight_length[i])
    _, lens, auc, _ = evaluate_policy_grid_obs(policy, env, n_eval_episodes=n, callback=cb)
    return {"final_coverage": float(np.mean([final[i] for i in range(n)])), "mean_AUC": float(auc.mean()),
            "mean_length": float(np.mean(lens)), "flight_length_m": float(np.mean([flown[i] for i in range(n)])),
            "fallback_share": float(torch.stack(policy.shares).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--seeds", default="1,2")
    ap.add_argument("--top", type=int, default=8)
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--r_min_m", type=float, default=1.0)
    ap.add_argument("--r_max_m", type=float, default=4.0)
    ap.add_argument("--voxel_value_mm", type=int, default=50)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--carve", action="store_true", help="every row flies and plans on a CarvedMap: free space along every camera ray")
    ap.add_argument("--carve-stride", type=int, default=2, help="the CarvedMap's pixel lattice")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_frontview needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = CollisionBody(sweep=True)
    lattice = FlightLattice(cfg, stride=args.stride)
    res = {k: getattr(args, k) for k in ("envs", "grid", "steps", "k", "top", "block", "r_min_m", "r_max_m", "voxel_value_mm", "stride")}
    res["carve"], res["rows"] = bool(args.carve), []
    names = ("map-greedy / uniform", "map-greedy / frontier aim", "frontier view / nearest", f"frontier view / value {args.voxel_value_mm}")
    for seed in (int(s) for s in args.seeds.split(",")):
        for name in names:
            flight = BeliefFlightField(n, lattice, body, scene.range_gt, scene.voxel_size, g, unknown="free", device=DEV)
            carve = CarvedMap(n, cfg, scene.range_gt, scene.voxel_size, stride=args.carve_stride, device=DEV) if args.carve else None
            env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps, collision=body, flight=flight,
                                    carve=carve)
            cands = None
            if name.endswith("aim"):
                cands = FrontierCandidates(cfg, args.k, seed, Frontier(n, g, block=args.block, device=DEV), scene.range_gt,
                                           scene.voxel_size, top=args.top, radius_m=None)
            pol = MapGreedyPolicy(env, k=args.k, weights=(1, 4), seed=seed, candidates=cands)
            if name.startswith("frontier view"):
                pol = FrontierViewPolicy(env, pol, top=args.top, block=args.block, r_min_m=args.r_min_m, r_max_m=args.r_max_m,
                                         voxel_value_mm=0 if name.endswith("nearest") else args.voxel_value_mm)
            row = {"seed": seed, "row": name}
            row.update(run(FallbackShare(pol), env))
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

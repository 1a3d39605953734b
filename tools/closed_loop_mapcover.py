"""Closed-loop table of DESIGN.md "Planning ahead on the map": MapCoverPolicy beside the map-greedy rows.

    python tools/closed_loop_mapcover.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--seeds 1,2] [--stride 2] [--mask hit] [--out FILE.json]

The set-up of tools/closed_loop_frontview.py's map-greedy rows: ReplayFeedEvalEnv over RenderFeed(MeshScene.from_boxes(make_scenes(
envs, grid, seed=1))), 60 x 80 camera, `steps`-step episodes, CollisionBody(sweep=True), BeliefFlightField(unknown="free") over the
stride-`stride` flight lattice, one episode per env.  Rows, per seed:

  map-greedy (1,4)              MapGreedyPolicy over LatticeCandidates, K candidates, weights (1, 4)
  map-greedy (0,1)              the same with weights (0, 1): what map-cover with horizon 1 chooses on the hit mask
  map-cover h1 c1               MapCoverPolicy(horizon=1, commit=1)
  map-cover h3 c1               horizon 3, commit 1: receding horizon
  map-cover h5 c1               horizon 5, commit 1
  map-cover h5 c5               horizon 5, commit 5: plan-then-fly in the plan's gain order
  map-cover h5 c5 route         the same, ordered into a tour on the belief field

Columns: final coverage (mean over envs of coverage_ratio on each env's done step), mean_AUC, mean episode length, the mean of
env.flight_length on the done step (metres flown in the episode), and the mean number of planned views per decision (1 for the
map-greedy rows: they plan one view).  Small samples: reported, not asserted.
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
from gennbv_amd.eval.baselines import MapCoverPolicy, MapGreedyPolicy  # noqa: E402
from gennbv_amd.ops.flight_field import BeliefFlightField  # noqa: E402

DEV = "cuda:0"

ROWS = [("map-greedy (1,4)", dict(weights=(1, 4))), ("map-greedy (0,1)", dict(weights=(0, 1))),
        ("map-cover h1 c1", dict(horizon=1, commit=1)), ("map-cover h3 c1", dict(horizon=3, commit=1)),
        ("map-cover h5 c1", dict(horizon=5, commit=1)), ("map-cover h5 c5", dict(horizon=5, commit=5)),
        ("map-cover h5 c5 route", dict(horizon=5, commit=5, route=True))]


class PlannedViews:
    """The wrapped planner, with the mean number of planned views of every decision kept on the device."""

    def __init__(self, inner):
        self.inner, self.views = inner, []

    def __call__(self, obs, deterministic: bool = True):
        out = self.inner(obs, deterministic)
        v = getattr(self.inner, "last_views", None)
        self.views.append(torch.ones((), device=obs.device) if v is None else v.float().mean())
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
            "planned_views": float(torch.stack(policy.views).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--seeds", default="1,2")
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--mask", default="hit", choices=("hit", "unknown"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_mapcover needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = CollisionBody(sweep=True)
    lattice = FlightLattice(cfg, stride=args.stride)
    res = {k: getattr(args, k) for k in ("envs", "grid", "steps", "k", "stride", "mask")}
    res["rows"] = []
    for seed in (int(s) for s in args.seeds.split(",")):
        for name, kw in ROWS:
            flight = BeliefFlightField(n, lattice, body, scene.range_gt, scene.voxel_size, g, unknown="free", device=DEV)
            env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps, collision=body, flight=flight)
            if name.startswith("map-greedy"):
                pol = MapGreedyPolicy(env, k=args.k, seed=seed, **kw)
            else:
                pol = MapCoverPolicy(env, k=args.k, seed=seed, mask=args.mask, **kw)
            row = {"seed": seed, "row": name}
            row.update(run(PlannedViews(pol), env))
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

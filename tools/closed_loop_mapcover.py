"""Closed-loop table of DESIGN.md "Planning ahead on the map": MapCoverPolicy beside the map-greedy rows.

    python tools/closed_loop_mapcover.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--seeds 1,2] [--stride 2] [--mask hit]
                                         [--weights 1,4] [--field free|costly] [--penalty-m 2.0] [--out FILE.json]

The set-up of tools/closed_loop_frontview.py's map-greedy rows: ReplayFeedEvalEnv over RenderFeed(MeshScene.from_boxes(make_scenes(
envs, grid, seed=1))), 60 x 80 camera, `steps`-step episodes, CollisionBody(sweep=True), BeliefFlightField(unknown="free") over the
stride-`stride` flight lattice (`--field costly`: unknown="costly" with `--penalty-m` metres per unknown node entered, the cautious
pilot), one episode per env.  `--mask` is the mask of the map-cover rows; the mixed rows below plan on both masks under
`--weights` (w_unknown, w_hit) whatever `--mask` says, and `--mask mixed` makes every map-cover row a mixed one.  `--grid` goes up
to 128: the planners take their backends from make_view_gain / make_view_gain_masks, the slab kernels above 64^3.  Rows, per seed:

  map-greedy (1,4)              MapGreedyPolicy over LatticeCandidates, K candidates, weights (1, 4)
  map-greedy (0,1)              the same with weights (0, 1): what map-cover with horizon 1 chooses on the hit mask
  map-cover h1 c1               MapCoverPolicy(horizon=1, commit=1)
  map-cover h3 c1               horizon 3, commit 1: receding horizon
  map-cover h5 c1               horizon 5, commit 1
  map-cover h5 c5               horizon 5, commit 5: plan-then-fly in the plan's gain order
  map-cover h5 c5 route         the same, ordered into a tour on the belief field
  map-mixed h1 c1               MapCoverPolicy(mask="mixed", weights): horizon 1 chooses what map-greedy with these weights chooses
  map-mixed h3 c1, h5 c1, h5 c5, h5 c5 route   the map-cover rows under the mixed score

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
        ("map-cover h5 c5 route", dict(horizon=5, commit=5, route=True)),
        ("map-mixed h1 c1", dict(horizon=1, commit=1, mask="mixed")), ("map-mixed h3 c1", dict(horizon=3, commit=1, mask="mixed")),
        ("map-mixed h5 c1", dict(horizon=5, commit=1, mask="mixed")), ("map-mixed h5 c5", dict(horizon=5, commit=5, mask="mixed")),
        ("map-mixed h5 c5 route", dict(horizon=5, commit=5, route=True, mask="mixed"))]


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
    ap.add_argument("--mask", default="hit", choices=("hit", "unknown", "mixed"))
    ap.add_argument("--weights", default="1,4", help="w_unknown,w_hit of the mixed rows")
    ap.add_argument("--field", default="free", choices=("free", "costly"), help="what unknown space is to the belief flight field")
    ap.add_argument("--penalty-m", type=float, default=2.0, help="--field costly: metres per unknown node entered")
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
    weights = tuple(int(w) for w in args.weights.split(","))
    field_kw = dict(unknown="costly", unknown_penalty_m=args.penalty_m) if args.field == "costly" else dict(unknown="free")
    res = {k: getattr(args, k) for k in ("envs", "grid", "steps", "k", "stride", "mask", "weights", "field", "penalty_m")}
    res["rows"] = []
    for seed in (int(s) for s in args.seeds.split(",")):
        for name, kw in ROWS:
            flight = BeliefFlightField(n, lattice, body, scene.range_gt, scene.voxel_size, g, device=DEV, **field_kw)
            env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps, collision=body, flight=flight)
            if name.startswith("map-greedy"):
                pol = MapGreedyPolicy(env, k=args.k, seed=seed, **kw)
            else:
                kw = dict(kw, mask=kw.get("mask", args.mask))
                if kw["mask"] == "mixed":
                    kw["weights"] = weights
                pol = MapCoverPolicy(env, k=args.k, seed=seed, **kw)
            row = {"seed": seed, "row": name}
            row.update(run(PlannedViews(pol), env))
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

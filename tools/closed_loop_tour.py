"""Closed-loop table of DESIGN.md "Plan-then-fly": coverage and metres flown for the pool planner online, for its offline plan flown
in gain order, and for the same plan flown as a short tour.

    python tools/closed_loop_tour.py [--envs 8] [--grid 20] [--steps 13] [--pool 256] [--seeds 1,2] [--stride 2] [--out FILE.json]

The set-up of tools/closed_loop_flight.py (box scenes, 60 x 80 camera, CollisionBody(sweep=True), `flight=FlightField(...)`, each
env's first episode, at most `steps` steps).  For the same scenes and the same pool (`--pool` views, drawn from the seed):

  pool online      PoolCoverPolicy: every step the pool view that adds the most, from where the drone is
  plan gain order  the greedy set-cover plan of `steps` - 1 views from the empty scanned set (PoolCoverPolicy.plan_route: an episode
                   of `steps` steps is the init pose and `steps` - 1 flights, so the whole plan is flown), its routed views flown
                   in the order the plan chose them
  plan tour        TourPolicy: the same views in the order of gnbv_tour_route

Per row: the columns of closed_loop_flight.py (final coverage, `mean_flown_m` = env.flight_length at the step that ends the
episode, ...) and, for the two plan rows, the planned lengths in metres from the pairwise matrix (`planned_m`) and the mean number
of routed views.
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
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.flight import FlightLattice  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.replay_feed import ReplayFeedEnv  # noqa: E402
from gennbv_amd.eval.baselines import PoolCoverPolicy, TourPolicy  # noqa: E402
from gennbv_amd.ops.flight_field import FlightField  # noqa: E402
from tools.closed_loop_flight import run  # noqa: E402

DEV = "cuda:0"


class GainOrderPolicy:
    """TourPolicy's protocol over RoutePlan.plan_actions: the routed views in the plan's own order."""

    def __init__(self, tour: TourPolicy):
        self.tour = tour

    def __call__(self, obs, deterministic: bool = True):
        t = self.tour
        slot = t.env.episode_length_buf.clamp(min=1, max=t.rounds) - 1
        return t.last_plan.plan_actions[t._rows, slot], None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=13)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--seeds", default="1,2")
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_tour needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = CollisionBody(sweep=True)
    lattice = FlightLattice(cfg, stride=args.stride)
    blocked = mesh.flight_blocked(lattice, body)  # once per scene set
    res = {"envs": n, "grid": g, "steps": args.steps, "pool": args.pool, "stride": args.stride, "rows": []}
    for seed in (int(s) for s in args.seeds.split(",")):
        for pname in ("pool online", "plan gain order", "plan tour"):
            flight = FlightField(mesh, lattice, body, blocked=blocked)
            env = ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps, collision=body, flight=flight)
            pool = PoolCoverPolicy(env, pool_size=args.pool, seed=seed)
            row = {"seed": seed, "policy": pname}
            if pname == "pool online":
                pol = pool
            else:
                tour = TourPolicy(env, pool, args.steps - 1)
                plan = tour.last_plan
                pol = tour if pname == "plan tour" else GainOrderPolicy(tour)
                mm = plan.length_mm if pname == "plan tour" else plan.plan_length_mm
                row.update(planned_m=float(mm.double().mean()) * 1e-3, routed_views=float(plan.views.float().mean()),
                           tour_status_or=int(plan.status.max()))
            row.update(run(pol, env, args.steps))
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

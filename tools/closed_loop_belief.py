"""Closed-loop table of DESIGN.md "Flying on the scanned map": the greedy planner with the privileged flight field beside the
pilot that knows only its own map.

    python tools/closed_loop_belief.py [--envs 16] [--grid 20] [--steps 20] [--k 32] [--seeds 1] [--stride 2] [--penalties 1,5,20] [--carve] [--carve-stride 2]
                                        [--out FILE.json]
                                        [--sensor-sigma a,b,c] [--sensor-drop p] [--sensor-edge r,abs,rel,p] [--sensor-quant q] [--sensor-range lo,hi]

The set-up of tools/closed_loop_flight.py (box scenes, 60 x 80 camera, CollisionBody(sweep=True), episodes of at most `steps`
steps, each env's first episode).  Rows:

  greedy / privileged        GreedyGainPolicy, flight=FlightField(mesh): contacts and routes from the ground-truth mesh
  map-greedy / optimistic    MapGreedyPolicy, flight=BeliefFlightField(unknown="free"): routes through what it has not seen
  map-greedy / conservative  MapGreedyPolicy, flight=BeliefFlightField(unknown="blocked"): routes through seen free space only
  map-greedy / cautious P m  MapGreedyPolicy, flight=BeliefFlightField(unknown="costly", unknown_penalty_m=P), P = 1, 5, 20: unknown
                             space is flyable at P metres per node entered (gnbv_flight_classify_tri, gnbv_flight_field_w)
  ... + shortcut             the belief rows with shortcut=True: straight legs judged on the map (csrc/sweepmap.hip), in the env
                             (straight to the farthest waypoint in the clear) and in the planner (a clear straight leg reaches)

Columns: final coverage, episode length, metres flown (env.flight_length at the step that ends the episode), the share of
flown steps that followed a route of the field (with the shortcut: flew at least one route node), the share flown fully
straight (privileged: the straight flight was free; belief: no route node was flown), the share of episodes ended by a path
collision and by a pose collision, for the belief rows the share of decisions in which every candidate was refused, and for
the shortcut rows the mean number of waypoints a step's straight first leg skipped, and for the cautious rows the mean
env.route_unknown per flown step (costly nodes entered).  Reported, not asserted.

`--carve` gives the belief rows' envs a CarvedMap (ops/carve.py; `--carve-stride` is its pixel lattice): the pilot's field and the
planner read the observation's grid plus the free space along every camera ray.  The privileged row does not change.  Two more
columns then: the mean share of free voxels on the map at the episode's end, beside the observation's.  The belief rows also
report, with or without --carve, `mean_routed_nodes`: the lattice nodes the field holds a route to, per decision of a live env
(1: the drone's own node and nothing else), and `path_collisions_on_a_route`: of the episodes ended by a path collision, the
share whose last step flew a route of the field (the others flew the straight fallback of a decision without a reachable
candidate).

Any `--sensor-*` flag puts a DepthSensor (ops/depth_sensor.py) between the renderer and the env of every row: range noise of
sigma = a + b t + c t^2 metres, random dropouts of probability p, dropouts of probability p at depth edges (window radius r, step
above abs + rel t), disparity quantisation t = q / round(q / t), returns outside [lo, hi] metres lost (default 0.1 to 50 m, the
updater's clamp).  Every row's sensor starts from the same seed and frame counters.  Without such a flag there is no sensor and
the output is what it was.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.collision import PATH, PATH_GROUND, CollisionBody  # noqa: E402
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.flight import FlightLattice  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.replay_feed import ReplayFeedEnv  # noqa: E402
from gennbv_amd.eval.baselines import GreedyGainPolicy, MapGreedyPolicy  # noqa: E402
from gennbv_amd.ops.carve import CarvedMap  # noqa: E402
from gennbv_amd.ops.depth_sensor import DepthSensor  # noqa: E402
from gennbv_amd.ops.flight_field import BeliefFlightField, FlightField  # noqa: E402

DEV = "cuda:0"


def run(policy, env, steps):
    n = env.num_envs
    belief = bool(getattr(env.flight, "belief", False))
    obs = env.reset()
    alive = torch.ones(n, dtype=torch.bool, device=DEV)
    final, length, flown, routed, moved, stuck, decisions, straight, skipped, unknown = (torch.zeros(n, device=DEV) for _ in range(10))
    cautious = belief and env.route_unknown is not None
    shortcut = belief and bool(getattr(env.flight, "shortcut", False))
    code = torch.zeros(n, dtype=torch.uint8, device=DEV)
    cfg = env.cfg
    free_map, free_obs, nodes = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    last_routed = torch.zeros(n, dtype=torch.bool, device=DEV)
    for t in range(steps):
        act = policy(obs)[0]
        if belief:
            stuck += (alive & (policy._contact != 0).all(dim=1)).float()
            nodes += torch.where(alive, (env.flight.field != -1).sum(dim=1), torch.zeros_like(alive, dtype=torch.int64)).float()
        decisions += alive.float()
        obs, _, done, _ = env.step(act)
        moved += alive.float()  # reset() set the first pose: every step of an env's first episode is flown
        if belief:
            routed += (alive & env.routed).float()
            straight += (alive & ~env.routed).float()
        else:  # the privileged env flies straight where it can and the field's detour where it must
            routed += (alive & (env.path_code != 0) & ((env.collision_buf & (PATH | PATH_GROUND)) == 0)).float()
            straight += (alive & (env.path_code == 0)).float()
        if shortcut:
            skipped += torch.where(alive, env.skipped, torch.zeros_like(env.skipped)).float()
        if cautious:
            unknown += torch.where(alive, env.route_unknown, torch.zeros_like(env.route_unknown)).float()
        flown = torch.where(alive, env.flight_length, flown)
        ends = alive & done
        if env.map_tri is not None:  # (a done env's row shows the finished episode's grid until its next step)
            free_map = torch.where(ends, (env.map_tri < 0).float().mean(dim=1), free_map)
            free_obs = torch.where(ends, (obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim] < 0).float().mean(dim=1), free_obs)
        if belief:
            last_routed = torch.where(ends, env.routed, last_routed)
        final = torch.where(ends, env.coverage_ratio, final)
        length = torch.where(ends, torch.full_like(length, t + 1), length)
        code = torch.where(ends, env.collision_buf, code)
        alive &= ~done
        if not bool(alive.any()):
            break
    assert not bool(alive.any()), "max_episode_length must end every episode"
    env.flight.check()
    pose_hit = (code & 7) != 0
    path_hit = (code & (PATH | PATH_GROUND)) != 0
    out = {"final_coverage": float(final.mean()), "mean_length": float(length.mean()), "mean_flown_m": float(flown.mean()),
           "routed_share": float(routed.sum() / moved.sum().clamp(min=1.0)),
           "straight_share": float(straight.sum() / moved.sum().clamp(min=1.0)), "ended_by_path_collision": float(path_hit.float().mean()),
           "ended_by_pose_collision": float(pose_hit.float().mean())}
    if belief:
        out["all_candidates_unreachable_share"] = float(stuck.sum() / decisions.sum().clamp(min=1.0))
        out["route_overflows"] = int(env.route_overflow)
        out["mean_routed_nodes"] = float(nodes.sum() / decisions.sum().clamp(min=1.0))
        out["path_collisions_on_a_route"] = float((path_hit & last_routed).float().sum() / path_hit.float().sum().clamp(min=1.0))
    if env.map_tri is not None:
        out["free_share_map"], out["free_share_observation"] = float(free_map.mean()), float(free_obs.mean())
    if shortcut:
        out["mean_skipped"] = float(skipped.sum() / moved.sum().clamp(min=1.0))
    if cautious:
        out["mean_route_unknown"] = float(unknown.sum() / moved.sum().clamp(min=1.0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--seeds", default="1")
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--penalties", default="1,5,20", help="the cautious rows' unknown_penalty_m, metres per unknown node entered")
    ap.add_argument("--carve", action="store_true", help="the belief rows fly and plan on a CarvedMap: free space along every camera ray")
    ap.add_argument("--carve-stride", type=int, default=2, help="the CarvedMap's pixel lattice")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sensor-sigma", default=None, help="a,b,c: range noise of a + b t + c t^2 metres")
    ap.add_argument("--sensor-drop", type=float, default=None, help="probability of a random dropout")
    ap.add_argument("--sensor-edge", default=None, help="r,abs,rel,p: pixels with a step above abs + rel t within radius r drop with probability p")
    ap.add_argument("--sensor-quant", type=float, default=None, help="disparity quantisation: t = q / round(q / t)")
    ap.add_argument("--sensor-range", default=None, help="lo,hi: returns outside it are lost")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_belief needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = CollisionBody(sweep=True)
    lattice = FlightLattice(cfg, stride=args.stride)
    blocked = mesh.flight_blocked(lattice, body)  # once per scene set
    res = {"envs": n, "grid": g, "steps": args.steps, "k": args.k, "stride": args.stride, "carve": bool(args.carve),
           "carve_stride": args.carve_stride if args.carve else None, "rows": []}
    sensor_kw = None
    if any(v is not None for v in (args.sensor_sigma, args.sensor_drop, args.sensor_edge, args.sensor_quant, args.sensor_range)):
        lo, hi = (float(x) for x in (args.sensor_range or "0.1,50").split(","))
        r, e_abs, e_rel, e_p = (float(x) for x in (args.sensor_edge or "0,0,0,0").split(","))
        sensor_kw = dict(min_range_m=lo, max_range_m=hi, edge_radius=int(r), edge_abs_m=e_abs, edge_rel=e_rel, edge_drop=e_p,
                         drop=args.sensor_drop or 0.0, sigma=tuple(float(x) for x in (args.sensor_sigma or "0,0,0").split(",")),
                         quant=args.sensor_quant or 0.0)
        res["sensor"] = dict(sensor_kw)
    for seed in (int(s) for s in args.seeds.split(",")):
        names = ["greedy / privileged", "map-greedy / optimistic", "map-greedy / conservative"]
        names += [f"map-greedy / cautious {p} m" for p in args.penalties.split(",")]
        for name in names + [f"{b} + shortcut" for b in names[1:]]:
            if name.startswith("greedy"):
                flight = FlightField(mesh, lattice, body, blocked=blocked)
            else:
                kind = name.split(" / ")[1].split(" ")[0]
                kw = dict(unknown="costly", unknown_penalty_m=float(name.split(" ")[3])) if kind == "cautious" else \
                    dict(unknown="free" if kind == "optimistic" else "blocked")
                flight = BeliefFlightField(n, lattice, body, scene.range_gt, scene.voxel_size, g, device=DEV,
                                           shortcut=name.endswith("shortcut"), **kw)
            carve = None
            if args.carve and not name.startswith("greedy"):
                carve = CarvedMap(n, cfg, scene.range_gt, scene.voxel_size, stride=args.carve_stride, device=DEV)
            sensor = DepthSensor(n, cfg.camera_height, cfg.camera_width, seed=seed, device=DEV, **sensor_kw) if sensor_kw else None
            env = ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg, sensor=sensor), DEV, max_episode_length=args.steps, collision=body, flight=flight,
                                carve=carve)
            pol = (GreedyGainPolicy if name.startswith("greedy") else MapGreedyPolicy)(env, k=args.k, weights=(1, 4), seed=seed)
            row = {"seed": seed, "row": name}
            row.update(run(pol, env, args.steps))
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

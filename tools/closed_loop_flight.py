"""Closed-loop table of DESIGN.md "Collision-free flight": the table of tools/closed_loop_sweep.py with rows "sweep + flight"
and the length really flown.

    python tools/closed_loop_flight.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--pool 256] [--seeds 1,2] [--stride 2] [--out FILE.json]

The set-up of tools/closed_loop_sweep.py (box scenes, 60 x 80 camera, episodes of at most `steps` steps, each env's first
episode) with CollisionBody(sweep=True) on the env, once without and once with `flight=FlightField(...)`, for the random, greedy,
oracle and pool planners.  Per row: the columns of closed_loop_sweep.py -- `mean_path_m` is its sum of straight jumps between
consecutive poses -- and, with flight, `mean_flown_m` = env.flight_length at the step that ends the episode (detours counted at
their route length) and `detour_steps` = the mean number of steps per episode flown round an obstacle.
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
from gennbv_amd.eval.baselines import GreedyGainPolicy, OracleGainPolicy, PoolCoverPolicy, RandomLatticePolicy  # noqa: E402
from gennbv_amd.ops.flight_field import FlightField  # noqa: E402

DEV = "cuda:0"


def run(policy, env, steps):
    """closed_loop_sweep.run plus the flown length and the number of detours (envs with a flight field)."""
    n = env.num_envs
    obs = env.reset()
    alive = torch.ones(n, dtype=torch.bool, device=DEV)
    path, final, length, flown, detours = (torch.zeros(n, device=DEV) for _ in range(5))
    code = torch.zeros(n, dtype=torch.uint8, device=DEV)
    prev = env.poses[:, :3].clone()
    for t in range(steps):
        obs, _, done, _ = env.step(policy(obs)[0])
        cur = env.poses[:, :3].clone()
        path += torch.where(alive, (cur - prev).norm(dim=1), torch.zeros_like(path))
        if env.flight is not None:
            # a detour: the straight flight was blocked (the env's own path code) and the step did not end on it
            took = alive & (env.path_code != 0) & ((env.collision_buf & (PATH | PATH_GROUND)) == 0)
            detours += took.float()
            flown = torch.where(alive, env.flight_length, flown)
        ends = alive & done
        final = torch.where(ends, env.coverage_ratio, final)
        length = torch.where(ends, torch.full_like(length, t + 1), length)
        code = torch.where(ends, env.collision_buf, code)
        alive &= ~done
        prev = cur
        if not bool(alive.any()):
            break
    assert not bool(alive.any()), "max_episode_length must end every episode"
    pose_hit = (code & 7) != 0
    path_hit = ((code & (PATH | PATH_GROUND)) != 0) & ~pose_hit
    out = {"final_coverage": float(final.mean()), "mean_length": float(length.mean()), "mean_path_m": float(path.mean()),
           "ended_by_pose_collision": float(pose_hit.float().mean()), "ended_by_blocked_flight": float(path_hit.float().mean())}
    if env.flight is not None:
        env.flight.check()
        out.update(mean_flown_m=float(flown.mean()), detour_steps=float(detours.mean()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--seeds", default="1,2")
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_flight needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = CollisionBody(sweep=True)
    lattice = FlightLattice(cfg, stride=args.stride)
    blocked = mesh.flight_blocked(lattice, body)  # once per scene set
    res = {"envs": n, "grid": g, "steps": args.steps, "k": args.k, "pool": args.pool, "stride": args.stride, "rows": []}
    for seed in (int(s) for s in args.seeds.split(",")):
        for pname in ("random", "greedy", "oracle", "pool"):
            for fly in (False, True):
                flight = FlightField(mesh, lattice, body, blocked=blocked) if fly else None
                env = ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps, collision=body, flight=flight)
                if pname == "random":
                    pol = RandomLatticePolicy(cfg, n, seed)
                elif pname == "greedy":
                    pol = GreedyGainPolicy(env, k=args.k, weights=(1, 4), seed=seed)
                elif pname == "oracle":
                    pol = OracleGainPolicy(env, k=args.k, seed=seed)
                else:
                    pol = PoolCoverPolicy(env, pool_size=args.pool, seed=seed)
                row = {"seed": seed, "policy": pname, "mode": "sweep + flight" if fly else "sweep"}
                row.update(run(pol, env, args.steps))
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

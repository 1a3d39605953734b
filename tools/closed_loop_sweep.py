"""Closed-loop table of DESIGN.md "Swept flight path": the baseline planners with and without CollisionBody(sweep=True).

    python tools/closed_loop_sweep.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--pool 256] [--seeds 1,2] [--out FILE.json]

The set-up of tools/closed_loop_view_pool.py (ReplayFeedEnv over RenderFeed(MeshScene.from_boxes(make_scenes(envs, grid, seed=1))),
60 x 80 camera, episodes of at most `steps` steps, surface ground truth) with a CollisionBody on the env, once with `sweep` off and
once with it on, for the random, greedy, oracle and pool planners.  Per row, over each env's first episode: the final coverage,
the episode length, the summed path length (a torch norm of consecutive `env.poses`, the reset pose included as the start), and
how the episodes ended (a pose collision, a blocked flight alone, neither).  With `sweep` off the planners may jump through
walls and the env lets them; with it on the env ends such an episode and the planners (random aside) avoid such flights.
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
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.replay_feed import ReplayFeedEnv  # noqa: E402
from gennbv_amd.eval.baselines import GreedyGainPolicy, OracleGainPolicy, PoolCoverPolicy, RandomLatticePolicy  # noqa: E402

DEV = "cuda:0"


def run(policy, env, steps):
    """Each env's first episode -> means of the final coverage, the length, the path length, and the shares of the endings."""
    n = env.num_envs
    obs = env.reset()
    alive = torch.ones(n, dtype=torch.bool, device=DEV)
    path, final, length = (torch.zeros(n, device=DEV) for _ in range(3))
    code = torch.zeros(n, dtype=torch.uint8, device=DEV)
    prev = env.poses[:, :3].clone()
    for t in range(steps):
        obs, _, done, _ = env.step(policy(obs)[0])
        cur = env.poses[:, :3].clone()
        path += torch.where(alive, (cur - prev).norm(dim=1), torch.zeros_like(path))
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
    return {"final_coverage": float(final.mean()), "mean_length": float(length.mean()), "mean_path_m": float(path.mean()),
            "ended_by_pose_collision": float(pose_hit.float().mean()), "ended_by_blocked_flight": float(path_hit.float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--seeds", default="1,2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_sweep needs a GPU")
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    res = {"envs": n, "grid": g, "steps": args.steps, "k": args.k, "pool": args.pool, "rows": []}
    for seed in (int(s) for s in args.seeds.split(",")):
        for pname in ("random", "greedy", "oracle", "pool"):
            for sweep in (False, True):
                env = ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps, collision=CollisionBody(sweep=sweep))
                if pname == "random":
                    pol = RandomLatticePolicy(cfg, n, seed)
                elif pname == "greedy":
                    pol = GreedyGainPolicy(env, k=args.k, weights=(1, 4), seed=seed)
                elif pname == "oracle":
                    pol = OracleGainPolicy(env, k=args.k, seed=seed)
                else:
                    pol = PoolCoverPolicy(env, pool_size=args.pool, seed=seed)
                row = {"seed": seed, "policy": pname, "sweep": sweep}
                row.update(run(pol, env, args.steps))
                print(json.dumps(row), flush=True)
                res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

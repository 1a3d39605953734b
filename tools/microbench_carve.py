"""Microbenchmark of CarvedMap.update (ops/carve.py: the merge and one measured-frame view-gain launch with k = 1) beside the
closed-loop env step it follows.

    python tools/microbench_carve.py [--repeats 7] [--iters 20] [--cases ...] [--envs128 64] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call.
Every call carves the same frame into a map restored from a snapshot of a mid-episode map (10 closed-loop steps of random
lattice poses), so that each timed call does the first call's work; the restoring copy (N G^3 bytes) is timed alone and
reported beside it.  Cases (N, G, camera, stride):

  g64_s2      256, 64^3, 240x320, 2     CarvedMap.update, its launch alone (`launch`: the merge left out) and its merge alone
  g64_s4      256, 64^3, 240x320, 4
  g128_s2     --envs128, 128^3, 240x320, 2     the slab kernels, one batch
  env_step    closed-loop ReplayFeedEnv.step at 256 x 240x320 x 64^3 without and with carve=CarvedMap(stride 2), in the same process

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/microbench_carve.py` run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.replay_feed import ReplayFeedEnv  # noqa: E402
from gennbv_amd.ops.carve import CarvedMap, merge_observation  # noqa: E402
from tools.microbench_render import time_calls  # noqa: E402
from tools.microbench_view_gain import stats  # noqa: E402

DEV = "cuda:0"


def carved_env(cfg, n, scene, stride):
    carve = CarvedMap(n, cfg, scene.range_gt, scene.voxel_size, stride=stride, device=DEV) if stride else None
    return ReplayFeedEnv(cfg, scene, RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg), DEV, carve=carve)


def carve_case(name, n, g, h, w, stride, args):
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    env = carved_env(cfg, n, scene, stride)
    obs = env.reset()
    gen = torch.Generator().manual_seed(5)
    for _ in range(10):
        obs = env.step(S.sample_actions(n, cfg, gen).to(DEV))[0]
    cm = env.carve
    before = cm.map_i8.clone()  # the map ten steps in; the eleventh frame is carved into it again and again
    obs = env.step(S.sample_actions(n, cfg, gen).to(DEV))[0]
    tri = obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim].to(torch.int8).contiguous()
    depth, poses = env.feed.depth_raw.clone(), env.poses.clone()
    newly = cm.last_gain[:, 0, 0].float().mean().item()
    pose3 = poses[:, :6].reshape(n, 1, 6).contiguous()

    def update():
        cm.map_i8.copy_(before)
        cm.update(tri, depth, poses)

    def launch():
        cm.map_i8.copy_(before)
        cm.op(cm.map_i8, pose3, depth=depth, carve_out=cm.map_i8)

    def merge():
        cm.map_i8.copy_(before)
        merge_observation(cm.map_i8, tri)
    out = {"case": name, "envs": n, "grid": g, "h": h, "w": w, "stride": stride, "rays": len(range(stride // 2, h, stride)) * len(range(stride // 2, w, stride)), "mean_newly_carved": newly,
           "free_share_observation": float((tri < 0).float().mean()), "free_share_map": float((cm.map_i8 < 0).float().mean())}
    if hasattr(cm.op, "workspace_bytes"):
        out["workspace_bytes"] = cm.op.workspace_bytes
    out["restore_copy"] = stats(time_calls(lambda: cm.map_i8.copy_(before), args.iters, args.repeats))
    out["update"] = stats(time_calls(update, args.iters, args.repeats))
    out["launch"] = stats(time_calls(launch, args.iters, args.repeats))
    out["merge"] = stats(time_calls(merge, args.iters, args.repeats))
    return out


def env_step_case(args, stride, n=256, g=64):
    cfg = TaskConfig(camera_width=320, camera_height=240, grid_size=g)
    env = carved_env(cfg, n, S.make_scenes(n, g, seed=1), stride)
    env.reset()
    gen = torch.Generator().manual_seed(5)
    acts = [S.sample_actions(n, cfg, gen).to(DEV) for _ in range(8)]
    k = [0]

    def step():
        env.step(acts[k[0] % len(acts)])
        k[0] += 1
    out = {"case": "env_step", "envs": n, "h": 240, "w": 320, "grid": g, "carve_stride": stride}
    out.update(stats(time_calls(step, args.iters, args.repeats)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default="g64_s2,g64_s4,g128_s2,env_step")
    ap.add_argument("--envs128", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_carve needs a GPU")
    table = {"g64_s2": (256, 64, 240, 320, 2), "g64_s4": (256, 64, 240, 320, 4), "g128_s2": (args.envs128, 128, 240, 320, 2)}
    results = []
    for c in args.cases.split(","):
        if c in table:
            rows = [carve_case(c, *table[c], args)]
        elif c == "env_step":
            rows = [env_step_case(args, 0), env_step_case(args, 2)]
        else:
            raise SystemExit("unknown case " + c)
        for r in rows:
            print(json.dumps(r), flush=True)
            results.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

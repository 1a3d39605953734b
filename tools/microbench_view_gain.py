"""Microbenchmark of the view gain (gnbv_view_gain, gnbv_view_gain_slab) beside the closed-loop env step it precedes.

    python tools/microbench_view_gain.py [--repeats 7] [--iters 5] [--cases ...] [--slabs 0,8] [--chunk 0] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call.
Cases (N, G, camera, stride, K):

  g64_k32     256, 64^3, 240x320, 4, 32     on all-unknown grids and on mid-episode grids (10 closed-loop steps of random
  g64_k128    256, 64^3, 240x320, 4, 128    lattice poses), with the ablations: walk without marking, marking without the
  g20_k32     256, 20^3, 400x400, 4, 32     second mask
  g128_k32    512, 128^3, 240x320, 4, 32    (BASELINE configs[4]'s shard; the slab path, once per slab height of --slabs,
                                            with its workspace bytes)
  env_step    closed-loop ReplayFeedEnv.step at 256 x 240x320 x 64^3 in the same process: the yardstick
  env_step128 the same at 512 x 240x320 x 128^3 (--envs128 to change the 512 of both 128^3 cases)
  torch       what the existing API offers for one small case (per candidate: utils.bresenham3D_pycuda on the lattice targets
              + torch set operations), timed once and checked equal to the kernel

Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/microbench_view_gain.py` run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gennbv_amd import utils as U  # noqa: E402
from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.eval.baselines import LatticeCandidates  # noqa: E402
from gennbv_amd.ops.view_gain import ViewGain, make_view_gain  # noqa: E402
from tools.microbench_render import time_calls  # noqa: E402

DEV = "cuda:0"


def stats(us):
    med = float(np.median(us))
    return {"us_median": med, "us_min": float(min(us)), "us_max": float(max(us))}


def closed_env(cfg, n, scene):
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    return ReplayFeedEnv(cfg, scene, RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg), DEV)


def mid_episode_grid(cfg, n, scene, steps=10):
    env = closed_env(cfg, n, scene)
    obs = env.reset()
    gen = torch.Generator().manual_seed(5)
    for _ in range(steps):
        obs = env.step(S.sample_actions(n, cfg, gen).to(DEV))[0]
    tri = obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim].to(torch.int8).contiguous()
    del env, obs
    torch.cuda.empty_cache()
    return tri


def gain_case(name, n, g, h, w, stride, k, args, slab=0):
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    lc = LatticeCandidates(cfg, k, seed=3)
    poses = lc.poses(lc.sample(n)).to(DEV)
    grids = {"all_unknown": torch.zeros(n, g ** 3, dtype=torch.int8, device=DEV), "mid_episode": mid_episode_grid(cfg, n, scene)}
    vg = make_view_gain(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, device=DEV, slab=slab, chunk=args.chunk)
    out = {"case": name, "envs": n, "grid": g, "h": h, "w": w, "stride": stride, "k": k, "chunk": args.chunk}
    if hasattr(vg, "workspace_bytes"):
        out.update(slab=slab, workspace_bytes=vg.workspace_bytes)
    for gname, tri in grids.items():
        for aname, ablate in (("full", 0), ("no_second_mask", 2), ("walk_only", 1)):
            vg._args.ablate = ablate
            out[f"{gname}_{aname}"] = stats(time_calls(lambda: vg(tri, poses), args.iters, args.repeats))
        vg._args.ablate = 0
        gain = vg(tri, poses)
        out[gname + "_mean_gain"] = gain.float().mean(dim=(0, 1)).tolist()
    return out


def env_step_case(args, name="env_step", n=256, g=64):
    cfg = TaskConfig(camera_width=320, camera_height=240, grid_size=g)
    env = closed_env(cfg, n, S.make_scenes(n, g, seed=1))
    env.reset()
    gen = torch.Generator().manual_seed(5)
    acts = [S.sample_actions(n, cfg, gen).to(DEV) for _ in range(8)]
    k = [0]

    def step():
        env.step(acts[k[0] % len(acts)])
        k[0] += 1
    out = {"case": name, "envs": n, "h": 240, "w": 320, "grid": g}
    out.update(stats(time_calls(step, args.iters, args.repeats)))
    return out


def torch_case(args):
    """One small case on the existing API; range 2 m keeps the targets inside what bresenham3D_pycuda takes."""
    n, g, h, w, stride, k, range_m = 4, 20, 60, 80, 4, 8, 2.0
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    lc = LatticeCandidates(cfg, k, seed=3)
    poses = lc.poses(lc.sample(n)).to(DEV)
    tri = mid_episode_grid(cfg, n, scene, steps=5)
    vg = ViewGain(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, range_m=range_m, device=DEV, with_c2w=True)
    gain = vg(tri, poses).clone()
    t_kernel = stats(time_calls(lambda: vg(tri, poses), args.iters, args.repeats))
    kinv = S.inverse_intrinsics(h, w, cfg.horizontal_fov).to(DEV)
    us, vs = torch.arange(stride // 2, w, stride, device=DEV), torch.arange(stride // 2, h, stride, device=DEV)
    vv, uu = torch.meshgrid(vs, us, indexing="ij")
    pix = torch.stack([uu, vv, torch.ones_like(uu)], -1).view(-1, 3).float() * range_m
    rng, vox = scene.range_gt.to(DEV), scene.voxel_size.to(DEV)

    def by_torch():
        out = torch.zeros(n, k, 3, dtype=torch.int64)
        for e in range(n):
            vmin = rng[e, [1, 3, 5]] - 0.5 * vox[e]
            cls = tri[e].long()
            for j in range(k):
                m = vg.c2w[e, j]
                pts = (pix @ kinv.T) @ m[:3, :3].T + m[:3, 3]
                tgt = torch.floor((pts - vmin) / vox[e]).long()
                src = torch.floor((m[:3, 3] - vmin) / vox[e]).long()
                traj, lens = U.bresenham3D_raw(src[None], tgt, g)  # bresenham3D_pycuda's kernel, per-ray outputs
                traj = traj.long()
                lens = lens.view(-1).long()
                lin = (traj[..., 0] * g + traj[..., 1]) * g + traj[..., 2]
                steps = torch.arange(lin.shape[1], device=DEV)[None]
                valid = steps < lens[:, None]
                c = cls[lin]
                occ = (c == 1) & valid
                blocked = occ.any(1)
                stop = torch.where(blocked, occ.float().argmax(1), torch.full_like(lens, lin.shape[1]))
                unk = valid & (steps < stop[:, None]) & (c == 0)
                out[e, j, 0] = torch.unique(lin[unk]).numel()
                out[e, j, 1] = torch.unique(lin[unk & blocked[:, None]]).numel()
                out[e, j, 2] = int(blocked.sum())
        return out
    res = {"case": "torch", "envs": n, "grid": g, "h": h, "w": w, "stride": stride, "k": k, "range_m": range_m, "kernel": t_kernel}
    try:
        by_torch()  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = by_torch()
        torch.cuda.synchronize()
        res["torch_us"] = (time.perf_counter() - t0) * 1e6
        # (the torch chain's fp32 matmul is not the canonical chain: a target on a voxel boundary may differ)
        res["equal_to_kernel"] = bool(torch.equal(got, gain.cpu().long()))
        res["max_abs_diff"] = int((got - gain.cpu().long()).abs().max())
        res["ratio"] = res["torch_us"] / t_kernel["us_median"]
    except Exception as ex:  # the existing operator's contract differs: report, do not hide
        res["error"] = repr(ex)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cases", default="g64_k32,g64_k128,g20_k32,g128_k32,env_step,env_step128,torch")
    ap.add_argument("--slabs", default="0", help="slab heights of the g128 case, comma-separated (0 = the default)")
    ap.add_argument("--envs128", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=0, help="candidates per workgroup (0 = chosen)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_view_gain needs a GPU")
    table = {"g64_k32": (256, 64, 240, 320, 4, 32), "g64_k128": (256, 64, 240, 320, 4, 128), "g20_k32": (256, 20, 400, 400, 4, 32)}
    results = []
    table["g128_k32"] = (args.envs128, 128, 240, 320, 4, 32)
    cases = []
    for c in args.cases.split(","):
        cases += [(c, int(s)) for s in args.slabs.split(",")] if c == "g128_k32" else [(c, 0)]
    for c, slab in cases:
        if c in table:
            r = gain_case(c, *table[c], args, slab=slab)
        elif c == "env_step":
            r = env_step_case(args)
        elif c == "env_step128":
            r = env_step_case(args, c, args.envs128, 128)
        elif c == "torch":
            r = torch_case(args)
        else:
            raise SystemExit("unknown case " + c)
        print(json.dumps(r), flush=True)
        results.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Microbenchmark of the straight leg judged on the map (gnbv_sweep_tri, ops/flight_field.py BeliefFlightField.sweep) beside its two
scales, in the same process: the swept sphere over the ground-truth mesh on the same N x K legs (gnbv_sweep_sphere,
MeshScene.sweep_candidates) and the belief free set of the same env step (gnbv_flight_blocked_tri, BeliefFlightField.refresh).
No parent-commit time exists for this kernel.

    python tools/microbench_sweepmap.py [--repeats 5] [--iters 10] [--envs 256] [--k 32] [--stride 2] [--grids 64,128] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times, the launches of one case alternated; reported:
median / min / max us per launch.  Cases: N envs of box scenes ten steps into a closed-loop episode -- the tri-class grid the env
has written by then, as int8 rows and as fp32 rows, and K random lattice candidates per env flown to from env.poses; the
optimistic pilot (unknown = free) and the conservative one (unknown = blocked); map_mode 1 (bits packed into LDS, where the grid
fits) and 2 (the grid read from global memory).
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
from gennbv_amd.eval.baselines import LatticeCandidates  # noqa: E402
from gennbv_amd.ops.flight_field import BeliefFlightField  # noqa: E402
from tools.microbench_view_cover import alternate  # noqa: E402
from tools.microbench_view_gain import stats  # noqa: E402

DEV = "cuda:0"


def mid_episode(cfg, mesh, scene, steps=10):
    """(tri int8 [N, G^3], poses f32 [N, 6]) of a closed-loop env `steps` random steps into its episode."""
    n = scene.range_gt.shape[0]
    env = ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV)
    obs = env.reset()
    gen = torch.Generator().manual_seed(5)
    for _ in range(steps):
        obs = env.step(S.sample_actions(n, cfg, gen).to(DEV))[0]
    tri = obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim].to(torch.int8).contiguous()
    poses = env.poses.clone()
    del env, obs
    torch.cuda.empty_cache()
    return tri, poses


def sweep_case(cfg, scene, mesh, tri_i8, poses, cands, unknown, args):
    n, g, k = scene.range_gt.shape[0], cfg.grid_size, cands.shape[1]
    lat = FlightLattice(cfg, stride=args.stride)
    body = CollisionBody(sweep=True)
    tri_f32 = tri_i8.to(torch.float32)
    ff = BeliefFlightField(n, lat, body, scene.range_gt, scene.voxel_size, g, unknown=unknown, device=DEV, shortcut=True)
    cap = int(ff.lib.gnbv_sweepmap_lds_max_grid())
    outs, fns, names = [], [], []
    for mode in (1, 2):
        if mode == 1 and g > cap:
            continue
        for form, tri in (("i8", tri_i8), ("f32", tri_f32)):
            out = torch.empty(n, k, dtype=torch.uint8, device=DEV)
            outs.append(out)

            def fn(mode=mode, tri=tri, out=out):
                ff.map_mode = mode
                ff.sweep(poses, cands, tri=tri, out=out)
            fns.append(fn)
            names.append(f"sweep_tri_mode{mode}_{form}")
    mesh_out = torch.empty(n, k, dtype=torch.uint8, device=DEV)
    fns.append(lambda: mesh.sweep_candidates(poses, cands, body, out=mesh_out))  # the same legs over the ground-truth mesh
    names.append("sweep_sphere_mesh")
    free_set = BeliefFlightField(n, lat, body, scene.range_gt, scene.voxel_size, g, unknown=unknown, device=DEV)  # map_mode 0, no snapshot
    fns.append(lambda: free_set.refresh(tri_i8))  # the node kernel of the same step
    names.append("flight_blocked_tri_i8")
    us = alternate(fns, args.iters, args.repeats)
    assert all(torch.equal(outs[0], o) for o in outs), "the modes or the grid forms disagree"
    code = outs[0]
    r = {"envs": n, "grid": g, "k": k, "stride": args.stride, "nodes": lat.num_nodes, "unknown": unknown, "radius": ff.sweep_radius,
         "rho": ff.rho, "lds_max_grid": cap, "map_blocked_leg_frac": float((code != 0).float().mean()),
         "mesh_blocked_leg_frac": float((mesh_out != 0).float().mean()),
         "mean_leg_m": float((cands[..., :3] - poses[:, None, :3]).norm(dim=-1).mean())}
    for name, u in zip(names, us):
        r[name] = stats(u)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--grids", default="64,128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_sweepmap needs a GPU")
    results = []
    for g in (int(s) for s in args.grids.split(",")):
        cfg = TaskConfig(camera_width=320, camera_height=240, grid_size=g)
        scene = S.make_scenes(args.envs, g, seed=1)
        mesh = MeshScene.from_boxes(scene, device=DEV)
        tri, poses = mid_episode(cfg, mesh, scene)
        lc = LatticeCandidates(cfg, args.k, seed=3)
        cands = lc.poses(lc.sample(args.envs)).to(DEV).contiguous()
        for unknown in ("free", "blocked"):
            r = sweep_case(cfg, scene, mesh, tri, poses, cands, unknown, args)
            print(json.dumps(r), flush=True)
            results.append(r)
        del tri
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

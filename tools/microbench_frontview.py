"""Microbenchmark of the frontier-viewpoint kernel (gnbv_frontier_viewpoints, ops/frontier_view.py FrontierViewpoints) beside what the
same decision costs as view-gain columns, in the same process.

    python tools/microbench_frontview.py [--repeats 5] [--iters 10] [--cases 256x64,512x128,8x64] [--targets 8] [--radii 2,4,8]
                                         [--check 2] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times, the launches of one case alternated; reported:
median / min / max us per launch.  Cases NxG: N envs of box scenes, the tri-class grid of a closed-loop env ten steps into its
episode (tools/microbench_view_gain.mid_episode_grid, made for at most 64 envs and tiled to N) as int8 rows; the stride-2 flight
lattice of the default task (41 x 41 x 26 nodes); the field of a BeliefFlightField(unknown="free") over that map from the task's
init pose; T targets per env: the centroid voxels of the T fullest frontier blocks (block 4); r_min 0.5 m, max_unknown 4; r_max of
--radii; mode 1 (LDS bit planes) and mode 2 (the grid in place) where both exist.  The outputs of the first `check` envs are
asserted equal to a numpy restatement over ALL nodes (vectorised Bresenham, no window).  Beside them: make_view_gain of K = T
candidate poses on the same grids (240 x 320, stride 4) -- the launch a gain-based planner pays to rate as many candidates.
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
from gennbv_amd.eval.baselines import LatticeCandidates  # noqa: E402
from gennbv_amd.ops.flight_field import BeliefFlightField, field_u32  # noqa: E402
from gennbv_amd.ops.frontier import Frontier  # noqa: E402
from gennbv_amd.ops.frontier_view import FrontierViewpoints, block_target_voxels  # noqa: E402
from gennbv_amd.ops.view_gain import make_view_gain  # noqa: E402
from tools.microbench_view_cover import alternate  # noqa: E402
from tools.microbench_view_gain import mid_episode_grid, stats  # noqa: E402

DEV = "cuda:0"
NO_ROUTE = 0xFFFFFFFF


def numpy_viewpoints(tri, range_gt, voxel_size, lattice, field, targets, r_min, r_max, max_unknown):
    """One env restated in numpy over all M nodes: tri int8 [g,g,g], field uint32 [M], targets [T,3] -> (node [T], cost [T],
    count [T,2]).  The Bresenham of every node's line runs vectorised, one step of all lines per turn."""
    g = tri.shape[0]
    cls = np.sign(tri.reshape(-1).astype(np.int64))
    f32 = np.float32
    r, vs = np.asarray(range_gt, f32), np.asarray(voxel_size, f32)
    vmin = (r[1::2] - f32(0.5) * vs).astype(f32)
    o, v = vmin.astype(np.float64), vs.astype(np.float64)
    pos = lattice.node_positions()
    src = np.clip(np.floor((pos.astype(f32) - vmin[None]) / vs[None]).astype(np.int64), -2 ** 24, 2 ** 24)
    fld = field.astype(np.int64)
    t = targets.shape[0]
    node, cost, count = np.full(t, -1, np.int32), np.full(t, NO_ROUTE, np.uint32), np.zeros((t, 2), np.int32)
    for j in range(t):
        tg = targets[j].astype(np.int64)
        if ((tg < 0) | (tg >= g)).any():
            continue
        q = o + (tg.astype(np.float64) + 0.5) * v
        e = pos - q[None]
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        ids = np.nonzero((d2 >= r_min * r_min) & (d2 <= r_max * r_max))[0]
        p = src[ids].copy()
        d = np.abs(tg[None] - p)
        s = np.where(p < tg[None], 1, -1)
        dm = d.max(1)
        # dominant axis tested x, y, z; the minors in the reference's order
        a = np.where(dm == d[:, 0], 0, np.where(dm == d[:, 1], 1, 2))
        b = np.where(a == 0, 1, 0)
        c = np.where(a == 2, 1, 2)
        rows = np.arange(ids.size)
        da, db, dc = d[rows, a], d[rows, b], d[rows, c]
        p1, p2 = 2 * db - da, 2 * dc - da
        occupied, unknown = np.zeros(ids.size, bool), np.zeros(ids.size, np.int64)
        for i in range(int(dm.max(initial=0))):
            live = i < da  # the voxel in front of step i is not the target: it counts
            inside = ((p >= 0) & (p < g)).all(1) & live
            w = cls[((p[:, 0] * g + p[:, 1]) * g + p[:, 2])[inside]]
            occupied[inside] |= w > 0
            unknown[inside] += w == 0
            up1, up2 = live & (p1 >= 0), live & (p2 >= 0)
            p[rows[up1], b[up1]] += s[rows[up1], b[up1]]
            p1[up1] -= 2 * da[up1]
            p[rows[up2], c[up2]] += s[rows[up2], c[up2]]
            p2[up2] -= 2 * da[up2]
            p[rows[live], a[live]] += s[rows[live], a[live]]
            p1[live] += 2 * db[live]
            p2[live] += 2 * dc[live]
        assert (p == tg[None]).all()
        sees = ~occupied & (unknown <= max_unknown)
        routed = ids[sees & (fld[ids] != NO_ROUTE)]
        count[j] = (int(sees.sum()), routed.size)
        if routed.size:
            best = routed[np.lexsort((routed, fld[routed]))[0]]
            node[j], cost[j] = best, fld[best]
    return node, cost, count


def case(n, g, args):
    cfg = TaskConfig(camera_width=320, camera_height=240, grid_size=g)
    base_n = min(n, 64)
    scene = S.make_scenes(base_n, g, seed=1)
    reps = (n + base_n - 1) // base_n
    tri = mid_episode_grid(cfg, base_n, scene).repeat(reps, 1)[:n].contiguous()
    range_gt, voxel_size = scene.range_gt.repeat(reps, 1)[:n].contiguous(), scene.voxel_size.repeat(reps, 1)[:n].contiguous()
    lattice = FlightLattice(cfg, stride=2)
    flight = BeliefFlightField(n, lattice, CollisionBody(sweep=True), range_gt, voxel_size, g, unknown="free", device=DEV)
    init = S.poses_from_actions(torch.tensor(cfg.init_action, dtype=torch.int64).repeat(n, 1), cfg).float().to(DEV).contiguous()
    flight.refresh(tri).update(init)
    fr = Frontier(n, g, block=4, device=DEV)
    fr(tri)
    idx, cnt = fr.top(args.targets)
    vox = block_target_voxels(fr.blocks, idx).contiguous()
    fits = g <= int(flight.lib.gnbv_frontview_lds_max_grid())
    out = {"envs": n, "grid": g, "nodes": lattice.num_nodes, "dims": list(lattice.dims), "targets": args.targets, "r_min": 0.5,
           "max_unknown": 4, "live_targets_per_env": float((cnt > 0).float().sum(1).mean()),
           "reachable_node_frac": float((flight.field != -1).float().mean())}
    fns, names, ops = [], [], []
    for r_max in args.radius_list:
        for mode in (1, 2) if fits else (2,):
            fv = FrontierViewpoints(n, g, lattice, range_gt, voxel_size, args.targets, 0.5, r_max, max_unknown=4, mode=mode, device=DEV)
            ops.append((r_max, mode, fv))
            fns.append(lambda fv=fv: fv(tri, flight, vox))
            names.append(f"r{r_max:g}_mode{mode}")
    # the same decision as view-gain columns: K = T candidates rated on the same grids
    lc = LatticeCandidates(cfg, args.targets, seed=3)
    poses = lc.poses(lc.sample(n)).to(DEV)
    vg = make_view_gain(n, args.targets, cfg, range_gt, voxel_size, stride=4, device=DEV)
    fns.append(lambda: vg(tri, poses))
    names.append(f"view_gain_k{args.targets}")
    us = alternate(fns, args.iters, args.repeats)
    for name, u in zip(names, us):
        out[name] = stats(u)
    host_tri = tri[:args.check].reshape(-1, g, g, g).cpu().numpy()
    host_field, host_vox = field_u32(flight.field[:args.check]), vox[:args.check].cpu().numpy()
    first = {}
    for r_max, mode, fv in ops:
        got = (fv.node.cpu().numpy(), field_u32(fv.cost_mm), fv.count.cpu().numpy())
        if r_max in first:
            assert all(np.array_equal(a, b) for a, b in zip(got, first[r_max])), "the modes disagree"
            continue
        first[r_max] = got
        for e in range(min(args.check, n)):
            want = numpy_viewpoints(host_tri[e], range_gt[e].numpy(), voxel_size[e].numpy(), lattice, host_field[e], host_vox[e], 0.5,
                                    float(r_max), 4)
            assert all(np.array_equal(a[e], b) for a, b in zip(got, want)), f"the numpy restatement disagrees: r_max {r_max}, env {e}"
        out[f"r{r_max:g}_with_node_frac"] = float((got[0] >= 0).mean())
        out[f"r{r_max:g}_mean_seen"] = float(got[2][..., 0].mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cases", default="256x64,512x128,8x64")
    ap.add_argument("--targets", type=int, default=8)
    ap.add_argument("--radii", default="2,4,8")
    ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.radius_list = [float(r) for r in args.radii.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("microbench_frontview needs a GPU")
    results = []
    for c in args.cases.split(","):
        n, g = (int(v) for v in c.split("x"))
        r = case(n, g, args)
        print(json.dumps(r), flush=True)
        results.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Microbenchmark of the belief free set (gnbv_flight_blocked_tri, ops/flight_field.py BeliefFlightField.refresh) beside the
flight-field launch it precedes in the same env step (gnbv_flight_field over the bits it has just written), in the same process.

    python tools/microbench_flightmap.py [--repeats 5] [--iters 10] [--envs 256] [--strides 2,5] [--grids 64,128] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times, the launches of one case alternated; reported:
median / min / max us per launch.  Cases: N envs of box scenes, the default task's lattice at each stride, the tri-class grid
of a closed-loop env ten steps into its episode (tools/microbench_view_gain.mid_episode_grid) at each grid size, as int8 rows
and as fp32 rows; the optimistic pilot (unknown = free) and the conservative one (unknown = blocked); map_mode 1 (bits packed
into LDS, where the grid fits) and 2 (the grid read from global memory).  `unknown = costly` is the cautious pilot's case: the one gnbv_flight_classify_tri launch
(`classify_*`) beside the two gnbv_flight_blocked_tri launches it replaces (`two_launches_*`: unknown_blocks = 0, then 1, over the same
grid), and gnbv_flight_field_w (`field_w`, penalty 5 m) beside gnbv_flight_field (`field`) over the same blocked bits, all alternated
in one process.
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
from gennbv_amd.ops.flight_field import BeliefFlightField, FlightField  # noqa: E402
from tools.microbench_view_cover import alternate  # noqa: E402
from tools.microbench_view_gain import mid_episode_grid, stats  # noqa: E402

DEV = "cuda:0"


def map_case(cfg, scene, tri_i8, stride, unknown, args):
    n, g = scene.range_gt.shape[0], cfg.grid_size
    lat = FlightLattice(cfg, stride=stride)
    body = CollisionBody(sweep=True)
    tri_f32 = tri_i8.to(torch.float32)
    poses = torch.tensor(cfg.init_pose_buf, dtype=torch.float32, device=DEV).repeat(n, 1)
    cap = None
    fields, fns, names = [], [], []
    for mode in (1, 2):
        ff = BeliefFlightField(n, lat, body, scene.range_gt, scene.voxel_size, g, unknown=unknown, map_mode=0, device=DEV)
        cap = int(ff.lib.gnbv_flightmap_lds_max_grid())
        if mode == 1 and g > cap:
            continue
        ff.map_mode = mode
        fields.append(ff)
        for form, tri in (("i8", tri_i8), ("f32", tri_f32)):
            fns.append(lambda ff=ff, tri=tri: ff.refresh(tri))
            names.append(f"map_mode{mode}_{form}")
    ff = fields[0]
    ff.refresh(tri_i8).update(poses)
    fns.append(lambda: FlightField.update(ff, poses))  # the field launch alone, over the belief bits
    names.append("field")
    us = alternate(fns, args.iters, args.repeats)
    words = [f.blocked_map.clone() for f in fields]
    assert all(torch.equal(words[0], w) for w in words), "the modes disagree"
    pad = lat.words * 32 - lat.num_nodes
    blocked = float(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in ff.blocked_map[0].tolist()) - pad) / lat.num_nodes
    r = {"envs": n, "grid": g, "stride": stride, "nodes": lat.num_nodes, "unknown": unknown, "rho": ff.rho, "lds_max_grid": cap,
         "blocked_node_frac_env0": blocked, "reachable_node_frac_env0": float((ff.field[0] != -1).float().mean())}
    for name, u in zip(names, us):
        r[name] = stats(u)
    return r


def classify_case(cfg, scene, tri_i8, stride, args, penalty_m=5.0):
    """The cautious pilot: classify vs the two blocked_tri launches it replaces, field_w vs field on the same bits."""
    n, g = scene.range_gt.shape[0], cfg.grid_size
    lat = FlightLattice(cfg, stride=stride)
    body = CollisionBody(sweep=True)
    tri_f32 = tri_i8.to(torch.float32)
    poses = torch.tensor(cfg.init_pose_buf, dtype=torch.float32, device=DEV).repeat(n, 1)
    mk = lambda **kw: BeliefFlightField(n, lat, body, scene.range_gt, scene.voxel_size, g, map_mode=0, device=DEV, **kw)  # noqa: E731
    fns, names, cautious = [], [], []
    cap = None
    for mode in (1, 2):
        ff = mk(unknown="costly", unknown_penalty_m=penalty_m)
        free, strict = mk(unknown="free"), mk(unknown="blocked")
        cap = int(ff.lib.gnbv_flightmap_classify_lds_max_grid())
        if mode == 1 and g > cap:  # (between the two limits the pair still has its LDS form: compared like with like, mode 2 only)
            continue
        ff.map_mode = free.map_mode = strict.map_mode = mode
        cautious.append((ff, free, strict))
        for form, tri in (("i8", tri_i8), ("f32", tri_f32)):
            fns.append(lambda ff=ff, tri=tri: ff.refresh(tri))
            names.append(f"classify_mode{mode}_{form}")
            fns.append(lambda free=free, strict=strict, tri=tri: (free.refresh(tri), strict.refresh(tri)))
            names.append(f"two_launches_mode{mode}_{form}")
    ff, free, _ = cautious[0]
    ff.refresh(tri_i8).update(poses)
    free.refresh(tri_i8).update(poses)
    fns.append(lambda: FlightField.update(ff, poses))
    names.append("field_w")
    fns.append(lambda: FlightField.update(free, poses))
    names.append("field")
    us = alternate(fns, args.iters, args.repeats)
    for one, loose, strict in cautious:
        assert torch.equal(one.blocked_map, loose.blocked_map) and torch.equal(one.costly_map, strict.blocked_map & ~loose.blocked_map), \
            "classify disagrees with the two launches"
    pad = lat.words * 32 - lat.num_nodes
    ones = lambda row: sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in row.tolist())  # noqa: E731
    r = {"envs": n, "grid": g, "stride": stride, "nodes": lat.num_nodes, "unknown": "costly", "penalty_m": penalty_m, "rho": ff.rho,
         "classify_lds_max_grid": cap, "blocked_node_frac_env0": float(ones(ff.blocked_map[0]) - pad) / lat.num_nodes,
         "costly_node_frac_env0": float(ones(ff.costly_map[0])) / lat.num_nodes,
         "reachable_node_frac_env0": float((ff.field[0] != -1).float().mean())}
    for name, u in zip(names, us):
        r[name] = stats(u)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--strides", default="2,5")
    ap.add_argument("--grids", default="64,128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_flightmap needs a GPU")
    results = []
    for g in (int(s) for s in args.grids.split(",")):
        cfg = TaskConfig(camera_width=320, camera_height=240, grid_size=g)
        scene = S.make_scenes(args.envs, g, seed=1)
        tri = mid_episode_grid(cfg, args.envs, scene)
        for stride in (int(s) for s in args.strides.split(",")):
            for unknown in ("free", "blocked"):
                r = map_case(cfg, scene, tri, stride, unknown, args)
                print(json.dumps(r), flush=True)
                results.append(r)
            r = classify_case(cfg, scene, tri, stride, args)
            print(json.dumps(r), flush=True)
            results.append(r)
        del tri
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Microbenchmark of plan-then-fly: FlightField.pairwise_mm (P field launches + P queries + the stub arithmetic) and the tour
kernel gnbv_tour_route (ops/tour.py route_tour).

    python tools/microbench_tour.py [--repeats 5] [--iters 10] [--envs 256] [--pair-envs 16] [--pair-points 17] [--points 17,33,65,128]
                                    [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call.

  pairwise   box scenes, the default task's lattice at stride 2 (41 x 41 x 26 nodes), P lattice poses per env, in both field
             modes the lattice admits (1: the field resident in LDS, refused where it does not fit; 2: the field in global memory);
             the default lattice does not fit LDS, so mode 1 is timed at stride 5 (17 x 17 x 11) as well as mode 2
  tour       N envs, P points uniform in a 16 m cube (euclid_mm matrices), every point on the route; the 2-opt loop is data
             dependent, so the time of the construction alone (max_moves = 0) and the length gained over it are reported too
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gennbv_amd import _lib  # noqa: E402
from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.collision import CollisionBody  # noqa: E402
from gennbv_amd.env.config import baseline_config  # noqa: E402
from gennbv_amd.env.flight import FlightLattice  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.ops.flight_field import FlightField  # noqa: E402
from gennbv_amd.ops.tour import euclid_mm, route_tour  # noqa: E402
from tools.microbench_collide import stats  # noqa: E402
from tools.microbench_render import time_calls  # noqa: E402

DEV = "cuda:0"


def pairwise_cases(args):
    from gennbv_amd.eval.baselines import LatticeCandidates
    cfg = baseline_config(1)
    n, p = args.pair_envs, args.pair_points
    mesh = MeshScene.from_boxes(S.make_scenes(n, cfg.grid_size, seed=1), device=DEV)
    body = CollisionBody(sweep=True)
    lc = LatticeCandidates(cfg, p, seed=3)
    points = lc.poses(lc.sample(n)).to(DEV).contiguous()
    cap = int(_lib.load().gnbv_flight_lds_max_nodes())
    out = []
    for stride in (2, 5):
        lat = FlightLattice(cfg, stride=stride)
        blocked = mesh.flight_blocked(lat, body)
        for mode in (1, 2):
            if mode == 1 and lat.num_nodes > cap:
                continue
            ff = FlightField(mesh, lat, body, mode=mode, blocked=blocked)
            r = stats(time_calls(lambda: ff.pairwise_mm(points), args.iters, args.repeats, warmup=2))
            ff.check()
            d = ff.pairwise_mm(points)
            r.update(case="pairwise", envs=n, points=p, stride=stride, nodes=lat.num_nodes, mode=mode,
                     no_route_frac=float((d == -1).float().mean()))
            print(json.dumps(r), flush=True)
            out.append(r)
    return out


def tour_cases(args):
    n = args.envs
    out = []
    gen = torch.Generator().manual_seed(7)
    for p in (int(v) for v in args.points.split(",")):
        pts = (torch.rand(n, p, 3, generator=gen) * 16.0).to(DEV)
        dist = euclid_mm(pts)
        nn = route_tour(dist, max_moves=0).length_mm.clone()  # (the outputs are reused per shape: keep copies)
        res = route_tour(dist)
        length, status = res.length_mm.clone(), int(res.status.max())
        r = stats(time_calls(lambda: route_tour(dist), args.iters, args.repeats, warmup=2))
        zero = stats(time_calls(lambda: route_tour(dist, max_moves=0), args.iters, args.repeats, warmup=2))
        r.update(case="tour", envs=n, points=p, us_median_nearest_neighbour_only=zero["us_median"],
                 length_over_nearest_neighbour=float((length.double() / nn.double()).mean()), status_or=status)
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--pair-envs", type=int, default=16)
    ap.add_argument("--pair-points", type=int, default=17)
    ap.add_argument("--points", default="17,33,65,128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_tour needs a GPU")
    results = pairwise_cases(args) + tour_cases(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Microbenchmark of the flight field (gnbv_flight_field / _query / _path, ops/flight_field.py FlightField) beside the straight-flight
test (gnbv_sweep_sphere, MeshScene.sweep_candidates) at the same N x K, in the same process.

    python tools/microbench_flight.py [--repeats 5] [--iters 10] [--envs 256] [--k 32] [--strides 2,5] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times, the four kernels alternated; reported:
median / min / max us per launch, and field / sweep.  Cases (N envs, the default task's lattice at each stride):

  boxes   make_scenes box scenes (<= 96 triangles per env)
  dense   two UV spheres + boxes per env (~20 k triangles)

The field starts from a random free lattice pose per env; query and sweep take K random lattice candidates per env; the path goes
to the first candidate.  The set-up time of the blocked bits (MeshScene.flight_blocked, once per scene set) is reported too.
At stride 2 the default task has 41 x 41 x 26 nodes (the field in global memory), at stride 5 17 x 17 x 11 (resident in LDS).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.collision import CollisionBody  # noqa: E402
from gennbv_amd.env.config import baseline_config  # noqa: E402
from gennbv_amd.env.flight import FlightLattice  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.ops.flight_field import FlightField  # noqa: E402
from tools.microbench_collide import stats  # noqa: E402
from tools.microbench_render import dense_mesh, time_calls  # noqa: E402

DEV = "cuda:0"


def flight_case(name, mesh, cfg, stride, args):
    from gennbv_amd.eval.baselines import LatticeCandidates
    n, k = mesh.num_envs, args.k
    body = CollisionBody(sweep=True)
    lat = FlightLattice(cfg, stride=stride)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ff = FlightField(mesh, lat, body)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    lc = LatticeCandidates(cfg, k, seed=3)
    to = lc.poses(lc.sample(n)).to(DEV).contiguous()
    # a start whose node is free, where the candidates offer one: the first candidate that has a free pose and node
    ls = LatticeCandidates(cfg, 16, seed=4)
    cand = ls.poses(ls.sample(n)).to(DEV).contiguous()
    start = cand[:, 0].clone()
    for j in range(16):
        ff.update(start)
        dead = ff.cost_mm(start[:, None])[:, 0] == -1
        if not bool(dead.any()):
            break
        start = torch.where(dead[:, None], cand[:, j], start)
    ff.update(start)
    ff.check()
    out_q = torch.empty(n, k, dtype=torch.int32, device=DEV)
    out_s = torch.empty(n, k, dtype=torch.uint8, device=DEV)
    first = to[:, 0].contiguous()
    nodes = torch.empty(n, 4 * sum(lat.dims), dtype=torch.int32, device=DEV)
    count = torch.empty(n, dtype=torch.int32, device=DEV)
    res = {"field": [], "query": [], "path": [], "sweep": []}
    for _ in range(args.repeats):
        res["field"] += time_calls(lambda: ff.update(start), args.iters, 1, warmup=2)
        res["query"] += time_calls(lambda: ff.cost_mm(to, out=out_q), args.iters, 1, warmup=2)
        res["path"] += time_calls(lambda: ff.path_into(first, nodes, count), args.iters, 1, warmup=2)
        res["sweep"] += time_calls(lambda: mesh.sweep_candidates(start, to, body, out=out_s), args.iters, 1, warmup=2)
    blocked_nodes = float(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in ff.blocked[0].tolist()) - (lat.words * 32 - lat.num_nodes)) / lat.num_nodes
    r = {"case": name, "envs": n, "k": k, "stride": stride, "nodes": lat.num_nodes, "dims": list(lat.dims),
         "lds": lat.num_nodes <= int(ff.lib.gnbv_flight_lds_max_nodes()), "triangles_per_env": mesh.num_triangles / n,
         "setup_blocked_bits_s": setup_s, "blocked_node_frac_env0": blocked_nodes,
         "sources_without_a_free_node": int((ff.cost_mm(start[:, None])[:, 0] == -1).sum()),
         "straight_blocked_frac": float((out_s != 0).float().mean()), "unreachable_frac": float((out_q == -1).float().mean()),
         "blocked_but_reachable_frac": float(((out_s != 0) & (out_q != -1)).float().mean())}
    for key, us in res.items():
        r[key] = stats(us)
    r["field_over_sweep"] = r["field"]["us_median"] / r["sweep"]["us_median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--strides", default="2,5")
    ap.add_argument("--cases", default="boxes,dense")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_flight needs a GPU")
    cfg = baseline_config(1)
    results = []
    for kind in args.cases.split(","):
        if kind not in ("boxes", "dense"):
            raise SystemExit("unknown case " + kind)
        torch.cuda.empty_cache()
        mesh = MeshScene.from_boxes(S.make_scenes(args.envs, cfg.grid_size, seed=1), device=DEV) if kind == "boxes" else dense_mesh(args.envs)
        for stride in (int(s) for s in args.strides.split(",")):
            r = flight_case(f"{kind}_stride{stride}", mesh, cfg, stride, args)
            print(json.dumps(r), flush=True)
            results.append(r)
        del mesh
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

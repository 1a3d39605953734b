"""Microbenchmark of the frontier kernel (gnbv_frontier_tri, ops/frontier.py Frontier) beside the same result written as a torch
expression (padded shifts plus scatter_add), in the same process.

    python tools/microbench_frontier.py [--repeats 5] [--iters 10] [--cases 256x64,512x128,8x64] [--block 4] [--slabs 0,4,8,16,32]
                                        [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times, the launches of one case alternated; reported:
median / min / max us per launch, and for the auto slab the share of the byte floor (N G^3 elements read once at 8 TB/s).  Cases
NxG: N envs of box scenes, the tri-class grid of a closed-loop env ten steps into its episode
(tools/microbench_view_gain.mid_episode_grid, made for at most 64 envs and tiled to N), as int8 rows and as fp32 rows, at each slab
height (0 = auto).  The torch expression runs on the int8 rows, `torch_iters` calls per repeat; its records must equal the kernel's.
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
from gennbv_amd.ops.frontier import Frontier  # noqa: E402
from tools.microbench_view_cover import alternate  # noqa: E402
from tools.microbench_view_gain import mid_episode_grid, stats  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12


def torch_frontier(tri: torch.Tensor, g: int, block: int) -> torch.Tensor:
    """The records [N, nb^3, 4] int32 of int8 rows tri [N, G^3] as a torch expression."""
    n = tri.shape[0]
    t = tri.view(n, g, g, g)
    free = torch.nn.functional.pad(t < 0, (1, 1, 1, 1, 1, 1))
    near = free[:, :-2, 1:-1, 1:-1] | free[:, 2:, 1:-1, 1:-1] | free[:, 1:-1, :-2, 1:-1] | free[:, 1:-1, 2:, 1:-1] \
        | free[:, 1:-1, 1:-1, :-2] | free[:, 1:-1, 1:-1, 2:]
    front = (near & (t == 0)).view(n, -1).to(torch.int32)
    nb = (g + block - 1) // block
    ax = torch.arange(g, device=tri.device)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    rec = (((x // block) * nb + y // block) * nb + z // block).reshape(1, -1).expand(n, -1)
    out = torch.zeros(n, nb ** 3, 4, dtype=torch.int32, device=tri.device)
    for col, w in enumerate((None, x, y, z)):
        src = front if w is None else front * w.reshape(1, -1).to(torch.int32)
        out[..., col].scatter_add_(1, rec, src)
    return out


def frontier_case(n, g, args):
    cfg = TaskConfig(camera_width=320, camera_height=240, grid_size=g)
    base_n = min(n, 64)
    tri = mid_episode_grid(cfg, base_n, S.make_scenes(base_n, g, seed=1))
    tri_i8 = tri.repeat((n + base_n - 1) // base_n, 1)[:n].contiguous()
    del tri
    tri_f32 = tri_i8.to(torch.float32)
    fns, names, ops = [], [], []
    for slab in args.slab_list:
        for form, t in (("i8", tri_i8), ("f32", tri_f32)):
            if slab != 0 and form == "f32":
                continue
            fr = Frontier(n, g, block=args.block, device=DEV, slab=slab)
            ops.append(fr)
            fns.append(lambda fr=fr, t=t: fr(t))
            names.append(f"slab{slab}_{form}")
    with_bits = Frontier(n, g, block=args.block, device=DEV, keep_bits=True)
    ops.append(with_bits)
    fns.append(lambda: with_bits(tri_i8))
    names.append("slab0_i8_bits")
    us = alternate(fns, args.iters, args.repeats)
    assert all(torch.equal(ops[0].blocks, o.blocks) for o in ops), "the slab heights or forms disagree"
    want = torch_frontier(tri_i8, g, args.block)
    assert torch.equal(want, ops[0].blocks), "the torch expression disagrees with the kernel"
    del want
    torch.cuda.empty_cache()
    us_torch = alternate([lambda: torch_frontier(tri_i8, g, args.block)], args.torch_iters, args.repeats, warmup=1)[0]
    count = ops[0].count()
    r = {"envs": n, "grid": g, "block": args.block, "frontier_frac": float(count.float().mean()) / g ** 3,
         "nonempty_block_frac": float((ops[0].blocks[..., 0] > 0).float().mean())}
    for name, u in zip(names, us):
        r[name] = stats(u)
    r["torch_expression_i8"] = stats(us_torch)
    for form, size in (("i8", 1), ("f32", 4)):
        floor_us = 1e6 * n * g ** 3 * size / HBM_BYTES_PER_S
        r[f"floor_us_{form}"] = floor_us
        r[f"share_of_floor_{form}"] = floor_us / r[f"slab0_{form}"]["us_median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch_iters", type=int, default=2)
    ap.add_argument("--cases", default="256x64,512x128,8x64")
    ap.add_argument("--block", type=int, default=4)
    ap.add_argument("--slabs", default="0,4,8,16,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.slab_list = [int(s) for s in args.slabs.split(",")]
    if 0 not in args.slab_list:
        args.slab_list.insert(0, 0)
    if not torch.cuda.is_available():
        raise SystemExit("microbench_frontier needs a GPU")
    results = []
    for case in args.cases.split(","):
        n, g = (int(v) for v in case.split("x"))
        r = frontier_case(n, g, args)
        print(json.dumps(r), flush=True)
        results.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

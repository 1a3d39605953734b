"""Microbenchmark of the depth sensor kernel (csrc/sensor.hip, ops/depth_sensor.py) beside a device copy of the same two
tensors, and of the closed-loop env step without and with a sensor.

    python tools/microbench_sensor.py [--repeats 21] [--iters 10] [--envs 256,512] [--cases kernel,env_step] [--out FILE.json]

Device events around `iters` back-to-back calls, after warm-up, `repeats` times; reported: median / min / max us per call and
the spread.  The kernel's traffic is 16 bytes per pixel (depth and seg in, depth and seg out): 315 MB at 256 x 240 x 320, more than
the last-level cache holds, so back-to-back calls stream from HBM.  Rows, per batch size:

  copy                 depth_out.copy_(depth_in); seg_out.copy_(seg_in): the same bytes through the device's copy kernel
  r0 / r1 / r2         gnbv_depth_sensor alone (the library call on the operator's struct) with every effect on (noise,
                       dropouts, quantisation) at edge_radius 0 / 1 / 2, on a rendered frame of box scenes (hits, ground and
                       sky mixed); `vs_copy` is its time over the copy's
  r0_op / ...          DepthSensor.__call__: the same launch plus the frame counter's increment (a second, tiny launch)
  r0_miss              the same launch on an all-miss frame: no pixel is a return, so no pixel draws random words -- the
                       kernel's memory traffic alone; r0 minus this is what Philox and the arithmetic cost
  env_step             ReplayFeedEnv.step at 256 x 240 x 320 x 64^3 without a sensor and with the r1 sensor
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gennbv_amd import _lib  # noqa: E402
from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.replay_feed import ReplayFeedEnv  # noqa: E402
from gennbv_amd.ops.depth_sensor import DepthSensor  # noqa: E402
from tools.microbench_render import time_calls  # noqa: E402

DEV = "cuda:0"
H, W = 240, 320


def stats(us):
    med = float(np.median(us))
    return {"us_median": med, "us_min": float(min(us)), "us_max": float(max(us)), "spread_pct": 100.0 * (max(us) - min(us)) / med}


def make_sensor(n, radius):
    return DepthSensor(n, H, W, seed=1, min_range_m=0.3, max_range_m=30.0, edge_radius=radius, edge_abs_m=0.05, edge_rel=0.02,
                       edge_drop=0.7 if radius else 0.0, drop=0.02, sigma=(0.002, 0.0, 0.003), quant=600.0, device=DEV)


def launch(sensor):
    _lib.check(sensor.lib.gnbv_depth_sensor(C.byref(sensor.args), _lib.stream_ptr(sensor.device)), "gnbv_depth_sensor")


def kernel_rows(n, args):
    cfg = TaskConfig(camera_width=W, camera_height=H, grid_size=16)
    scene = S.make_scenes(n, 16, seed=1)
    feed = RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg, with_rgba=False)
    gen = torch.Generator().manual_seed(5)
    env = ReplayFeedEnv(cfg, scene, feed, DEV)
    env.reset()
    env.step(S.sample_actions(n, cfg, gen).to(DEV))
    depth, seg = feed.depth_raw.clone(), feed.seg_raw.clone()
    del env
    out_d, out_s = torch.empty_like(depth), torch.empty_like(seg)
    nbytes = 16 * n * H * W
    rows = []

    def row(name, fn, extra=None):
        r = {"case": name, "envs": n, "h": H, "w": W, "bytes": nbytes}
        r.update(stats(time_calls(fn, args.iters, args.repeats)))
        r["gb_per_s"] = nbytes / r["us_median"] * 1e-3
        r.update(extra or {})
        rows.append(r)
        return r

    def copy():
        out_d.copy_(depth)
        out_s.copy_(seg)
    base = row("copy", copy)
    for radius in (0, 1, 2):
        sensor = make_sensor(n, radius)
        sensor(depth, seg, out=(out_d, out_s))  # (fills the struct's pointers)
        r = row(f"r{radius}", lambda: launch(sensor))
        r["vs_copy"] = r["us_median"] / base["us_median"]
        row(f"r{radius}_op", lambda: sensor(depth, seg, out=(out_d, out_s)))
        r["returns_share"] = float((torch.isfinite(depth) & (depth <= -0.3) & (depth >= -30.0)).float().mean())
        r["no_return_share"] = float((out_d == -2.0 ** -100).float().mean())
    miss = torch.full_like(depth, float("-inf"))
    sensor = make_sensor(n, 0)
    sensor(miss, seg, out=(out_d, out_s))
    r = row("r0_miss", lambda: launch(sensor))
    r["vs_copy"] = r["us_median"] / base["us_median"]
    return rows


def env_step_rows(args, n=256, g=64):
    rows = []
    for with_sensor in (False, True):
        cfg = TaskConfig(camera_width=W, camera_height=H, grid_size=g)
        scene = S.make_scenes(n, g, seed=1)
        sensor = make_sensor(n, 1) if with_sensor else None
        env = ReplayFeedEnv(cfg, scene, RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg, sensor=sensor), DEV)
        env.reset()
        gen = torch.Generator().manual_seed(5)
        acts = [S.sample_actions(n, cfg, gen).to(DEV) for _ in range(8)]
        k = [0]

        def step():
            env.step(acts[k[0] % len(acts)])
            k[0] += 1
        r = {"case": "env_step", "envs": n, "h": H, "w": W, "grid": g, "sensor": with_sensor}
        r.update(stats(time_calls(step, args.iters, args.repeats)))
        rows.append(r)
        del env
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--envs", default="256,512")
    ap.add_argument("--cases", default="kernel,env_step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_sensor needs a GPU")
    results = []
    for c in args.cases.split(","):
        if c == "kernel":
            rows = [r for n in args.envs.split(",") for r in kernel_rows(int(n), args)]
        elif c == "env_step":
            rows = env_step_rows(args)
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

"""The shared case table of the measured-frame view gain (tests/test_carve_cpu.py, tests/test_carve_gpu.py).

TEST INFRASTRUCTURE.  A case is (g, stride, k): 3 envs of make_scenes' boxes, a 30 x 37 camera (w % 4 != 0; 1 110 rays at stride
1: more than one pass of rays per lane), k look-at poses per env of which env 0's first stands outside the grid, range 12 m (so
that far ground lies beyond it), the updater's depth_sense_dist.  `build` renders the depth through a caller's renderer (the
analytic one on the CPU, the mesh renderer on the GPU), writes rows of special values into every image and takes env 0's grid
from a caller's voxel update of its first frame; the other envs get random grids (5 % occupied, 40 % free).  `ray_classes` counts
the rays of a built case per class, by the oracle alone.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import carve_oracle as CO
from tests import gain_masks_oracle as MO

N, H, W, RANGE = 3, 30, 37, 12.0
CASES = [(g, stride, k) for g in (7, 16, 33) for stride in (1, 3) for k in (1, 3)]
CHUNKS = (0, 1, 2)
CLASSES = ("surface_fg", "surface_ground", "range_miss", "beyond_range", "stopped_early", "target_outside", "target_excluded")

# the rows v = 1 (mod 3) lie on the lattice of stride 1 and of stride 3; one special per row
SPECIAL_ROWS = {1: "-inf", 4: "nan", 7: "zeros", 10: "positive", 13: "clamp", 16: "beyond", 19: "source"}


def cfg_of(g: int) -> TaskConfig:
    return TaskConfig(camera_width=W, camera_height=H, grid_size=g)


def poses_of(k: int, seed: int, n: int = N) -> torch.Tensor:
    """[n, k, 6] f32: cameras above the boxes (z 9.2 .. 9.8, inside the grid) that look at (0, 0, 2.5) plus a few degrees of
    jitter, so that the top image rows see the sky; env 0's first camera stands outside the grid."""
    rs = np.random.RandomState(seed)
    p = torch.zeros(n, k, 6)
    for e in range(n):
        for j in range(k):
            ang = rs.uniform(0, 2 * math.pi)
            rad = rs.uniform(4.0, 7.0)
            x, y, z = rad * math.cos(ang), rad * math.sin(ang), rs.uniform(9.2, 9.8)
            if e == 0 and j == 0:
                x, y, z = -11.0, 3.0, 6.0
            p[e, j, :3] = torch.tensor([x, y, z])
            p[e, j, 5] = (math.atan2(-y, -x) + rs.uniform(-0.1, 0.1)) % (2 * math.pi)
            p[e, j, 4] = math.atan2(z - 2.5, math.hypot(x, y)) - 0.45 + rs.uniform(-0.05, 0.05)
    return p


def write_specials(depth: torch.Tensor, sense_dist: float) -> torch.Tensor:
    """depth [..., H, W], in place: the rows of SPECIAL_ROWS."""
    inf = float("inf")
    half = W // 2
    for v, what in SPECIAL_ROWS.items():
        row = depth[..., v, :]
        if what == "-inf":
            row[...] = -inf
        elif what == "nan":
            row[..., :half] = float("nan")
            row[..., half:] = inf
        elif what == "zeros":
            row[..., :half] = 0.0
            row[..., half:] = -0.0
        elif what == "positive":   # the updater takes |d|: a surface 3 m away
            row[...] = 3.0
        elif what == "clamp":      # at and below the clamp: not a surface
            row[..., :half] = sense_dist
            row[..., half:] = sense_dist - 10.0
        elif what == "beyond":     # a hit the updater keeps, beyond the range
            row[...] = -(RANGE + 5.0)
        elif what == "source":     # the target is the source voxel
            row[...] = -1e-3
    return depth


def build(case, render, update, seed: int = 5, n: int = N):
    """`n` envs (the table's cases have N).  render(scene, poses [n,6]) -> (depth_raw, seg_raw) [n,H,W] f32 torch (any device);
    update(scene, cfg, depth_raw, seg_raw, poses [n,6]) -> tri [n, g^3] (any dtype, taken by sign; env 0's row is used).
    -> dict of CPU tensors / numbers."""
    g, stride, k = case
    cfg = cfg_of(g)
    scene = S.make_scenes(n, g, seed=seed)
    poses = poses_of(k, seed + 10 * g + k, n)
    depth = torch.empty(n, k, H, W)
    seg = torch.empty(n, k, H, W)
    for j in range(k):
        d, s = render(scene, poses[:, j].contiguous())
        depth[:, j], seg[:, j] = d.cpu(), s.cpu()
    write_specials(depth, cfg.depth_sense_dist)
    tri = MO.random_tri(n, g, 0.05, seed=seed + g)
    tri0 = update(scene, cfg, depth[:, 0].contiguous(), seg[:, 0].contiguous(), poses[:, 0].contiguous())
    tri[0] = torch.sign(torch.as_tensor(tri0).reshape(n, -1)[0].float()).to(torch.int8)
    return dict(cfg=cfg, scene=scene, poses=poses, depth=depth, seg=seg, tri=tri, n=n, g=g, stride=stride, k=k,
                sense=float(cfg.depth_sense_dist), kinv=S.inverse_intrinsics(H, W, cfg.horizontal_fov).numpy())


def ray_classes(built, c2w) -> dict:
    """Rays of the built case per class of CLASSES, over all envs and candidates; c2w [N,k,4,4]."""
    n, g, stride, k = built["n"], built["g"], built["stride"], built["k"]
    rng, vox = built["scene"].range_gt.numpy(), built["scene"].voxel_size.numpy()
    depth, seg, tri = built["depth"].numpy(), built["seg"].numpy(), built["tri"].numpy()
    c2w = np.asarray(c2w, np.float32).reshape(n, k, 4, 4)
    out = dict.fromkeys(CLASSES, 0)
    for e in range(n):
        cls = np.sign(tri[e].astype(np.int64))
        for j in range(k):
            rays = CO.ray_voxels(c2w[e, j], depth[e, j], rng[e], vox[e], built["kinv"], H, W, stride, RANGE, built["sense"], g)
            f = CO.ray_fates(cls, rays)
            raw, fg = depth[e, j][rays.vs, rays.us], seg[e, j][rays.vs, rays.us] > 0
            ranged = ~rays.surface
            with np.errstate(invalid="ignore"):
                beyond = ranged & np.isfinite(raw) & (raw > built["sense"]) & (np.abs(raw) > RANGE)
            # the ray's last in-grid voxel, had nothing stopped it
            last = np.where(rays.valid.any(1), rays.lin[np.arange(len(rays.lin)), np.maximum(rays.valid.sum(1) - 1, 0)], -1)
            occ = (cls[rays.lin] == 1) & rays.valid
            stop_lin = rays.lin[np.arange(len(rays.lin)), occ.argmax(1)]
            out["surface_fg"] += int((rays.surface & fg).sum())
            out["surface_ground"] += int((rays.surface & ~fg).sum())
            out["range_miss"] += int((ranged & np.isneginf(raw)).sum())
            out["beyond_range"] += int(beyond.sum())
            out["stopped_early"] += int((f.blocked & (stop_lin != last)).sum())
            out["target_outside"] += int((rays.tgt_lin < 0).sum())
            out["target_excluded"] += int(f.excluded.sum())
    return out

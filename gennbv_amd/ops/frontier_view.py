"""Frontier viewpoints: where to stand to see a frontier target, and what the flight there costs (csrc/frontview.hip).

    fv = FrontierViewpoints(num_envs, grid_size, lattice, range_gt, voxel_size, targets=8, r_min_m=0.5, r_max_m=4.0)
    node, cost_mm, count = fv(tri, field, target_vox)   # one launch

For env e and target voxel target_vox[e, j] (int32 [N,T,3]; a coordinate outside the grid: no target): among the nodes of the
flight lattice within [r_min_m, r_max_m] of the target's centre whose Bresenham line to the target crosses no occupied voxel and at
most `max_unknown` unknown ones (include/gennbv_hip.h gnbv_frontier_viewpoints has the exact rule), `node` [N,T] int32 is the one
with the smallest (field value, node id), -1 where there is none; `cost_mm` [N,T] its field value (u32 bits in an int32 tensor,
0xFFFFFFFF where node is -1); `count` [N,T,2] = {nodes that see the target, of which with a route}.  `tri` takes the forms
Frontier takes; `field` is a FlightField (BeliefFlightField) or its `field` tensor [N, M].  GPU only.

block_target_voxels, node_actions and aim_indices are the plain-torch glue between the frontier's block records, the kernel and
the task's action lattice (any device).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .. import _lib


def block_target_voxels(blocks: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """int32 [N,m,3]: per axis sum_a // count of the records blocks[e, index[e, j]] (blocks [N, nb^3, 4] = {count, sum x, sum y,
    sum z}) -- the voxel that holds the block's frontier centroid; -1 on every axis where the block is empty."""
    rec = blocks.gather(1, index[..., None].expand(-1, -1, 4)).to(torch.int64)
    cnt = rec[..., :1]
    vox = rec[..., 1:] // cnt.clamp(min=1)
    return torch.where(cnt > 0, vox, torch.full_like(vox, -1)).to(torch.int32)


def node_actions(lattice, cfg, node: torch.Tensor) -> torch.Tensor:
    """int64 [..., 3]: the position indices on the task's action lattice (pose = action * action_unit + clip_pose_low) of flight
    lattice node ids [...].  Node (i, j, k) of FlightLattice(cfg, stride) is action clip_pose_idx_low + stride * i on an axis with
    a unit >= 0 and clip_pose_idx_up - stride * i where the unit is negative (the lattice counts its nodes from the low end of the
    axis).  A negative id is read as node 0: the caller masks it."""
    nx, ny, _ = lattice.dims
    c = node.to(torch.int64).clamp(min=0)
    ijk = torch.stack([c % nx, (c // nx) % ny, c // (nx * ny)], dim=-1)
    out = []
    for a in range(3):
        step = ijk[..., a] * int(lattice.stride)
        if float(cfg.action_unit[a]) < 0.0:
            out.append(int(cfg.clip_pose_idx_up[a]) - step)
        else:
            out.append(int(cfg.clip_pose_idx_low[a]) + step)
    return torch.stack(out, dim=-1)


def aim_indices(p: torch.Tensor, c: torch.Tensor, pitch_angles: torch.Tensor, yaw_angles: torch.Tensor, pitch_low, yaw_low,
                base_yaw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(pitch, yaw) lattice indices [...] that make a camera at p [..., 3] look at c [..., 3] (fp64): yaw is the index whose angle
    (yaw_angles, fp64, index yaw_low first) is circularly nearest to atan2(c_y - p_y, c_x - p_x), pitch the index nearest to
    atan2(p_z - c_z, hypot(c_x - p_x, c_y - p_y)) (camera_to_world's sign: forward = (cos p cos y, cos p sin y, -sin p)); both an
    argmin in fp64, lowest index on ties; where the horizontal offset is zero `base_yaw` stays."""
    dx, dy = c[..., 0] - p[..., 0], c[..., 1] - p[..., 1]
    want_yaw = torch.atan2(dy, dx)
    want_pitch = torch.atan2(p[..., 2] - c[..., 2], torch.hypot(dx, dy))
    two_pi = 2.0 * torch.pi
    d_yaw = (torch.remainder(yaw_angles - want_yaw[..., None] + torch.pi, two_pi) - torch.pi).abs()
    yaw = d_yaw.argmin(dim=-1) + yaw_low  # (argmin returns the first minimum: the lowest index on ties)
    yaw = torch.where((dx == 0) & (dy == 0), base_yaw, yaw)
    pitch = (pitch_angles - want_pitch[..., None]).abs().argmin(dim=-1) + pitch_low
    return pitch, yaw


class FrontierViewpoints:
    def __init__(self, num_envs: int, grid_size: int, lattice, range_gt: torch.Tensor, voxel_size: torch.Tensor, targets: int,
                 r_min_m: float, r_max_m: float, max_unknown: int = 0, mode: int = 0, device="cuda:0", chunk: int = 0):
        n, g, t = int(num_envs), int(grid_size), int(targets)
        r0, r1 = float(r_min_m), float(r_max_m)
        if n < 1 or t < 1 or not 1 <= g <= 128 or int(max_unknown) < 0 or int(mode) not in (0, 1, 2) or int(chunk) < 0:
            raise ValueError(f"FrontierViewpoints: num_envs >= 1, targets >= 1, grid_size in 1..128, max_unknown >= 0, mode in 0..2, "
                             f"chunk >= 0; got {num_envs}, {targets}, {grid_size}, {max_unknown}, {mode}, {chunk}")
        if not (np.isfinite(r0) and np.isfinite(r1) and 0.0 <= r0 <= r1 and r1 > 0.0):
            raise ValueError(f"FrontierViewpoints: 0 <= r_min_m <= r_max_m, finite, r_max_m > 0; got {r_min_m}, {r_max_m}")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.GennbvHipError("FrontierViewpoints runs on the GPU only (no CPU fallback)")
        self.lib = _lib.load()
        if int(mode) == 1 and g > int(self.lib.gnbv_frontview_lds_max_grid()):
            raise _lib.GennbvHipError(f"FrontierViewpoints: the classes of a {g}^3 grid do not fit LDS (mode 1)")
        self.num_envs, self.grid_size, self.targets, self.lattice, self.device = n, g, t, lattice, device
        self.r_min_m, self.r_max_m, self.max_unknown, self.mode, self.chunk = r0, r1, int(max_unknown), int(mode), int(chunk)
        self.range_gt = range_gt.to(device, torch.float32).contiguous()
        self.voxel_size = voxel_size.to(device, torch.float32).contiguous()
        assert self.range_gt.shape == (n, 6) and self.voxel_size.shape == (n, 3)
        self.node = torch.full((n, t), -1, dtype=torch.int32, device=device)
        self.cost_mm = torch.full((n, t), -1, dtype=torch.int32, device=device)  # u32 bits
        self.count = torch.zeros(n, t, 2, dtype=torch.int32, device=device)
        self.launches = 0

    def __call__(self, tri: torch.Tensor, field, target_vox: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One gnbv_frontier_viewpoints launch on the current stream into `node`, `cost_mm`, `count`; returns the three."""
        n, g3, t = self.num_envs, self.grid_size ** 3, self.targets
        m = int(self.lattice.num_nodes)
        tri_i8, tri_i8_row, tri_f32, tri_f32_row = _lib.tri_args(tri, n, g3, "FrontierViewpoints")
        field = getattr(field, "field", field)
        _lib.require_cuda(field)
        if field.dtype != torch.int32 or field.shape != (n, m) or not field.is_contiguous():
            raise _lib.GennbvHipError(f"FrontierViewpoints: field must be a contiguous int32 [{n}, {m}] tensor of u32 bits, got "
                                      f"{field.dtype} {tuple(field.shape)}")
        _lib.require_cuda(target_vox)
        if target_vox.dtype != torch.int32 or target_vox.shape != (n, t, 3) or not target_vox.is_contiguous():
            raise _lib.GennbvHipError(f"FrontierViewpoints: target_vox must be a contiguous int32 [{n}, {t}, 3] tensor, got "
                                      f"{target_vox.dtype} {tuple(target_vox.shape)}")
        nx, ny, nz = self.lattice.dims
        a = _lib.GnbvFrontView(n=n, t=t, g=self.grid_size, tri_i8=tri_i8, tri_i8_row_stride=tri_i8_row, tri_f32=tri_f32,
                               tri_f32_row_stride=tri_f32_row,
                               range_gt=self.range_gt.data_ptr(), voxel_size=self.voxel_size.data_ptr(), nx=nx, ny=ny, nz=nz,
                               lo=(_lib.C.c_double * 3)(*[float(v) for v in self.lattice.lo]),
                               h=(_lib.C.c_double * 3)(*[float(v) for v in self.lattice.h]), field=field.data_ptr(),
                               targets=target_vox.data_ptr(), r_min=self.r_min_m, r_max=self.r_max_m, max_unknown=self.max_unknown,
                               node_out=self.node.data_ptr(), cost_out=self.cost_mm.data_ptr(), count_out=self.count.data_ptr(),
                               chunk=self.chunk, mode=self.mode)
        _lib.check(self.lib.gnbv_frontier_viewpoints(_lib.C.byref(a), _lib.stream_ptr(self.device)), "gnbv_frontier_viewpoints")
        self.launches += 1
        return self.node, self.cost_mm, self.count


__all__ = ["FrontierViewpoints", "block_target_voxels", "node_actions", "aim_indices"]

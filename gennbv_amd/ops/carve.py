"""CarvedMap: the map a pilot can fly on -- the observation's tri-class grid plus the free space along EVERY camera ray
(csrc/viewgain.hip, the view gain of a measured frame: include/gennbv_hip.h GnbvViewGain depth_raw / carve_i8).

The voxel update carves free space only along the rays that hit foreground, as the reference does.  A depth frame says more: a
ray that hit the ground was free up to the ground, a ray that hit nothing was free up to the sensor's range.  CarvedMap keeps
that as a second map beside the observation, `map_i8` int8 [N, G^3] (< 0 free, 0 unknown, > 0 occupied; all zero at first); the
observation, the rewards and every reference-parity path stay what they are.

    update(tri, depth_raw, poses, reset_mask=None)
      1. map = where(reset | tri != 0, tri, map): a reset env starts from its fresh grid; elsewhere the observation's class wins
         wherever it has one, and earlier carving survives where the observation is still unknown;
      2. one launch of the measured-frame view gain with k = 1, tri_i8 = carve_i8 = map_i8 and the env's own camera: every
         unknown voxel a lattice ray crosses before its first occupied voxel becomes free, but the voxel a surface-ended ray
         ends in.

`last_gain` int32 [N, 1, 3] is the launch's gain: `[:, 0, 0]` is the number of voxels newly carved.  The rays are the pixel
lattice of `stride` (2 by default: a stated choice, not a measured one); `range_m` defaults to |cfg.depth_sense_dist|.  Runs on
the current stream, no host synchronisation.  GPU only, no CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ..env.config import TaskConfig
from .view_gain import make_view_gain


def merge_observation(map_i8: torch.Tensor, tri: torch.Tensor, reset_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Step 1 of CarvedMap.update, in place on map_i8 int8 [N, G^3]: tri (int8, or the fp32 grid slice of a flat observation,
    taken by sign; [N, G^3] or [N,G,G,G], any row stride) replaces the map where it is not unknown and, whole, in the envs whose
    reset_mask [N] is non-zero.  Plain torch on the tensors' device."""
    n = map_i8.shape[0]
    tri = tri.reshape(n, -1)
    if tri.shape != map_i8.shape:
        raise _lib.GennbvHipError(f"CarvedMap: tri must hold {tuple(map_i8.shape)} voxels, got {tuple(tri.shape)}")
    if tri.dtype != torch.int8:
        # fp32 rows: the classes from two comparisons written straight into the map -- no fp32 temporary of the grid's size
        if reset_mask is not None:
            map_i8.masked_fill_(reset_mask.reshape(n, 1) != 0, 0)
        map_i8.masked_fill_(tri > 0, 1)
        map_i8.masked_fill_(tri < 0, -1)
        return map_i8
    t = torch.sign(tri)
    take = t != 0
    if reset_mask is not None:
        take |= reset_mask.reshape(n, 1) != 0
    torch.where(take, t, map_i8, out=map_i8)  # elementwise: out may be an input
    return map_i8


class CarvedMap:
    def __init__(self, num_envs: int, cfg: TaskConfig, range_gt: torch.Tensor, voxel_size: torch.Tensor, stride: int = 2,
                 range_m: Optional[float] = None, inv_intrinsics: Optional[torch.Tensor] = None, device="cuda:0", slab: int = 0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("CarvedMap runs on the GPU only (no CPU fallback)")
        self.num_envs, self.g = int(num_envs), int(cfg.grid_size)
        self.h, self.w, self.stride = int(cfg.camera_height), int(cfg.camera_width), int(stride)
        # the LDS kernel up to 64^3 (one workgroup per env at k = 1), the slab kernels above
        self.op = make_view_gain(self.num_envs, 1, cfg, range_gt, voxel_size, inv_intrinsics, self.stride, range_m, self.device, slab=slab)
        self.range_m = self.op.range_m
        self.map_i8 = torch.zeros(self.num_envs, self.g ** 3, dtype=torch.int8, device=self.device)
        self.last_gain = self.op.gain

    def update(self, tri: torch.Tensor, depth_raw: torch.Tensor, poses: torch.Tensor, reset_mask: Optional[torch.Tensor] = None):
        """tri: the grid the voxel update has just written (int8 rows or the observation's fp32 slice); depth_raw [N,H,W] f32,
        the frame it was written from; poses [N,>=6] f32, the poses the frame was taken at (the camera is the pose's matrix);
        reset_mask [N] uint8 / bool or None.  -> map_i8."""
        _lib.require_cuda(tri, depth_raw, poses)
        n = self.num_envs
        if poses.dtype != torch.float32 or poses.dim() != 2 or poses.shape[0] != n or poses.shape[1] < 6:
            raise _lib.GennbvHipError(f"CarvedMap: poses must be f32 [{n}, >=6], got {poses.dtype} {tuple(poses.shape)}")
        if depth_raw.dtype != torch.float32 or depth_raw.shape != (n, self.h, self.w):
            raise _lib.GennbvHipError(f"CarvedMap: depth_raw must be f32 [{n}, {self.h}, {self.w}], got {depth_raw.dtype} "
                                      f"{tuple(depth_raw.shape)}")
        merge_observation(self.map_i8, tri, reset_mask)
        self.op(self.map_i8, poses[:, :6].reshape(n, 1, 6), depth=depth_raw, carve_out=self.map_i8)
        return self.map_i8

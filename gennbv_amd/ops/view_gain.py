"""ViewGain: how much would each env's map change if its camera went to candidate pose j?  (csrc/viewgain.hip)

For the tri-class grid an env holds now (the observation's grid slice) and K candidate poses per env, the voxel update's ray
model is run hypothetically: per candidate three int32 -- distinct unknown voxels the rays of a pixel lattice would cross
before their first occupied voxel, the same over the rays that meet one, and the number of those rays (the exact definition:
include/gennbv_hip.h gnbv_view_gain).  One launch for all N x K candidates; outputs are preallocated and reused: a result is
valid until the next call.  GPU only, no CPU fallback.

With `depth` (the raw depth images measured at the poses) the same call is the view gain of a MEASURED frame: every ray ends
where its pixel's depth says, and `carve_out` receives -1 in every unknown voxel a ray crossed (ops/carve.py CarvedMap is the
map built on it).

ViewGain keeps an env's grid in LDS (grid_size <= 64); ViewGainSlab computes the same integers for grid_size <= 128 through
gnbv_view_gain_slab (the rays' fates first, then slabs of x-planes) with a preallocated workspace; make_view_gain picks.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ..env import synthetic as S
from ..env.config import TaskConfig

MAX_GRID = 64  # the grid (2 bits per voxel) and two visited masks live in LDS: G^3 / 2 bytes
MAX_GRID_SLAB = 128  # ViewGainSlab


class ViewGain:
    _max_grid = MAX_GRID

    def __init__(self, num_envs: int, k: int, cfg: TaskConfig, range_gt: torch.Tensor, voxel_size: torch.Tensor,
                 inv_intrinsics: Optional[torch.Tensor] = None, stride: int = 4, range_m: Optional[float] = None,
                 device="cuda:0", with_c2w: bool = False, chunk: int = 0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("ViewGain runs on the GPU only (no CPU fallback)")
        g = int(cfg.grid_size)
        if g > self._max_grid:
            raise _lib.GennbvHipError(f"{type(self).__name__}: grid_size <= {self._max_grid}, got {g}" + (
                " (ViewGain keeps the grid and its visited masks in LDS; ViewGainSlab / make_view_gain go up to "
                f"{MAX_GRID_SLAB})" if self._max_grid == MAX_GRID else ""))
        self.lib = _lib.load()
        self.num_envs, self.k, self.g = int(num_envs), int(k), g
        self.h, self.w, self.stride = int(cfg.camera_height), int(cfg.camera_width), int(stride)
        self.range_m = float(abs(cfg.depth_sense_dist) if range_m is None else range_m)
        kinv = S.inverse_intrinsics(self.h, self.w, cfg.horizontal_fov) if inv_intrinsics is None else inv_intrinsics
        self.inv_intri_host = kinv.detach().to("cpu", torch.float32).contiguous()
        assert self.inv_intri_host.shape == (3, 3)
        dev = self.device
        self.range_gt = range_gt.to(dev, torch.float32).contiguous()
        self.voxel_size = voxel_size.to(dev, torch.float32).contiguous()
        assert self.range_gt.shape == (self.num_envs, 6) and self.voxel_size.shape == (self.num_envs, 3)
        self.gain = torch.empty(self.num_envs, self.k, 3, dtype=torch.int32, device=dev)
        self.c2w = torch.empty(self.num_envs, self.k, 4, 4, dtype=torch.float32, device=dev) if with_c2w else None
        a = _lib.GnbvViewGain()
        a.n, a.k, a.g = self.num_envs, self.k, g
        a.range_gt, a.voxel_size = self.range_gt.data_ptr(), self.voxel_size.data_ptr()
        a.inv_intri = self.inv_intri_host.data_ptr()
        a.h, a.w, a.stride, a.range = self.h, self.w, self.stride, self.range_m
        a.gain, a.c2w_out = self.gain.data_ptr(), _lib.ptr(self.c2w)
        a.chunk, a.ablate = int(chunk), 0
        self.depth_sense_dist = float(cfg.depth_sense_dist)
        self._args = a

    def __call__(self, tri: torch.Tensor, poses: torch.Tensor, depth: Optional[torch.Tensor] = None,
                 carve_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tri: int8 rows [N, G^3] (or [N,G,G,G]; unit element stride, any row stride) or the fp32 grid slice of a flat
        observation (converted with one .to(torch.int8)); poses [N,K,6] f32 (x, y, z, roll, pitch, yaw), env-local.
        -> gain [N,K,3] int32 (unknown, unknown_hit, blocked).
        depth: None, or the raw depth images measured at the poses, f32 [N,K,H,W] ([N,H,W] with K = 1): the view gain of a
        measured frame (include/gennbv_hip.h), rays ended by their pixel's depth.  carve_out: with depth only, int8 rows
        [N, G^3] (unit element stride) in which every unknown voxel a ray visited becomes -1; it may be `tri` itself where the
        header allows it (K = 1, or the slab operators)."""
        _lib.require_cuda(tri, poses)
        n, k, g3 = self.num_envs, self.k, self.g ** 3
        if tri.dtype != torch.int8:
            tri = tri.to(torch.int8)
        if tri.shape[0] != n or tri.numel() != n * g3:
            raise _lib.GennbvHipError(f"ViewGain: tri must hold [{n}, {g3}] voxels, got {tuple(tri.shape)}")
        if tri.dim() != 2:
            tri = tri.reshape(n, g3)
        if tri.stride(1) != 1:
            tri = tri.contiguous()
        if poses.dtype != torch.float32 or poses.shape != (n, k, 6):
            raise _lib.GennbvHipError(f"ViewGain: poses must be f32 [{n}, {k}, 6], got {poses.dtype} {tuple(poses.shape)}")
        poses = poses.contiguous()
        a = self._args
        a.tri_i8, a.tri_row_stride, a.poses = tri.data_ptr(), max(int(tri.stride(0)), g3), poses.data_ptr()
        a.depth_raw = a.carve_i8 = None
        a.depth_env_stride = a.depth_cand_stride = a.carve_row_stride = 0
        a.depth_sense_dist = 0.0
        if carve_out is not None and depth is None:
            raise _lib.GennbvHipError("ViewGain: carve_out needs depth")
        if depth is not None:
            _lib.require_cuda(depth)
            hw = self.h * self.w
            if depth.dtype != torch.float32 or depth.shape[0] != n or depth.numel() != n * k * hw:
                raise _lib.GennbvHipError(f"ViewGain: depth must be f32 [{n}, {k}, {self.h}, {self.w}], got {depth.dtype} {tuple(depth.shape)}")
            depth = depth.contiguous()
            a.depth_raw, a.depth_env_stride, a.depth_cand_stride = depth.data_ptr(), k * hw, hw
            a.depth_sense_dist = self.depth_sense_dist
            if carve_out is not None:
                _lib.require_cuda(carve_out)
                if carve_out.dtype != torch.int8 or carve_out.dim() != 2 or carve_out.shape != (n, g3) or carve_out.stride(1) != 1:
                    raise _lib.GennbvHipError(f"ViewGain: carve_out must be int8 rows [{n}, {g3}] with unit element stride, got "
                                              f"{carve_out.dtype} {tuple(carve_out.shape)}")
                a.carve_i8, a.carve_row_stride = carve_out.data_ptr(), max(int(carve_out.stride(0)), g3)
        self._launch(a)
        return self.gain

    def _launch(self, a):
        _lib.check(self.lib.gnbv_view_gain(C.byref(a), _lib.stream_ptr(self.device)), "gnbv_view_gain")


def slab_workspace(op, name: str) -> None:
    """The workspace of the slab path for operator `op` (ViewGainSlab, ViewGainMasksSlab): the library's size for the operator's
    shapes, its refusal under `name`, and the allocation, once; sets op.workspace_bytes and op.workspace."""
    op.workspace_bytes = int(op.lib.gnbv_view_gain_slab_workspace_bytes(op.num_envs, op.k, op.g, op.h, op.w, op.stride))
    if op.workspace_bytes == 0:
        raise _lib.GennbvHipError(f"{name}: sizes refused (n {op.num_envs}, k {op.k}, g {op.g}, camera {op.h}x{op.w}, stride {op.stride})")
    op.workspace = torch.empty(op.workspace_bytes, dtype=torch.uint8, device=op.device)


class ViewGainSlab(ViewGain):
    """The same operator for grid_size <= 128 (gnbv_view_gain_slab): ViewGain's arguments plus `slab`, the x-planes per
    slab (0 = chosen from the grid size; any height gives the same integers).  The workspace is allocated once, here."""
    _max_grid = MAX_GRID_SLAB

    def __init__(self, num_envs: int, k: int, cfg: TaskConfig, range_gt: torch.Tensor, voxel_size: torch.Tensor,
                 inv_intrinsics: Optional[torch.Tensor] = None, stride: int = 4, range_m: Optional[float] = None,
                 device="cuda:0", with_c2w: bool = False, chunk: int = 0, slab: int = 0):
        super().__init__(num_envs, k, cfg, range_gt, voxel_size, inv_intrinsics, stride, range_m, device, with_c2w, chunk)
        self.slab = int(slab)
        slab_workspace(self, "ViewGainSlab")

    def _launch(self, a):
        _lib.check(self.lib.gnbv_view_gain_slab(C.byref(a), self.slab, self.workspace.data_ptr(), self.workspace_bytes,
                                                _lib.stream_ptr(self.device)), "gnbv_view_gain_slab")


def make_view_gain(num_envs: int, k: int, cfg: TaskConfig, *args, **kwargs) -> ViewGain:
    """ViewGain for grid_size <= 64 (one launch, the grid in LDS), ViewGainSlab above; `slab` is passed to the latter only."""
    if int(cfg.grid_size) <= MAX_GRID:
        kwargs.pop("slab", None)
        return ViewGain(num_envs, k, cfg, *args, **kwargs)
    return ViewGainSlab(num_envs, k, cfg, *args, **kwargs)

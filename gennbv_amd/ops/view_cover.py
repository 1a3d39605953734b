"""ViewCover: which ground-truth voxels would the voxel update mark if an env's camera stood at candidate pose j?
(csrc/viewcover.hip)

The renderer's trace and the update's back-projection fused into one launch for all N x K candidates, without an image in
between: per candidate three int32 -- ground-truth voxels the view would ADD to the scanned set (the coverage reward's
numerator increment), ground-truth voxels it sees at all, and its foreground pixels that land inside the grid (the exact
definition: include/gennbv_hip.h gnbv_view_cover).  At stride 1 with the env's own camera the first integer is exactly the
`coverage_count` increment a step to that pose pays.  `accumulate` ORs the seen ground-truth voxels of all candidates into a
bit row per env: the observable ground truth (MeshScene.observable_ground_truth).  Outputs are preallocated and reused: a
result is valid until the next call.  GPU only, no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ..env import synthetic as S
from ..env.config import TaskConfig

MAX_GRID = 128


class ViewCover:
    def __init__(self, mesh, cfg: TaskConfig, range_gt: torch.Tensor, voxel_size: torch.Tensor, k: int, stride: int = 1,
                 inv_intrinsics: Optional[torch.Tensor] = None, device=None, chunk: int = 0, window: int = 0):
        self.device = torch.device(mesh.device if device is None else device)
        if self.device.type != "cuda" or mesh.device.type != "cuda":
            raise _lib.GennbvHipError("ViewCover runs on the GPU only (no CPU fallback): build the MeshScene on a cuda device")
        g = int(cfg.grid_size)
        if not 2 <= g <= MAX_GRID:
            raise _lib.GennbvHipError(f"ViewCover: grid_size in 2..{MAX_GRID}, got {g}")
        if int(k) < 1 or int(stride) < 1:
            raise _lib.GennbvHipError(f"ViewCover: k >= 1 and stride >= 1, got k {k}, stride {stride}")
        self.lib = _lib.load()
        self.mesh = mesh
        self.num_envs, self.k, self.g = int(mesh.num_envs), int(k), g
        self.h, self.w, self.stride = int(cfg.camera_height), int(cfg.camera_width), int(stride)
        kinv = S.inverse_intrinsics(self.h, self.w, cfg.horizontal_fov) if inv_intrinsics is None else inv_intrinsics
        self.inv_intri_host = kinv.detach().to("cpu", torch.float32).contiguous()
        assert self.inv_intri_host.shape == (3, 3)
        dev, n = self.device, self.num_envs
        self.range_gt = range_gt.to(dev, torch.float32).contiguous()
        self.voxel_size = voxel_size.to(dev, torch.float32).contiguous()
        assert self.range_gt.shape == (n, 6) and self.voxel_size.shape == (n, 3)
        self.words = int(self.lib.gnbv_grid_bit_words(g))
        self.cover = torch.empty(n, self.k, 3, dtype=torch.int32, device=dev)
        self._scene = mesh.c_struct()
        a = _lib.GnbvViewCover()
        a.n, a.k, a.g = n, self.k, g
        a.range_gt, a.voxel_size = self.range_gt.data_ptr(), self.voxel_size.data_ptr()
        a.inv_intri = self.inv_intri_host.data_ptr()
        a.h, a.w, a.stride, a.depth_sense_dist = self.h, self.w, self.stride, float(cfg.depth_sense_dist)
        a.chunk, a.window = int(chunk), int(window)
        self._args = a

    def _check(self, poses, *bits):
        n, k = self.num_envs, self.k
        _lib.require_cuda(poses, *bits)
        if poses.dtype != torch.float32 or poses.shape != (n, k, 6):
            raise _lib.GennbvHipError(f"ViewCover: poses must be f32 [{n}, {k}, 6], got {poses.dtype} {tuple(poses.shape)}")
        for b in bits:
            if b is not None and (b.dtype != torch.int32 or b.shape != (n, self.words) or not b.is_contiguous()):
                raise _lib.GennbvHipError(f"ViewCover: bit rows must be contiguous int32 [{n}, {self.words}] "
                                          f"(gnbv_grid_bit_words), got {b.dtype} {tuple(b.shape)}")
        return poses.contiguous()

    def _launch(self, poses, gt_bits, scanned_bits, cover, seen_bits):
        a = self._args
        a.poses, a.gt_bits, a.scanned_bits = poses.data_ptr(), gt_bits.data_ptr(), _lib.ptr(scanned_bits)
        a.cover, a.seen_bits = _lib.ptr(cover), _lib.ptr(seen_bits)
        _lib.check(self.lib.gnbv_view_cover(C.byref(self._scene), C.byref(a), _lib.stream_ptr(self.device)), "gnbv_view_cover")

    def __call__(self, poses: torch.Tensor, gt_bits: torch.Tensor, scanned_bits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """poses [N,K,6] f32 (x, y, z, roll, pitch, yaw), env-local; gt_bits / scanned_bits int32 [N, words] in the
        updater's layout (OccupancyGridUpdater.gt_bits / .scanned_bits; None = nothing scanned)
        -> cover [N,K,3] int32 (new_gt, seen_gt, hits)."""
        poses = self._check(poses, gt_bits, scanned_bits)
        self._launch(poses, gt_bits, scanned_bits, self.cover, None)
        return self.cover

    def accumulate(self, poses: torch.Tensor, gt_bits: torch.Tensor, out_bits: torch.Tensor) -> torch.Tensor:
        """out_bits [N, words] int32 |= (voxels seen from any of poses [N,K,6]) & gt_bits.  The caller zeroes out_bits, or
        keeps accumulating over batches of candidates."""
        poses = self._check(poses, gt_bits, out_bits)
        self._launch(poses, gt_bits, None, None, out_bits)
        return out_bits

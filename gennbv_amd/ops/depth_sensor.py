"""DepthSensor: the depth camera a policy would really fly with, between the renderer and everything that reads a frame
(csrc/sensor.hip; include/gennbv_hip.h gnbv_depth_sensor has the exact rule, DESIGN.md "Depth sensor model" the reasons).

gnbv_render_depth returns the exact ray parameter of every pixel and an exact silhouette.  DepthSensor turns such a frame into a
measured one: returns outside [min_range_m, max_range_m] are lost, pixels at depth edges and at random drop out, the range
carries noise of sigma = s0 + s1 t + s2 t^2 metres and is quantised in disparity (t = quant / round(quant / t)).  A pixel
without a return carries NO_RETURN with seg 0: a tiny negative depth that the voxel update, the scan set and the carve kernels
all treat as "nothing seen along this ray" -- no foreground point, no free space.

    sensor = DepthSensor(n, h, w, min_range_m=0.3, max_range_m=20.0, sigma=(0.0, 0.0, 0.002), edge_radius=1, edge_rel=0.05,
                         edge_drop=0.7, drop=0.01, quant=600.0)
    depth, seg = sensor(depth_raw, seg_raw)          # one launch on the current stream, then frame += 1 on the device

The noise of env e is a pure function of (seed, frame[e], e, pixel): two sensors with the same seed and frame counters give the
same bits, whatever the batch holds.  GPU only, no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from statistics import NormalDist
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib

NO_RETURN = float(np.float32(-2.0 ** -100))  # GNBV_DEPTH_NO_RETURN
LUT_SIZE = 4096


def gauss_table() -> torch.Tensor:
    """The 4096-entry inverse normal CDF at the bin centres, fp32 [4096] on the host (computed in fp64)."""
    nd = NormalDist()
    return torch.from_numpy(np.array([nd.inv_cdf((i + 0.5) / LUT_SIZE) for i in range(LUT_SIZE)], np.float64).astype(np.float32))


def threshold_u32(p: float) -> int:
    """A probability in [0, 1] as the kernel's threshold on a 32-bit word: 0 never, 0xFFFFFFFF always."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise _lib.GennbvHipError(f"DepthSensor: a probability must lie in [0, 1], got {p}")
    return min(int(p * 4294967296.0), 0xFFFFFFFF)


class DepthSensor:
    def __init__(self, n: int, h: int, w: int, *, seed: int = 0, min_range_m: float, max_range_m: float, edge_radius: int = 0,
                 edge_abs_m: float = 0.0, edge_rel: float = 0.0, edge_drop: float = 0.0, drop: float = 0.0,
                 sigma: Sequence[float] = (0, 0, 0), quant: float = 0.0, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("DepthSensor runs on the GPU only (no CPU fallback)")
        self.lib = _lib.load()
        self.num_envs, self.h, self.w = int(n), int(h), int(w)
        if len(sigma) != 3:
            raise _lib.GennbvHipError("DepthSensor: sigma is (s0, s1, s2) of s0 + s1 t + s2 t^2")
        self.frame = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        noisy = any(float(s) != 0.0 for s in sigma)
        self.gauss_lut = gauss_table().to(self.device) if noisy else None
        a = self.args = _lib.GnbvDepthSensor()
        a.n, a.h, a.w = self.num_envs, self.h, self.w
        a.frame = self.frame.data_ptr()
        a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        a.min_range, a.max_range = float(min_range_m), float(max_range_m)
        a.edge_radius, a.edge_abs, a.edge_rel = int(edge_radius), float(edge_abs_m), float(edge_rel)
        a.edge_drop, a.drop = threshold_u32(edge_drop), threshold_u32(drop)
        a.sigma0, a.sigma1, a.sigma2 = (float(s) for s in sigma)
        a.gauss_lut = _lib.ptr(self.gauss_lut)
        a.quant = float(quant)
        # every effect off: a frame inside the range limits comes back bit for bit
        self.is_identity = not noisy and a.quant == 0.0 and a.drop == 0 and (a.edge_radius == 0 or a.edge_drop == 0)

    def _frame_arg(self, t: torch.Tensor, name: str):
        _lib.require_cuda(t)
        n, h, w = self.num_envs, self.h, self.w
        ok = t.dtype == torch.float32 and tuple(t.shape) == (n, h, w) and (w == 1 or t.stride(2) == 1) and (h == 1 or t.stride(1) == w)
        stride = h * w if n == 1 else t.stride(0)  # (a dimension of size 1 may carry any stride)
        if not ok or stride < h * w:
            raise _lib.GennbvHipError(f"DepthSensor: {name} must be f32 [{n}, {h}, {w}] with contiguous rows, got {t.dtype} "
                                      f"{tuple(t.shape)} strides {tuple(t.stride())}")
        return t.data_ptr(), stride

    def __call__(self, depth_raw: torch.Tensor, seg_raw: torch.Tensor, out: Optional[tuple] = None):
        """depth_raw, seg_raw f32 [n, h, w] (env stride >= h w) -> (depth, seg), written to `out` = (depth, seg) where given
        (the same layout rules; no overlap with the inputs).  Then frame += 1."""
        if out is None:
            out = tuple(torch.empty(self.num_envs, self.h, self.w, dtype=torch.float32, device=self.device) for _ in range(2))
        a = self.args
        a.depth_in, si = self._frame_arg(depth_raw, "depth_raw")
        a.seg_in, si2 = self._frame_arg(seg_raw, "seg_raw")
        a.depth_out, so = self._frame_arg(out[0], "out[0]")
        a.seg_out, so2 = self._frame_arg(out[1], "out[1]")
        if si != si2 or so != so2:
            raise _lib.GennbvHipError("DepthSensor: depth and seg of a frame share one env stride")
        a.in_env_stride, a.out_env_stride = si, so
        _lib.check(self.lib.gnbv_depth_sensor(C.byref(a), _lib.stream_ptr(self.device)), "gnbv_depth_sensor")
        self.frame += 1
        return out[0], out[1]

"""RenderFeed: the closed-loop camera of ReplayFeedEnv.

ReplayFeed hands out recorded frames whatever the policy did.  RenderFeed renders every env from the pose step()
has just computed from the actions (gnbv_render_depth, csrc/render.hip) and hands out the same four tensors in the
same order as `ReplayFeed.next()`:

    depth_raw [N,H,W] f32   Isaac convention: -t, -inf on a miss
    seg_raw   [N,H,W] f32   255 on an object, 0 on ground / miss
    rgba      [N,H,W,4] u8  synthetic.render_depth's shading of the hit object, or None (with_rgba=False)
    c2w       [N,4,4] f32   the camera the frame was rendered with; the voxel update back-projects with it

The buffers are preallocated and reused: a frame is valid until the next `render()`.  `.last` is the last frame.

With `sensor=` (ops/depth_sensor.py DepthSensor) the renderer writes `ideal_depth_raw` / `ideal_seg_raw` and the sensor writes
`depth_raw` / `seg_raw` from them: `.last` and the return value carry the MEASURED pair, so the env, the voxel update, CarvedMap
and the scan sets see what the sensor saw.  Without one the feed is what it was: no extra buffers, no extra launch.
Roll is ignored by the renderer (as by synthetic.camera_to_world), so a task whose roll lattice is not fixed is refused.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from . import synthetic as S
from .config import TaskConfig
from .mesh_scene import MeshScene


class RenderFeed:
    closed_loop = True  # ReplayFeedEnv: poses first, then render(poses)

    def __init__(self, mesh: MeshScene, cfg: TaskConfig, inv_intrinsics: Optional[torch.Tensor] = None, with_rgba: bool = True,
                 sensor=None):
        if int(cfg.clip_pose_idx_up[3]) != 0:
            raise _lib.GennbvHipError("RenderFeed ignores roll: the roll lattice must be fixed (clip_pose_idx_up[3] == 0)")
        self.lib = _lib.load()
        self.mesh = mesh
        self.device = mesh.device
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("RenderFeed renders on the GPU only (no CPU fallback): build the MeshScene on a cuda device")
        n, h, w = mesh.num_envs, cfg.camera_height, cfg.camera_width
        self.num_envs, self.h, self.w = n, h, w
        # the updater's inverse intrinsics (ReplayFeedEnv uses the same default): ray parameter == depth
        kinv = S.inverse_intrinsics(h, w, cfg.horizontal_fov) if inv_intrinsics is None else inv_intrinsics
        self.inv_intri_host = kinv.detach().to("cpu", torch.float32).contiguous()
        assert self.inv_intri_host.shape == (3, 3)
        dev = self.device
        self.depth_raw = torch.empty(n, h, w, dtype=torch.float32, device=dev)
        self.seg_raw = torch.empty(n, h, w, dtype=torch.float32, device=dev)
        self.rgba = torch.empty(n, h, w, 4, dtype=torch.uint8, device=dev) if with_rgba else None
        self.c2w = torch.empty(n, 4, 4, dtype=torch.float32, device=dev)
        self.sensor = sensor
        self.ideal_depth_raw = self.ideal_seg_raw = None
        if sensor is not None:
            if (sensor.num_envs, sensor.h, sensor.w) != (n, h, w):
                raise _lib.GennbvHipError(f"RenderFeed: the sensor was built for {(sensor.num_envs, sensor.h, sensor.w)}, "
                                          f"the feed renders {(n, h, w)}")
            self.ideal_depth_raw, self.ideal_seg_raw = torch.empty_like(self.depth_raw), torch.empty_like(self.seg_raw)
        self._scene = mesh.c_struct()
        self.last = None

    def render(self, poses: torch.Tensor):
        """Frames of every env seen from poses [N,>=6] f32 (x, y, z, roll, pitch, yaw), env-local."""
        _lib.require_cuda(poses)
        assert poses.dtype == torch.float32 and poses.shape[0] == self.num_envs and poses.shape[1] >= 6 and poses.stride(1) == 1
        depth, seg = (self.depth_raw, self.seg_raw) if self.sensor is None else (self.ideal_depth_raw, self.ideal_seg_raw)
        _lib.check(self.lib.gnbv_render_depth(C.byref(self._scene), poses.data_ptr(), poses.stride(0), self.inv_intri_host.data_ptr(),
                                              self.h, self.w, self.c2w.data_ptr(), depth.data_ptr(), seg.data_ptr(),
                                              _lib.ptr(self.rgba), _lib.stream_ptr(self.device)), "gnbv_render_depth")
        if self.sensor is not None:
            self.sensor(depth, seg, out=(self.depth_raw, self.seg_raw))
        self.last = (self.depth_raw, self.seg_raw, self.rgba, self.c2w)
        return self.last

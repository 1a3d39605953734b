"""ReplayFeedEnv: Env_Train_GenNBV with Isaac Gym cut at the observation boundary.

The reference env (gennbv/env/env_train_gennbv.py + env_train_base.py) renders
depth / segmentation / RGB with Isaac Gym and then runs the state encoding.  Here a
recorded or synthetic feed supplies exactly the tensors the simulator would
(`depth_raw`, `seg_raw`, `rgba`, camera view matrix), everything after that
boundary runs on gfx950 kernels through the C-ABI, and the env speaks the
protocol the reference algorithm expects from `EnvWrapperGenNBVTrain`
(gennbv/wrapper/env_wrapper_gennbv_train.py:90-133):

    num_envs, device, observation_space (flat Box (D_obs,)), action_space
    (MultiDiscrete [81,81,51,1,13,13]), episode_length_buf (int64 [N], writable),
    max_episode_length, seed(), close(),
    reset() -> obs f32 [N, D_obs]
    step(actions int64 [N,6]) -> (obs, rewards f32 [N], dones bool [N], infos)
        infos["time_outs"] bool [N], infos["episode"] dict

The flat observation is written in place by the kernels in the wrapper's key
order [state | grid | state_rgb]; `step(..., obs_out=rows)` lets the rollout
buffer hand its own storage to the env (no assemble + copy pass).

`collision=CollisionBody(...)` (env/collision.py) adds the reference's collision
termination: every step and reset tests the body at the step's poses against the
mesh's solids (MeshScene.collide) into `collision_buf` [N] u8, and an env with
contact resets with the termination reward (gnbv_env_post_step_contacts).  The
mesh is `collision_mesh`, by default the RenderFeed's own.  With `collision.sweep`
the straight flight from the previous pose to the step's pose is tested too
(MeshScene.sweep, csrc/sweep.hip): its path bits are ORed into `collision_buf`,
except on the first step of an episode, whose pose is set, not flown to.

`flight=FlightField(...)` (ops/flight_field.py; needs `collision.sweep`) lets the drone fly round what blocks the straight
line: a step whose straight flight is blocked but whose detour over the flight lattice from the previous pose is finite has
its PATH / PATH_GROUND bits cleared before the post-step kernel (pose bits are untouched), and `flight_length` [N] f32 counts
the metres flown in the episode: the straight distance where the straight flight was free, the detour length otherwise
(nothing for a flight with no route: it ends the episode), reset to 0 by the step that sets an episode's first pose -- so
after the step that ends an episode it still holds that episode's length.  The field is computed once per step from the
poses the env has just arrived at and kept in `env.flight`: the next step's check and the planners' queries both read it.

`flight=BeliefFlightField(...)` (a field whose `belief` is true) is the pilot that knows only its own map: the drone flies the
route that the field -- computed last step from the map scanned so far -- holds to the step's pose, and the true mesh judges
what was flown.  One path launch (buffer length max(2 (nx + ny + nz), 8); a route that does not fit counts as none and is
counted in `route_overflow`); where a route exists its legs previous pose -> nodes -> new pose, otherwise the straight flight,
go through ONE sweep_candidates call and their codes are ORed into `path_code` and, in full, into `collision_buf`: nothing is
dropped.  `flight_length` adds the route's length where there is one and the straight distance otherwise.  After the voxel
update the field is refreshed from the tri-class grid the step has just written (grid_i8_out where given, else the observation's
grid slice) and updated from the poses arrived at.
With `flight.shortcut` the pilot also asks its map about straight legs (BeliefFlightField.sweep, csrc/sweepmap.hip, over the
snapshot of the map it had): it flies straight from the previous pose to the farthest waypoint of the route -- the new pose
included -- that the map shows in the clear, and the rest of the route from there.  The flown legs alone go to the truth,
`flight_length` adds their Euclidean lengths, `routed` is true where a route node was flown, and `skipped` [N] int64 is the number
of waypoints the straight first leg passed over (0: the route as it was; the route's node count: straight to the new pose).
With a field that puts a price on unknown space (`flight.costly_map`, BeliefFlightField(unknown="costly")) the route is the
penalised field's; `flight_length` still counts metres -- the Euclidean lengths of the flown legs, never `flight.cost`, which
holds penalties -- and `route_unknown` [N] int64 is the number of costly nodes entered on the route flown this step: the flown
route nodes but the first, the node the drone already sat at (0 on an episode's first pose and without a route; None for
other fields).

`carve=CarvedMap(...)` (ops/carve.py; closed-loop feeds only: an open-loop feed's camera is not the pose's matrix) keeps a
second map beside the observation: after the voxel update of each step the env calls carve.update(the tri just written, the
frame's raw depth, self.poses, self.reset_mask), `env.map_tri` is carve.map_i8 (None without carve), and a BeliefFlightField is
refreshed from it instead of the observation's grid.  Nothing else in the step changes: observation rows, rewards, dones and
the update's outputs are byte-identical to the same env without `carve`.  The planners of eval/baselines.py that score or route
on the tri-class grid read `env.map_tri` (planning_grid).
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .. import _lib
from ..spaces import Box, MultiDiscrete
from .config import TaskConfig
from .state_encoding import OccupancyGridUpdater
from . import synthetic as S


@dataclass
class ReplayFeed:
    """A pool of recorded frames, resident in HBM: frame f of env e."""
    depth_raw: torch.Tensor  # [F,N,H,W] f32, Isaac convention (negative metres, -inf = nothing)
    seg_raw: torch.Tensor  # [F,N,H,W] f32
    rgba: Optional[torch.Tensor]  # [F,N,H,W,4] u8 or None (gray frames stay zero)
    c2w: torch.Tensor  # [F,N,4,4] f32: inv(view^T) @ blender2opencv, translation - env_origins
    cursor: int = 0

    @property
    def num_frames(self):
        return self.depth_raw.shape[0]

    def next(self):
        f = self.cursor % self.num_frames
        self.cursor += 1
        return (self.depth_raw[f], self.seg_raw[f], None if self.rgba is None else self.rgba[f], self.c2w[f])

    @staticmethod
    def from_views(depth_raw, seg_raw, rgba, view, env_origins):
        """Host plumbing of back_projection_fg (env_train_gennbv.py:512-514) done once for the
        whole recording: c2w = inv(view^T) @ blender2opencv, translation minus env_origins."""
        f, n = view.shape[0], view.shape[1]
        c2w = S.c2w_from_view(view.reshape(f * n, 4, 4), env_origins.repeat(f, 1)).reshape(f, n, 4, 4)
        return ReplayFeed(depth_raw.contiguous(), seg_raw.contiguous(), None if rgba is None else rgba.contiguous(),
                          c2w.contiguous())

    @staticmethod
    def from_file(path: str, device, first: int = 0, count: Optional[int] = None):
        """Frames of a recorded-feed container (env/feed_file.py), decoded on `device`."""
        from . import feed_file
        return feed_file.load_feed(feed_file.FeedFile(path), device, first, count)

    @staticmethod
    def synthetic(scene: S.Scene, cfg: TaskConfig, num_frames: int, seed: int = 1, with_rgba: bool = True):
        frames = S.make_frames(scene, cfg, num_frames, seed=seed, with_rgba=with_rgba)
        return ReplayFeed.from_views(torch.stack([f.depth_raw for f in frames]), torch.stack([f.seg_raw for f in frames]),
                                     torch.stack([f.rgba for f in frames]) if with_rgba else None,
                                     torch.stack([f.view for f in frames]), scene.env_origins)


class ReplayFeedEnv:
    @classmethod
    def from_file(cls, cfg: TaskConfig, path: str, device="cuda:0", max_episode_length: Optional[int] = None):
        """Env over a recorded-feed container: scene block + frames (env/feed_file.py)."""
        import dataclasses

        from . import feed_file
        ff = feed_file.FeedFile(path)
        cfg = dataclasses.replace(cfg, camera_height=ff.height, camera_width=ff.width, grid_size=ff.grid_size)
        # the recording's own inverse intrinsics (a different FOV than cfg's must not be back-projected with cfg's K)
        kinv = torch.from_numpy(np.array(ff.scene("inv_intrinsics"), dtype=np.float32))
        return cls(cfg, feed_file.load_scene(ff, "cpu"), feed_file.load_feed(ff, device), device, max_episode_length,
                   inv_intrinsics=kinv)

    def __init__(self, cfg: TaskConfig, scene: S.Scene, feed, device="cuda:0",
                 max_episode_length: Optional[int] = None, inv_intrinsics: Optional[torch.Tensor] = None,
                 collision=None, collision_mesh=None, flight=None, carve=None):
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("ReplayFeedEnv runs on the GPU only (no CPU fallback)")
        self.feed = feed
        # a RenderFeed (env/render_feed.py) renders each frame from the poses of the step: actions -> poses -> render ->
        # observation -> voxel update, in place of the recorded frame pool
        self.closed_loop = bool(getattr(feed, "closed_loop", False))
        n = scene.grid_gt.shape[0]
        self.num_envs = n
        # free space along every camera ray (module docstring): None keeps every launch of the env as it was
        if carve is not None:
            if not self.closed_loop:
                raise _lib.GennbvHipError("carve needs a closed-loop feed: an open-loop feed's camera is not the pose's matrix")
            if carve.num_envs != n or int(carve.g) != int(cfg.grid_size) or (carve.h, carve.w) != (cfg.camera_height, cfg.camera_width):
                raise ValueError(f"carve is built for {carve.num_envs} envs, a {carve.g}^3 grid and a {carve.h} x {carve.w} camera; the "
                                 f"env has {n}, {cfg.grid_size}^3 and {cfg.camera_height} x {cfg.camera_width}")
        self.carve = carve
        self.map_tri = carve.map_i8 if carve is not None else None
        # collision termination (check_termination's collision_buf): None keeps the replay feed's "no contacts"
        self.collision = collision
        self.collision_mesh = None
        self.collision_buf = None
        if collision is not None:
            mesh = collision_mesh if collision_mesh is not None else getattr(feed, "mesh", None)
            if mesh is None:
                raise _lib.GennbvHipError("collision termination needs a mesh: pass collision_mesh (an open-loop feed has none)")
            if mesh.num_envs != n:
                raise ValueError(f"collision_mesh must hold {n} envs, got {mesh.num_envs}")
            mesh.objects()  # the per-object index, built once
            self.collision_mesh = mesh
            self.collision_buf = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._sweep = collision is not None and bool(getattr(collision, "sweep", False))
        self._prev_poses = None  # the poses before the step's head overwrites them (collision.sweep only)
        # detours round a blocked straight flight (module docstring): None keeps every launch of the env as it was
        if flight is not None:
            if not self._sweep:
                raise ValueError("flight needs collision=CollisionBody(sweep=True): without the swept path there is nothing to fly round")
            if flight.num_envs != n:
                raise ValueError(f"flight must hold {n} envs, got {flight.num_envs}")
        self.flight = flight
        self.flight_length = torch.zeros(n, dtype=torch.float32, device=self.device) if flight is not None else None
        self.path_code = torch.zeros(n, dtype=torch.uint8, device=self.device) if flight is not None else None
        self._belief = flight is not None and bool(getattr(flight, "belief", False))
        self.route_overflow = self.routed = None
        self.skipped = None  # with flight.shortcut: the waypoints the last step's straight first leg skipped, int64 [N]
        self.route_unknown = None  # with a price on unknown space: the costly nodes entered on the last step's route, int64 [N]
        self._cautious = self._belief and getattr(flight, "costly_map", None) is not None
        if self._belief:
            if int(flight.grid_size) != int(cfg.grid_size):
                raise ValueError(f"flight is built for a {flight.grid_size}^3 grid, the env's is {cfg.grid_size}^3")
            nx, ny, nz = flight.lattice.dims
            self._route_len = length = max(2 * (nx + ny + nz), 8)
            self._route_nodes = torch.full((n, length), -1, dtype=torch.int32, device=self.device)
            self._route_count = torch.zeros(n, dtype=torch.int32, device=self.device)
            self._route_codes = torch.zeros(n, length + 1, dtype=torch.uint8, device=self.device)
            self._node_pos = torch.as_tensor(flight.lattice.node_positions(), device=self.device).to(torch.float32)
            self.route_overflow = torch.zeros((), dtype=torch.int64, device=self.device)  # routes longer than the buffer, so far
            self.routed = torch.zeros(n, dtype=torch.bool, device=self.device)  # the last step flew a route of the field
            self.route_unknown = torch.zeros(n, dtype=torch.int64, device=self.device) if self._cautious else None
            if getattr(flight, "shortcut", False):
                self._map_codes = torch.zeros(n, length + 1, dtype=torch.uint8, device=self.device)
                self.skipped = torch.zeros(n, dtype=torch.int64, device=self.device)
        self.grid_size = cfg.grid_size
        self.max_episode_length = int(cfg.max_episode_length if max_episode_length is None else max_episode_length)
        self.max_episode_length_s = cfg.episode_length_s
        dev = self.device
        self.updater = OccupancyGridUpdater(n, cfg.grid_size, cfg.camera_height, cfg.camera_width,
                                            S.inverse_intrinsics(cfg.camera_height, cfg.camera_width, cfg.horizontal_fov)
                                            if inv_intrinsics is None else inv_intrinsics,
                                            scene.range_gt, scene.voxel_size, scene.grid_gt, dev, cfg.depth_sense_dist,
                                            max_steps_between_resets=self.max_episode_length + 1)  # (+1: the reset observation)
        self.num_valid_voxel_gt = scene.num_valid_voxel_gt.to(dev, torch.float32).contiguous()
        # spaces (update_observation_space :459-492 flattened by the wrapper :59-88)
        self.action_space = MultiDiscrete(cfg.action_nvec)
        self.observation_space = Box(-np.inf, np.inf, shape=(cfg.obs_dim,), dtype=np.float32)
        # lattice constants for the kernels
        lat = _lib.GnbvLattice()
        for i in range(6):
            lat.clip_low[i], lat.clip_up[i] = cfg.clip_pose_idx_low[i], cfg.clip_pose_idx_up[i]
            lat.init_action[i] = cfg.init_action[i]
            lat.action_unit[i] = float(np.float32(cfg.action_unit[i]))
            lat.pose_low[i] = float(np.float32(cfg.clip_pose_low[i]))
            lat.init_pose[i] = float(np.float32(cfg.init_pose_buf[i]))
        self._lat = lat
        # state tensors
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        self.episode_length_buf = z(n, dt=torch.int64)
        self.actions = torch.tensor(cfg.init_action, dtype=torch.int64, device=dev).repeat(n, 1)
        self.poses = z(n, 6)
        self.pose_hist = torch.tensor(cfg.init_pose_buf, dtype=torch.float32, device=dev).repeat(n, cfg.stack, 1)
        self.gray_prev = z(n, cfg.rgb_h * cfg.rgb_w)
        self.prev_ratio = z(n)
        self.rew_buf = z(n)
        self.reset_buf = z(n, dt=torch.uint8)
        # `flag_views` (off by default; collect_rollouts of PPO_Grid_Obs turns it on): step() hands out `dones` and infos["time_outs"] as
        # bool VIEWS of the kernels' 0 / 1 bytes instead of `.bool()` copies (two element-wise launches per env step).  `dones` of step t is
        # still needed after step t + 1 has run (it is step t + 1's episode_starts): two buffers take turns.  time_outs is read inside the
        # step that produced it (the time-out bootstrap) and is STATEFUL on the device (the reference only refreshes it on steps with a
        # reset): one buffer, and a reader that keeps infos["time_outs"] across env steps must copy it.
        self.flag_views = False
        self.fused_observe = True  # pre-step + both observation slices as one launch (False: the three separate entry points, kept covered by tests/test_envstep_gpu.py)
        self._reset_bufs = (self.reset_buf, z(n, dt=torch.uint8))
        self._reset_turn = 0
        self.reset_mask = torch.ones(n, dtype=torch.uint8, device=dev)
        self.time_out_buf = z(n, dt=torch.uint8)
        self.extras_time_outs = z(n, dt=torch.uint8)
        self.coverage_ratio = z(n)
        self.episode_sums = z(3, n)
        self.cur_reward_sum = z(n)
        self.cur_episode_length = z(n)
        self.ring_len = 100
        self.ring_reward = z(self.ring_len)
        self.ring_length = z(self.ring_len)
        self.ring_state = z(1, dt=torch.int64)
        self._zero_rgba = None
        self._obs = torch.zeros(n, cfg.obs_dim, dtype=torch.float32, device=dev)
        p = _lib.GnbvEnvPost()
        p.n, p.only_positive, p.max_episode_length = n, int(cfg.only_positive_rewards), self.max_episode_length
        # a Python-float scale multiplying an fp32 tensor is rounded to fp32 first
        p.scale_cov = float(np.float32(cfg.scale_surface_coverage * cfg.dt))
        p.scale_short = float(np.float32(cfg.scale_short_path * cfg.dt))
        p.scale_term = float(np.float32(cfg.scale_termination * cfg.dt))
        p.coverage_threshold = float(np.float32(cfg.coverage_threshold))
        p.coverage_count = self.updater.coverage_count.data_ptr()
        p.num_valid_voxel_gt = self.num_valid_voxel_gt.data_ptr()
        p.prev_ratio = self.prev_ratio.data_ptr()
        p.rewards, p.dones = self.rew_buf.data_ptr(), self.reset_buf.data_ptr()
        p.reset_mask, p.step_time_out = self.reset_mask.data_ptr(), self.time_out_buf.data_ptr()
        p.extras_time_outs, p.coverage_ratio = self.extras_time_outs.data_ptr(), self.coverage_ratio.data_ptr()
        p.episode_sums, p.cur_reward_sum = self.episode_sums.data_ptr(), self.cur_reward_sum.data_ptr()
        p.cur_episode_length = self.cur_episode_length.data_ptr()
        p.ring_reward, p.ring_length = self.ring_reward.data_ptr(), self.ring_length.data_ptr()
        p.ring_state, p.ring_len = self.ring_state.data_ptr(), self.ring_len
        # extras["episode"] snapshots: k_env_post_step writes this step's (mean reward, mean length) into slot
        # step % H; the dict handed out with the step reads its own slot on demand (no per-step host sync)
        self._ep_hist = 1024
        self.episode_info_hist = z(self._ep_hist, 6, dt=torch.float64)  # per step: generation, 2 deque means, 3 rew_<name>
        self.episode_state = z(4, dt=torch.float64)
        p.episode_state, p.max_episode_length_s = self.episode_state.data_ptr(), float(np.float32(self.max_episode_length_s))
        self._ep_step = 0
        self._ep_cache = (-1, None)
        self._ep_live = collections.deque()
        self._post = p
        self.extras = {}

    # reference attribute names for the grids
    @property
    def prob_grid(self):
        return self.updater.prob_grid

    @property
    def scanned_gt_grid(self):
        return self.updater.scanned_gt_grid

    @property
    def grid_gt(self):
        return self.updater.grid_gt

    def seed(self, seed=None):
        return [seed]

    def close(self):
        pass

    # ------------------------------------------------------------------------
    def _observe_and_finish(self, actions_in: torch.Tensor, obs_out: Optional[torch.Tensor], grid_i8_out: Optional[torch.Tensor] = None):
        cfg, n, lib = self.cfg, self.num_envs, self.lib
        st = _lib.stream_ptr(self.device)
        obs = self._obs if obs_out is None else obs_out
        # compact rows [state | state_rgb]: the grid goes to `grid_i8_out` only (coded update)
        compact = obs.shape == (n, cfg.obs_dim - cfg.grid_dim)
        if compact and (grid_i8_out is None or not self.updater.coded):
            raise _lib.GennbvHipError("compact observation rows need grid_i8_out and the coded grid update")
        assert (compact or obs.shape == (n, cfg.obs_dim)) and obs.dtype == torch.float32 and obs.stride(1) == 1
        stride = obs.stride(0)
        closed_loop = self.closed_loop
        if not closed_loop:
            depth_raw, seg_raw, rgba, c2w = self.feed.next()
        # step(): clip, forced init action, poses; episode_length_buf += 1
        self._post.episode_length_buf = self.episode_length_buf.data_ptr()  # the algorithm may have replaced the tensor
        rgb_off = cfg.state_dim + (0 if compact else cfg.grid_dim)
        if self._sweep:
            if self._prev_poses is None:
                self._prev_poses = torch.empty_like(self.poses)
            self._prev_poses.copy_(self.poses)
        if closed_loop:
            # closed loop (RenderFeed): the frame is rendered from the poses this step computes, so the fused
            # gnbv_env_observe (poses and the rgba read in one launch) cannot be used
            self._pre_step(actions_in, st)
            if self.collision is not None:  # step order: pre-step -> collide -> render -> ... -> post-step with contacts
                self._collide_step()
            depth_raw, seg_raw, rgba, c2w = self.feed.render(self.poses)
            self._observe_slices(obs, stride, self._rgba_or_zero(rgba), rgb_off, st)
        elif self.fused_observe and getattr(lib, "gnbv_env_observe", None) is not None:
            rgba = self._rgba_or_zero(rgba)
            # round 5: the three launches below as one (same arithmetic, bit-identical: tests/test_envstep_gpu.py)
            _lib.check(lib.gnbv_env_observe(actions_in.data_ptr(), C.byref(self._lat), self.episode_length_buf.data_ptr(), n, self.actions.data_ptr(),
                                            self.poses.data_ptr(), self.pose_hist.data_ptr(), self.reset_mask.data_ptr(), cfg.stack, obs.data_ptr(), stride,
                                            rgba.data_ptr(), self.gray_prev.data_ptr(), cfg.camera_height, cfg.camera_width, cfg.rgb_h, cfg.rgb_w,
                                            obs.data_ptr() + 4 * rgb_off, st), "gnbv_env_observe")
        else:
            self._observe_three_launches(actions_in, obs, stride, self._rgba_or_zero(rgba), rgb_off, st)
        if self.collision is not None and not closed_loop:
            self._collide_step()
        # obs["grid"]: tri-class grid straight into the observation rows
        if compact:
            self.updater.update(depth_raw, seg_raw, c2w, self.poses, reset_mask=self.reset_mask, tri_i8_out=grid_i8_out, fp32_out=False)
        else:
            self.updater.update(depth_raw, seg_raw, c2w, self.poses, reset_mask=self.reset_mask,
                                tri_out=obs[:, cfg.state_dim:], tri_row_stride=stride,
                                tri_i8_out=grid_i8_out if self.updater.coded else None)
        wrote_i8 = grid_i8_out is not None and (compact or self.updater.coded)
        tri_written = grid_i8_out if wrote_i8 else obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]
        if self.carve is not None:  # the observation's grid plus the free space along every ray of the frame it was written from
            self.carve.update(tri_written, depth_raw, self.poses, self.reset_mask)
        if self._belief:  # what the pilot knows next step: the map just written, from the poses just arrived at
            self.flight.refresh(self.map_tri if self.carve is not None else tri_written)
            self.flight.update(self.poses)
        # rewards / termination / reset bookkeeping
        self._ep_step += 1
        self._post.episode_info = self.episode_info_hist[self._ep_step % self._ep_hist].data_ptr()
        if self.collision is not None:
            _lib.check(lib.gnbv_env_post_step_contacts(C.byref(self._post), self.collision_buf.data_ptr(), st), "gnbv_env_post_step_contacts")
        else:
            _lib.check(lib.gnbv_env_post_step(C.byref(self._post), st), "gnbv_env_post_step")
        return obs

    def _collide_step(self):
        """collision_buf = the body at the step's poses, and with `collision.sweep` | the flight from the previous poses to
        them (episode_length_buf <= 1 after the step's head: the first pose of an episode, not flown to)."""
        self.collision_mesh.collide(self.poses, self.collision, out=self.collision_buf)
        if self._belief:
            self._fly_belief_step()
        elif self.flight is not None:
            self._fly_step()
        elif self._sweep:
            self.collision_mesh.sweep_candidates(self._prev_poses, self.poses.unsqueeze(1), self.collision, self.episode_length_buf,
                                                 out=self.collision_buf.unsqueeze(1), accumulate=True)

    def _fly_step(self):
        """The sweep of _collide_step with detours: the path bits of a blocked straight flight are dropped where `flight` (the
        field from the previous poses) holds a finite route to the step's poses; flight_length follows; then the one field
        launch of the step, from the poses just arrived at."""
        fl, poses, prev = self.flight, self.poses, self._prev_poses
        code = self.collision_mesh.sweep_candidates(prev, poses.unsqueeze(1), self.collision, self.episode_length_buf,
                                                    out=self.path_code.unsqueeze(1))[:, 0]
        detour = fl.cost(poses.unsqueeze(1))[:, 0]
        blocked, routed = code != 0, torch.isfinite(detour)
        self.collision_buf |= torch.where(blocked & routed, torch.zeros_like(code), code)
        straight = (poses[:, :3] - prev[:, :3]).norm(dim=-1)
        flown = torch.where(blocked, torch.where(routed, detour, torch.zeros_like(detour)), straight)
        first = self.episode_length_buf <= 1  # after the step's head: the pose was set, not flown to
        self.flight_length.copy_(torch.where(first, torch.zeros_like(flown), self.flight_length + flown))
        fl.update(poses)

    def _route_waypoints(self):
        """The waypoints of the belief pilot's route [N, L + 2, 3] (previous pose, the route's nodes, then the new pose up to the
        end) and the number of nodes [N] int64 (0: no route): `flight` still holds the field from the previous poses over the
        previous map."""
        fl, poses, prev = self.flight, self.poses, self._prev_poses
        n, length = self.num_envs, self._route_len
        nodes, count = self._route_nodes, self._route_count
        fl.path_into(poses, nodes, count)
        self.route_overflow += (count < 0).sum()
        cnt = count.clamp(min=0).long()
        j = torch.arange(length, device=self.device)[None]
        back = (cnt[:, None] - 1 - j).clamp(min=0)  # nodes run target -> source: waypoint 1 + j is node count - 1 - j
        ids = nodes.long().gather(1, back).clamp(min=0)
        new = poses[:, None, :3]
        way = torch.empty(n, length + 2, 3, dtype=torch.float32, device=self.device)
        way[:, 0] = prev[:, :3]
        way[:, 1:length + 1] = torch.where((j < cnt[:, None])[..., None], self._node_pos[ids], new)  # past the route: the new pose
        way[:, length + 1] = poses[:, :3]
        self._route_ids = torch.where(j < cnt[:, None], ids, torch.full_like(ids, -1))  # the node of waypoint 1 + j; -1 past the route
        return way, cnt

    def _fly_belief_step(self):
        """The sweep of _collide_step for a pilot that plans on its own map (module docstring): `flight` still holds the field
        from the previous poses over the previous map.  Waypoints: previous pose, the route's nodes, new pose; an env without a
        route has the one leg previous pose -> new pose, the straight flight.  The truth judges every leg."""
        if self.flight.shortcut:
            return self._fly_belief_shortcut_step()
        fl, poses, prev = self.flight, self.poses, self._prev_poses
        length = self._route_len
        way, cnt = self._route_waypoints()
        routed = self._route_count > 0
        codes = self.collision_mesh.sweep_candidates(way[:, :-1].contiguous(), way[:, 1:].contiguous(), self.collision,
                                                     self.episode_length_buf, out=self._route_codes)
        legs = torch.arange(length + 1, device=self.device)[None] <= cnt[:, None]  # count + 1 legs; 1 without a route
        codes = torch.where(legs, codes, torch.zeros_like(codes))
        code = ((codes & 8) != 0).any(dim=1).to(torch.uint8) * 8 | ((codes & 16) != 0).any(dim=1).to(torch.uint8) * 16
        self.path_code.copy_(code)
        self.collision_buf |= code
        first = self.episode_length_buf <= 1  # after the step's head: the pose was set, not flown to
        if self._cautious:  # the field holds penalties: the metres are the legs' own (an env without a route has the one straight leg)
            lens = (way[:, 1:] - way[:, :-1]).norm(dim=-1)
            flown = torch.where(legs, lens, torch.zeros_like(lens)).sum(dim=1)
            self._count_unknown(torch.ones_like(cnt), first)
        else:
            straight = (poses[:, :3] - prev[:, :3]).norm(dim=-1)
            flown = torch.where(routed, fl.cost(poses.unsqueeze(1))[:, 0], straight)
        self.flight_length.copy_(torch.where(first, torch.zeros_like(flown), self.flight_length + flown))
        self.routed.copy_(routed & ~first)

    def _count_unknown(self, jstar, first):
        """route_unknown: the costly nodes among the flown route nodes, waypoints max(j*, 2) .. count (waypoint 1 is the node the
        drone sat at: not entered)."""
        wp = torch.arange(1, self._route_len + 1, device=self.device)[None]
        entered = self.flight.costly_at(self._route_ids) & (wp >= jstar[:, None].clamp(min=2))
        self.route_unknown.copy_(torch.where(first, torch.zeros_like(jstar), entered.sum(dim=1)))

    def _fly_belief_shortcut_step(self):
        """_fly_belief_step with the straight shortcut judged on the map (`flight.shortcut`): of the legs w_0 -> w_j, j = 1 .. c + 1
        (c route nodes, w_{c+1} the new pose), one gnbv_sweep_tri launch over the snapshot of the map the pilot had; j* is the
        farthest one the map shows in the clear (1 if none).  The drone flies w_0 -> w_j* -> w_{j*+1} -> ... -> new pose, exactly
        those legs are judged by the truth (the one sweep_candidates call, the skipped ones masked), `flight_length` adds their
        Euclidean lengths, `routed` says whether a route node was flown, `skipped` = j* - 1."""
        fl = self.flight
        n, length = self.num_envs, self._route_len
        way, cnt = self._route_waypoints()
        ahead = way[:, 1:].contiguous()
        if fl.has_map:
            map_codes = fl.sweep(self._prev_poses, ahead, out=self._map_codes)
        else:  # the env's very first step, the reset: no map yet, and every pose is set, not flown to
            map_codes = self._map_codes.zero_()
        jj = torch.arange(1, length + 2, device=self.device)[None]
        clear = (map_codes == 0) & (jj <= cnt[:, None] + 1)
        jstar = torch.where(clear, jj, torch.zeros_like(jj)).max(dim=1).values.clamp(min=1)
        ahead[:, 0] = way[torch.arange(n, device=self.device), jstar]  # the first leg flown: w_0 -> w_j*
        start = way[:, :-1].contiguous()
        codes = self.collision_mesh.sweep_candidates(start, ahead, self.collision, self.episode_length_buf, out=self._route_codes)
        leg = jj - 1  # leg i > 0 is w_i -> w_{i+1}
        legs = (leg == 0) | ((leg >= jstar[:, None]) & (leg <= cnt[:, None]))
        codes = torch.where(legs, codes, torch.zeros_like(codes))
        code = ((codes & 8) != 0).any(dim=1).to(torch.uint8) * 8 | ((codes & 16) != 0).any(dim=1).to(torch.uint8) * 16
        self.path_code.copy_(code)
        self.collision_buf |= code
        lens = (ahead - start).norm(dim=-1)
        flown = torch.where(legs, lens, torch.zeros_like(lens)).sum(dim=1)
        first = self.episode_length_buf <= 1  # after the step's head: the pose was set, not flown to
        self.flight_length.copy_(torch.where(first, torch.zeros_like(flown), self.flight_length + flown))
        self.routed.copy_((jstar <= cnt) & ~first)
        self.skipped.copy_(torch.where(first, torch.zeros_like(jstar), jstar - 1))
        if self._cautious:
            self._count_unknown(jstar, first)

    def _rgba_or_zero(self, rgba):
        if rgba is None:
            if self._zero_rgba is None:
                cfg = self.cfg
                self._zero_rgba = torch.zeros(self.num_envs, cfg.camera_height, cfg.camera_width, 4, dtype=torch.uint8, device=self.device)
            rgba = self._zero_rgba
        return rgba

    def _observe_three_launches(self, actions_in, obs, stride, rgba, rgb_off, st):
        """step()'s head and the two small observation slices as the three separate launches (`fused_observe = False`)."""
        self._pre_step(actions_in, st)
        self._observe_slices(obs, stride, rgba, rgb_off, st)

    def _pre_step(self, actions_in, st):
        """step()'s head: clip, forced init action, poses; episode_length_buf += 1."""
        _lib.check(self.lib.gnbv_env_pre_step(actions_in.data_ptr(), C.byref(self._lat), self.episode_length_buf.data_ptr(), self.num_envs,
                                              self.actions.data_ptr(), self.poses.data_ptr(), st), "gnbv_env_pre_step")

    def _observe_slices(self, obs, stride, rgba, rgb_off, st):
        """obs["state"] and obs["state_rgb"]: the two small observation slices."""
        cfg, n, lib = self.cfg, self.num_envs, self.lib
        # (Round 5 ran the two small observation kernels below on a second stream beside the voxel update, joined in front of the
        # post-step kernel: the env step +1.9 ... +5.4 us, the voxel update +4.9 us -- they take slots from k_hit_list's single round of
        # workgroups.  profiles/r05_ab_rollout_obs_overlap.json)
        # obs["state"]
        _lib.check(lib.gnbv_env_obs_state(self.pose_hist.data_ptr(), self.poses.data_ptr(), self.reset_mask.data_ptr(),
                                          C.byref(self._lat), n, cfg.stack, obs.data_ptr(), stride, st), "gnbv_env_obs_state")
        # obs["state_rgb"]
        _lib.check(lib.gnbv_env_obs_rgb(rgba.data_ptr(), self.gray_prev.data_ptr(), self.reset_mask.data_ptr(), n,
                                        cfg.camera_height, cfg.camera_width, cfg.rgb_h, cfg.rgb_w,
                                        obs.data_ptr() + 4 * rgb_off, stride, st), "gnbv_env_obs_rgb")

    @property
    def supports_grid_i8(self) -> bool:
        """step(..., grid_i8_out=rows) also writes an int8 copy of the tri-class grid (coded update only)."""
        return bool(self.updater.coded)

    def reset(self, obs_out: Optional[torch.Tensor] = None, grid_i8_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Env_Train_GenNBV.reset (:229-244): reset every env, observe at the init pose."""
        n = self.num_envs
        self.episode_length_buf.zero_()
        self.reset_mask.fill_(1)
        self.prev_ratio.zero_()
        self.extras_time_outs.zero_()
        self.gray_prev.zero_()
        # reset_idx(all envs) (:231): a new extras["episode"] dict with rew_<name> = mean(episode_sums) / episode_length_s
        self.episode_state[0] += 1
        self.episode_state[1:] = (self.episode_sums.mean(dim=1) / np.float32(self.max_episode_length_s)).double()
        self.episode_sums.zero_()
        init = torch.tensor(self.cfg.init_action, dtype=torch.int64, device=self.device).repeat(n, 1)
        return self._observe_and_finish(init, obs_out, grid_i8_out)

    def step(self, actions: torch.Tensor, obs_out: Optional[torch.Tensor] = None, grid_i8_out: Optional[torch.Tensor] = None):
        _lib.require_cuda(actions)
        a = actions.to(torch.int64).contiguous()
        views = self.flag_views
        if views:
            self._reset_turn ^= 1
            self.reset_buf = self._reset_bufs[self._reset_turn]
            self._post.dones = self.reset_buf.data_ptr()
        obs = self._observe_and_finish(a, obs_out, grid_i8_out)
        self.extras["time_outs"] = self.extras_time_outs.view(torch.bool) if views else self.extras_time_outs.bool()
        info = _LazyEpisodeInfo(self, self._ep_step)
        self.extras["episode"] = info
        # dicts that are still referenced when their snapshot slot is about to be overwritten keep their last values (the
        # reference hands out plain dicts that never fail); the common case -- nobody holds a dict for ~1000 env steps --
        # costs one weakref per step and no read-back
        live = self._ep_live
        live.append(weakref.ref(info))
        while live:
            d = live[0]()
            if d is not None and self._ep_step - d._step < self._ep_hist - 2:
                break
            live.popleft()
            if d is not None:
                d._freeze()
        return obs, self.rew_buf, (self.reset_buf.view(torch.bool) if views else self.reset_buf.bool()), self.extras

    # ------------------------------------------------------------------------
    REWARD_NAMES = ("surface_coverage", "short_path", "termination")  # cfg.rewards.scales order = episode_sums order

    def episode_info(self, step: Optional[int] = None):
        """extras["episode"] of the reference as a reader of the entry handed out at env step `step` sees it NOW
        (default: the latest step).  The reference creates a new dict only on steps where some env resets
        (reset_idx :424-428) and otherwise keeps mutating the same object (update_extra_episode_info base:629-639), so
        an older buffer entry shows the values of the LAST step its dict was alive.  Resolved on demand from the
        per-step device snapshots the post-step kernel wrote (one read-back per env step at most; the reference pays
        a .cpu() per step)."""
        step = self._ep_step if step is None else step
        if self._ep_step - step >= self._ep_hist or step < 1:
            raise _lib.GennbvHipError("episode info of a step outside the snapshot history")
        if self._ep_cache[0] != self._ep_step:
            self._ep_cache = (self._ep_step, self.episode_info_hist.cpu().numpy())
        hist = self._ep_cache[1]
        gen = hist[step % self._ep_hist][0]
        last = step
        while last < self._ep_step and hist[(last + 1) % self._ep_hist][0] == gen:
            last += 1
        row = hist[last % self._ep_hist]
        out = {"rew_" + k: float(row[3 + i]) for i, k in enumerate(self.REWARD_NAMES)}
        out["episode_reward"], out["episode_length"] = float(row[1]), float(row[2])
        return out


class _LazyEpisodeInfo(dict):
    """The reference's extras["episode"] dict handed out with ONE env step; filled from the device snapshots when
    something reads it (every dict accessor fills first; see ReplayFeedEnv.episode_info for the aliasing rule)."""

    def __init__(self, env, step):
        super().__init__()
        self._env, self._step, self._seen = env, step, -1

    def _freeze(self):
        """Resolve once more and detach from the env: from here on a plain dict with the last values."""
        self._fill()
        self._env = None

    def _fill(self):
        if self._env is None:
            return
        if self._seen != self._env._ep_step:  # (the reference keeps mutating the dict while it is alive: refresh per env step)
            self._seen = self._env._ep_step
            super().update(self._env.episode_info(self._step))

    def __getitem__(self, k):
        self._fill()
        return super().__getitem__(k)

    def __iter__(self):
        self._fill()
        return super().__iter__()

    def __contains__(self, k):
        self._fill()
        return super().__contains__(k)

    def __len__(self):
        self._fill()
        return super().__len__()

    def keys(self):
        self._fill()
        return super().keys()

    def values(self):
        self._fill()
        return super().values()

    def items(self):
        self._fill()
        return super().items()

    def get(self, k, d=None):
        self._fill()
        return super().get(k, d)

    def __repr__(self):
        self._fill()
        return super().__repr__()

    def __eq__(self, o):
        self._fill()
        return super().__eq__(o)

    def copy(self):
        self._fill()
        return super().copy()

    __hash__ = None

    def __bool__(self):
        self._fill()
        return super().__len__() > 0

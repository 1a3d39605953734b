"""CPU reference of the five env-step entry points of include/gennbv_hip.h (gnbv_env_pre_step, gnbv_env_obs_state,
gnbv_env_obs_rgb, gnbv_env_observe, gnbv_env_post_step[_contacts]).  TEST INFRASTRUCTURE ONLY: plain numpy, no GPU.

fp32 arithmetic is numpy float32, one rounding per operation, in the association order the header documents.  The episode
ring is two real `collections.deque(maxlen=ring_len)` extended in env order (update_extra_episode_info,
env_train_base.py:629-639); the slot arrays are derived from the deques and the running total: entry p lives at
p % ring_len.  The nearest-resize source pixels come from torch.nn.functional.interpolate on a CPU index image, not from
the formula of oracle/oracle.c, so the resize is checked by an independent implementation."""
from __future__ import annotations

import math
from collections import deque

import numpy as np

f32 = np.float32
TILE = 1024  # envs per pass of the post-step kernel's single workgroup (only used to DESCRIBE a step, never to compute it)


# ---------------------------------------------------------------------------
# the episode ring
# ---------------------------------------------------------------------------
class RingModel:
    """deque(maxlen=ring_len) + the number of entries ever appended + the slot array [ring_len] where entry p sits at
    p % ring_len.  Slots that no entry of the deque maps to keep what they held."""

    def __init__(self, ring_len, total=0, slots=None):
        self.ring_len = int(ring_len)
        self.total = int(total)
        self.slots = np.zeros(self.ring_len, f32) if slots is None else np.array(slots, f32)
        k = min(self.total, self.ring_len)
        self.dq = deque((f32(self.slots[p % self.ring_len]) for p in range(self.total - k, self.total)), maxlen=self.ring_len)

    def extend(self, values):
        values = [f32(v) for v in values]
        self.dq.extend(values)
        self.total += len(values)
        for i, v in enumerate(self.dq):
            self.slots[(self.total - len(self.dq) + i) % self.ring_len] = v

    def mean(self):
        """(exact mean rounded to fp64, sum |x_i|); (0, 0) when empty."""
        k = len(self.dq)
        if k == 0:
            return 0.0, 0.0
        xs = [float(v) for v in self.dq]
        return math.fsum(xs) / k, math.fsum(abs(x) for x in xs)


# ---------------------------------------------------------------------------
# post-step
# ---------------------------------------------------------------------------
class PostRef:
    """The state GnbvEnvPost points at, as numpy arrays, and the scalars of the struct."""
    ARRAYS = ("coverage_count", "num_valid", "prev_ratio", "episode_length_buf", "rewards", "dones", "reset_mask", "step_time_out",
              "extras_time_outs", "coverage_ratio", "episode_sums", "cur_reward_sum", "cur_episode_length", "ring_state",
              "episode_info", "episode_state")

    def __init__(self, arrays, *, only_positive, max_episode_length, scale_cov, scale_short, scale_term, coverage_threshold,
                 ring_len, max_episode_length_s, with_info=True):
        for k in self.ARRAYS:
            setattr(self, k, np.array(arrays[k]))
        self.n = self.num_valid.shape[0]
        self.only_positive, self.max_episode_length = bool(only_positive), int(max_episode_length)
        self.scale_cov, self.scale_short, self.scale_term = f32(scale_cov), f32(scale_short), f32(scale_term)
        self.coverage_threshold, self.max_episode_length_s = f32(coverage_threshold), f32(max_episode_length_s)
        self.with_info = with_info
        total = int(self.ring_state[0])
        self.ring_r = RingModel(ring_len, total, arrays["ring_reward"])
        self.ring_l = RingModel(ring_len, total, arrays["ring_length"])

    @property
    def ring_reward(self):
        return self.ring_r.slots

    @property
    def ring_length(self):
        return self.ring_l.slots


def post_step(st: PostRef, contact=None):
    """One gnbv_env_post_step (contact None) / gnbv_env_post_step_contacts call on `st`, in place.  Returns what the step did
    (for the tests' own assertions about their cases) and the quantities the episode_info tolerances are made of."""
    n = st.n
    length = st.episode_length_buf
    # compute_reward: _reward_surface_coverage, _reward_short_path, clip, termination (each product and sum rounded once)
    ratio = (st.coverage_count.astype(f32) / st.num_valid).astype(f32)
    r_cov = ((ratio - st.prev_ratio).astype(f32) * st.scale_cov).astype(f32)
    rew = (np.zeros(n, f32) + r_cov).astype(f32)
    extra = np.clip(length - 30, 0, 2)
    r_short = ((-extra).astype(f32) * st.scale_short).astype(f32)
    rew = (rew + r_short).astype(f32)
    if st.only_positive:
        rew = np.where(rew < 0, f32(0), rew).astype(f32)
    collided = np.zeros(n, bool) if contact is None else np.asarray(contact) != 0
    time_out = length >= st.max_episode_length
    reset = collided | time_out | (ratio > st.coverage_threshold)
    r_term = ((reset & ~time_out).astype(f32) * st.scale_term).astype(f32)
    rew = (rew + r_term).astype(f32)
    st.rewards = rew
    st.dones = reset.astype(np.uint8)
    st.coverage_ratio = ratio
    # episode_sums += the step's terms; reset_idx logs their mean over the reset envs and zeroes them
    sums = (st.episode_sums + np.stack([r_cov, r_short, r_term])).astype(f32)
    st.episode_sums = np.where(reset[None, :], f32(0), sums).astype(f32)
    st.prev_ratio = np.where(reset, f32(0), ratio).astype(f32)
    st.reset_mask = reset.astype(np.uint8)
    st.episode_length_buf = np.where(reset, 0, length).astype(np.int64)
    st.step_time_out = time_out.astype(np.uint8)
    # update_extra_episode_info: finished episodes go to the deques in env order
    cur_sum = (st.cur_reward_sum + rew).astype(f32)
    cur_len = (st.cur_episode_length + f32(1)).astype(f32)
    st.cur_reward_sum = np.where(reset, f32(0), cur_sum).astype(f32)
    st.cur_episode_length = np.where(reset, f32(0), cur_len).astype(f32)
    ids = np.nonzero(reset)[0]
    st.ring_r.extend(cur_sum[ids])
    st.ring_l.extend(cur_len[ids])
    st.ring_state = np.array([st.ring_r.total], np.int64)
    count = ids.size
    out = {"reset": reset, "time_out": time_out, "r_short": r_short, "r_term": r_term, "count": count,
           "max_tile_finished": max(int(reset[t:t + TILE].sum()) for t in range(0, n, TILE))}
    if count:  # infos["time_outs"] is refreshed only on steps where some env resets
        st.extras_time_outs = time_out.astype(np.uint8)
    if st.with_info:
        if count:  # a new extras["episode"] dict
            st.episode_state = st.episode_state.copy()
            st.episode_state[0] += 1.0
            out["sum_abs"] = []  # sum |s| over the reset envs, per reward name
            for k in range(3):
                s = [float(v) for v in sums[k][ids]]
                st.episode_state[1 + k] = float(f32(math.fsum(s) / count) / st.max_episode_length_s)
                out["sum_abs"].append(math.fsum(abs(v) for v in s))
        (mr, ar), (ml, al) = st.ring_r.mean(), st.ring_l.mean()
        st.episode_info = np.array([st.episode_state[0], mr, ml, *st.episode_state[1:4]], np.float64)
        out["mean_abs"] = (ar, al)  # sum |x_i| over each deque
    return out


# ---------------------------------------------------------------------------
# observe: step()'s head + the pose-history slice + the gray-frame slice
# ---------------------------------------------------------------------------
class Lattice:
    """GnbvLattice on the host."""

    def __init__(self, clip_low, clip_up, init_action, action_unit, pose_low, init_pose):
        self.clip_low, self.clip_up = np.array(clip_low, np.int64), np.array(clip_up, np.int64)
        self.init_action = np.array(init_action, np.int64)
        self.action_unit, self.pose_low, self.init_pose = np.array(action_unit, f32), np.array(pose_low, f32), np.array(init_pose, f32)

    @classmethod
    def from_config(cls, cfg):
        return cls(cfg.clip_pose_idx_low, cfg.clip_pose_idx_up, cfg.init_action, cfg.action_unit, cfg.clip_pose_low, cfg.init_pose_buf)


def resize_source_index(h, w, oh, ow):
    """[oh*ow] flat source pixel of every output pixel of a nearest resize, from torch's own CPU implementation."""
    import torch
    idx = torch.arange(h * w, dtype=torch.float32).reshape(1, 1, h, w)  # (exact: h*w < 2^24)
    assert h * w < 2 ** 24
    return torch.nn.functional.interpolate(idx, size=(oh, ow), mode="nearest").reshape(-1).long().numpy()


def gray_resized(rgba, oh, ow):
    """[n, oh*ow] fp32: nearest-resized gray frames, three fp32 products and two fp32 additions in channel order, through uint8."""
    rgba = np.asarray(rgba, np.uint8)
    n, h, w, _ = rgba.shape
    px = rgba.reshape(n, h * w, 4)[:, resize_source_index(h, w, oh, ow)].astype(f32)
    v = (f32(0.2989) * px[..., 0]).astype(f32)
    v = (v + (f32(0.587) * px[..., 1]).astype(f32)).astype(f32)
    v = (v + (f32(0.114) * px[..., 2]).astype(f32)).astype(f32)
    return v.astype(np.uint8).astype(f32)


def observe(actions_in, lat: Lattice, episode_length_buf, pose_hist, gray_prev, rgba, reset_mask, oh, ow):
    """gnbv_env_observe (= gnbv_env_pre_step, gnbv_env_obs_state, gnbv_env_obs_rgb in that order).  episode_length_buf [n],
    pose_hist [n, stack, 6] and gray_prev [n, oh*ow] are updated in place; reset_mask [n] or None.
    Returns actions_out [n,6] i64, poses_out [n,6] f32, the state slice [n, stack*6] and the rgb slice [n, 2*oh*ow]."""
    n, stack = pose_hist.shape[0], pose_hist.shape[1]
    a = np.clip(np.asarray(actions_in, np.int64), lat.clip_low, lat.clip_up)
    a[episode_length_buf == 0] = lat.init_action
    poses = ((a.astype(f32) * lat.action_unit).astype(f32) + lat.pose_low).astype(f32)
    episode_length_buf += 1
    reset = np.zeros(n, bool) if reset_mask is None else np.asarray(reset_mask) != 0
    old = np.where(reset[:, None, None], lat.init_pose[None, None, :], pose_hist).astype(f32)
    pose_hist[:] = np.concatenate([old[:, 1:], poses[:, None, :]], axis=1)
    gray = gray_resized(rgba, oh, ow)
    older = np.where(reset[:, None], f32(0), gray_prev).astype(f32)
    gray_prev[:] = gray
    return a, poses, pose_hist.reshape(n, stack * 6).copy(), np.concatenate([older, gray], axis=1)

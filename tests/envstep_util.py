"""Shared by the env-step tests: the device state of gnbv_env_post_step and the oracle env with contacts."""
import numpy as np
import torch

DEV = "cuda:0"
f32 = np.float32


class PostState:
    """The device state of gnbv_env_post_step, random but consistent."""
    NAMES = ("coverage_count", "num_valid", "prev_ratio", "episode_length_buf", "rewards", "dones", "reset_mask", "step_time_out",
             "extras_time_outs", "coverage_ratio", "episode_sums", "cur_reward_sum", "cur_episode_length", "ring_reward", "ring_length",
             "ring_state", "episode_info", "episode_state")

    def __init__(self, n, cfg, max_len, seed, ring_len=100):
        g = torch.Generator().manual_seed(seed)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
        self.n, self.cfg, self.max_len, self.ring_len = n, cfg, max_len, ring_len
        self.with_info = True  # False: GnbvEnvPost.episode_info = NULL
        self.coverage_count = z(n, dt=torch.int32)
        self.num_valid = (200 + torch.randint(0, 100, (n,), generator=g)).float().to(DEV)
        self.prev_ratio, self.episode_length_buf = z(n), torch.randint(0, max_len, (n,), generator=g).to(DEV)
        self.rewards, self.dones, self.reset_mask = z(n), z(n, dt=torch.uint8), z(n, dt=torch.uint8)
        self.step_time_out, self.extras_time_outs, self.coverage_ratio = z(n, dt=torch.uint8), z(n, dt=torch.uint8), z(n)
        self.episode_sums, self.cur_reward_sum, self.cur_episode_length = z(3, n), z(n), z(n)
        self.ring_reward, self.ring_length, self.ring_state = z(ring_len), z(ring_len), z(1, dt=torch.int64)
        self.episode_info, self.episode_state = z(6, dt=torch.float64), z(4, dt=torch.float64)

    def clone(self):
        c = PostState.__new__(PostState)
        c.n, c.cfg, c.max_len, c.ring_len, c.with_info = self.n, self.cfg, self.max_len, self.ring_len, self.with_info
        for k in self.NAMES:
            setattr(c, k, getattr(self, k).clone())
        return c

    def scalars(self):
        """The scalar fields of GnbvEnvPost, as the env computes them (a Python-float scale is rounded to fp32 first)."""
        cfg = self.cfg
        return dict(only_positive=int(cfg.only_positive_rewards), max_episode_length=self.max_len,
                    scale_cov=float(f32(cfg.scale_surface_coverage * cfg.dt)), scale_short=float(f32(cfg.scale_short_path * cfg.dt)),
                    scale_term=float(f32(cfg.scale_termination * cfg.dt)), coverage_threshold=float(f32(cfg.coverage_threshold)),
                    ring_len=self.ring_len, max_episode_length_s=float(f32(cfg.episode_length_s)))

    def struct(self):
        from gennbv_amd import _lib
        sc, p = self.scalars(), _lib.GnbvEnvPost()
        p.n, p.only_positive, p.max_episode_length = self.n, sc["only_positive"], sc["max_episode_length"]
        p.scale_cov, p.scale_short, p.scale_term = sc["scale_cov"], sc["scale_short"], sc["scale_term"]
        p.coverage_threshold = sc["coverage_threshold"]
        p.coverage_count, p.num_valid_voxel_gt = self.coverage_count.data_ptr(), self.num_valid.data_ptr()
        p.prev_ratio, p.episode_length_buf = self.prev_ratio.data_ptr(), self.episode_length_buf.data_ptr()
        p.rewards, p.dones, p.reset_mask = self.rewards.data_ptr(), self.dones.data_ptr(), self.reset_mask.data_ptr()
        p.step_time_out, p.extras_time_outs = self.step_time_out.data_ptr(), self.extras_time_outs.data_ptr()
        p.coverage_ratio, p.episode_sums = self.coverage_ratio.data_ptr(), self.episode_sums.data_ptr()
        p.cur_reward_sum, p.cur_episode_length = self.cur_reward_sum.data_ptr(), self.cur_episode_length.data_ptr()
        p.ring_reward, p.ring_length, p.ring_state, p.ring_len = (self.ring_reward.data_ptr(), self.ring_length.data_ptr(),
                                                                  self.ring_state.data_ptr(), sc["ring_len"])
        p.episode_info = self.episode_info.data_ptr() if self.with_info else None
        p.episode_state = self.episode_state.data_ptr()
        p.max_episode_length_s = sc["max_episode_length_s"]
        return p

    def advance(self, g, grow_max=40):
        """What the step does before the post-step: coverage grows (from 0 after a reset), the step is counted."""
        grow = torch.randint(0, grow_max, (self.n,), generator=g).to(DEV).int()
        self.coverage_count.copy_(torch.where(self.reset_mask.bool(), grow, self.coverage_count + grow))
        self.coverage_count.copy_(torch.minimum(self.coverage_count, self.num_valid.int()))
        self.episode_length_buf += 1

    def snapshot(self):
        return [getattr(self, k).cpu().numpy().tobytes() for k in self.NAMES]

    def host(self):
        """name -> numpy copy of every array."""
        return {k: getattr(self, k).cpu().numpy() for k in self.NAMES}


def contact_oracle_cls():
    from oracle.env_oracle import OracleEnv

    class ContactOracleEnv(OracleEnv):
        """oracle/env_oracle.OracleEnv with check_termination's collision_buf ORed into the resets (env_train_gennbv.py:445-457):
        `contact` [n] u8 for the next step, or -- with `collider` = (CollisionOracle, r, h, ground) -- the oracle's collisions at
        the oracle's own poses."""
        contact = None
        collider = None

        def _observe(self, depth_raw, seg_raw, rgba, c2w, poses):
            if self.collider is not None:
                o, r, h, ground = self.collider
                self.contact = o.codes(np.arange(self.n), poses, float(f32(r)), float(f32(h)), ground)
            return super()._observe(depth_raw, seg_raw, rgba, c2w, poses)

        def _reward_done(self, cov):
            n = self.n
            ratio = (cov.astype(f32) / self.num_valid).astype(f32)
            rew = np.zeros(n, f32)
            rew = (rew + ((ratio - self.prev_ratio).astype(f32) * self.s_cov).astype(f32)).astype(f32)
            extra = np.clip(self.episode_length_buf - 30, 0, 2)
            rew = (rew + ((-extra).astype(f32) * self.s_short).astype(f32)).astype(f32)
            if self.cfg.only_positive_rewards:
                rew = np.where(rew < 0, f32(0), rew).astype(f32)
            collided = np.zeros(n, bool) if self.contact is None else np.asarray(self.contact) != 0
            time_out = self.episode_length_buf >= self.max_episode_length
            reset = collided | time_out | (ratio > f32(self.cfg.coverage_threshold))
            self.time_out = time_out
            self.term = ((reset & ~time_out).astype(f32) * self.s_term).astype(f32)  # the termination reward of this step
            rew = (rew + self.term).astype(f32)
            return rew, reset, time_out, ratio
    return ContactOracleEnv

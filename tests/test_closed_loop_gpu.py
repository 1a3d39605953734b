"""GPU: the closed-loop env -- ReplayFeedEnv over a RenderFeed renders every step from the poses the actions give."""
import math

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _closed_env(n=8, h=48, w=64, g=20, max_len=6, seed=3, eval_env=False):
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=seed)
    feed = RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg)
    cls = ReplayFeedEvalEnv if eval_env else ReplayFeedEnv
    return cls(cfg, scene, feed, DEV, max_episode_length=max_len), cfg, scene


def _random_actions(cfg, n, gen):
    return torch.stack([torch.randint(0, int(u) + 1, (n,), generator=gen) for u in cfg.clip_pose_idx_up], -1).to(DEV)


def _frame(feed):
    return tuple(x.clone() for x in feed.last)


def test_closed_loop_equals_open_loop_over_its_own_frames():
    """Record every rendered frame of a closed-loop run with resets and forced init actions; an open-loop env over those
    frames with the same actions must give bit-identical observations, rewards, dones and grids (pins the step order)."""
    from gennbv_amd.env.replay_feed import ReplayFeed, ReplayFeedEnv
    n, steps = 8, 20
    env, cfg, scene = _closed_env(n=n, max_len=6)
    gen = torch.Generator().manual_seed(7)
    acts = [_random_actions(cfg, n, gen) for _ in range(steps)]
    outs = [(env.reset().clone(),)]
    frames = [_frame(env.feed)]
    for a in acts:
        o, r, d, _ = env.step(a)
        outs.append((o.clone(), r.clone(), d.clone()))
        frames.append(_frame(env.feed))
    grids = (env.prob_grid.clone(), env.scanned_gt_grid.clone(), env.coverage_ratio.clone())
    assert any(bool(o[2].any()) for o in outs[1:]), "no episode ended: resets not exercised"
    feed = ReplayFeed(*[torch.stack([f[i] for f in frames]).contiguous() for i in range(4)])
    ref = ReplayFeedEnv(cfg, scene, feed, DEV, max_episode_length=6)
    assert torch.equal(ref.reset(), outs[0][0])
    for k, a in enumerate(acts):
        o, r, d, _ = ref.step(a)
        assert torch.equal(o, outs[k + 1][0]) and torch.equal(r, outs[k + 1][1]) and torch.equal(d, outs[k + 1][2]), f"step {k}"
    for x, y in zip((ref.prob_grid, ref.scanned_gt_grid, ref.coverage_ratio), grids):
        assert torch.equal(x, y)


def test_constant_action_sees_nothing_new():
    n = 8
    env, cfg, _ = _closed_env(n=n, max_len=50)
    env.reset()
    gen = torch.Generator().manual_seed(1)
    a = S.sample_actions(n, cfg, gen).to(DEV)
    env.step(a)
    cov, scanned = env.coverage_ratio.clone(), env.scanned_gt_grid.clone()
    assert (cov > 0).any()
    for _ in range(3):
        env.step(a)
        assert torch.equal(env.coverage_ratio, cov) and torch.equal(env.scanned_gt_grid, scanned)


def test_yaw_orbit_raises_coverage():
    """Four views from the four sides of the scene, each looking at its centre: every step adds surface."""
    n = 8
    env, cfg, _ = _closed_env(n=n, max_len=50)
    env.reset()
    unit, low = cfg.action_unit, cfg.clip_pose_low
    prev = env.coverage_ratio.clone()
    for k in range(4):
        th = k * math.pi / 2
        x, y = 8.0 * math.cos(th), 8.0 * math.sin(th)  # on the scene's border, above its tallest box (z 10.1 m), 45 deg down
        yaw = (th + math.pi) % (2 * math.pi)
        a = [round((x - low[0]) / unit[0]), round((y - low[1]) / unit[1]), 50, 0, 9, round(yaw / unit[5]) % 12]
        env.step(torch.tensor([a] * n, dtype=torch.int64, device=DEV))
        cov = env.coverage_ratio.clone()
        assert (cov > prev).all(), f"view {k}: coverage {prev.tolist()} -> {cov.tolist()}"
        prev = cov


def test_different_actions_give_different_depth():
    n = 8
    env, cfg, _ = _closed_env(n=n, max_len=50)
    gen = torch.Generator().manual_seed(5)
    a, b = S.sample_actions(n, cfg, gen).to(DEV), S.sample_actions(n, cfg, gen).to(DEV)
    b[:, 5] = (a[:, 5] + 3) % 12  # at least a different yaw
    env.reset()
    env.step(a)
    da = env.feed.last[0].clone()
    env.reset()
    env.step(b)
    db = env.feed.last[0]
    for e in range(n):
        assert not torch.equal(da[e], db[e])


def test_ppo_learns_on_the_closed_loop_env():
    from gennbv_amd.network.hybrid_encoder import Hybrid_Encoder
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from gennbv_amd.sb3.ppo_grid_obs import PPO_Grid_Obs
    env, cfg, _ = _closed_env(n=16, h=64, w=64, g=20, max_len=8)
    kw = dict(net_arch=[], features_extractor_class=Hybrid_Encoder, features_extractor_kwargs=dict(
        encoder_param={"hidden_shapes": [256, 256], "visual_dim": 256},
        net_param={"transformer_params": [[1, 256], [1, 256]], "append_hidden_shapes": [256, 256]},
        state_input_shape=(cfg.state_dim,), visual_input_shape=(cfg.stack, 64, 64)))
    algo = PPO_Grid_Obs(ActorCriticPolicy_Train_Eval, env, learning_rate=1e-4, n_steps=8, batch_size=32, n_epochs=2, gamma=0.99,
                        gae_lambda=0.95, clip_range=0.2, clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.8, max_grad_norm=1.0,
                        target_kl=None, seed=1, device=DEV, policy_kwargs=kw)
    algo.learn(total_timesteps=2 * 8 * 16)
    rows = [d for _, d in algo.logger.history] + [algo.logger.name_to_value]
    losses = [float(d[k]) for d in rows for k in ("train/loss", "train/value_loss", "train/policy_gradient_loss") if k in d]
    assert losses and np.isfinite(losses).all(), losses
    for p in algo.policy.parameters():
        assert torch.isfinite(p).all()


def test_eval_env_scores_what_the_agent_saw():
    n, L = 6, 4
    env, cfg, _ = _closed_env(n=n, max_len=L, eval_env=True)
    gen = torch.Generator().manual_seed(2)
    env.reset()
    for _ in range(L + 1):
        *_, acc = env.step(S.sample_actions(n, cfg, gen).to(DEV))
    assert sorted(acc) == sorted(str(e) for e in range(n))
    assert all(np.isfinite(v) and v >= 0 for v in acc.values())

"""GPU: gnbv_view_gain (csrc/viewgain.hip) against the CPU oracle (tests/view_gain_oracle.py), exactly, and the greedy
next-best-view baseline built on it (gennbv_amd/eval/baselines.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import view_gain_oracle as VO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(h, w, g):
    return TaskConfig(camera_width=w, camera_height=h, grid_size=g)


def _lattice_poses(cfg, n, k, seed, extremes=True):
    from gennbv_amd.eval.baselines import LatticeCandidates
    lc = LatticeCandidates(cfg, k, seed)
    a = lc.sample(n)
    if extremes and k >= 2:
        a[:, 0, 4], a[:, 1, 4] = 0, 12  # pitch -pi/2 and +pi/2
    return lc.poses(a)


def _outside_poses(n, k):
    """Hand-placed sources outside the grid on each side, looking back at the scene centre (0, 0, 5)."""
    spots = [(-14.0, 0.3, 4.0), (14.0, -0.2, 5.0), (0.4, -15.0, 3.0), (-0.3, 15.0, 6.0), (0.5, 0.5, 17.0), (1.0, -1.0, -3.0),
             (-13.0, -12.5, 14.0), (12.0, 13.0, -2.0)]
    p = torch.zeros(n, k, 6)
    for e in range(n):
        for j in range(k):
            x, y, z = spots[(e + j) % len(spots)]
            p[e, j, :3] = torch.tensor([x, y, z])
            p[e, j, 5] = math.atan2(-y, -x) % (2 * math.pi)
            p[e, j, 4] = math.atan2(z - 5.0, math.hypot(x, y))
    return p


def _random_tri(n, g, occ, seed):
    gen = torch.Generator().manual_seed(seed)
    r = torch.rand(n, g ** 3, generator=gen)
    return torch.where(r < occ, 1, torch.where(r < occ + 0.4 * (1 - occ), -1, 0)).to(torch.int8)


def _run(cfg, scene, tri, poses, stride, range_m, chunk=0):
    from gennbv_amd.ops.view_gain import ViewGain
    n, k = poses.shape[:2]
    vg = ViewGain(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, range_m=range_m, device=DEV, with_c2w=True, chunk=chunk)
    gain = vg(tri.to(DEV), poses.to(DEV)).cpu().numpy()
    return vg, gain, vg.c2w.cpu().numpy()


def _oracle(cfg, scene, tri, c2w, stride, range_m):
    kinv = S.inverse_intrinsics(cfg.camera_height, cfg.camera_width, cfg.horizontal_fov).numpy()
    return VO.view_gain(tri.cpu().numpy(), c2w, scene.range_gt.numpy(), scene.voxel_size.numpy(), kinv, cfg.camera_height,
                        cfg.camera_width, stride, range_m)


CASES = [  # g, (h, w), stride, range, n, k, chunk, occupied density (None: all unknown), poses
    (16, (60, 80), 1, 2.0, 1, 5, 2, 0.02, "lattice"),
    (16, (60, 80), 4, 50.0, 37, 3, 2, 0.10, "lattice"),
    (20, (60, 80), 1, 50.0, 1, 5, 2, 0.01, "lattice"),
    (20, (240, 320), 4, 50.0, 1, 7, 3, 0.05, "outside"),
    (20, (400, 400), 8, 2.0, 1, 5, 2, 0.30, "lattice"),
    (20, (60, 80), 4, 50.0, 37, 3, 2, None, "lattice"),
    (33, (240, 320), 8, 50.0, 1, 5, 2, 0.02, "outside"),
    (33, (60, 80), 4, 2.0, 1, 5, 0, 0.10, "lattice"),
    (64, (240, 320), 4, 50.0, 1, 5, 2, 0.005, "lattice"),
    (64, (400, 400), 8, 50.0, 1, 3, 2, None, "lattice"),
    (64, (60, 80), 4, 2.0, 37, 3, 2, 0.05, "lattice"),
    (64, (240, 320), 8, 50.0, 1, 7, 3, 0.02, "outside"),
    # a lattice of exactly one wave (64 rays), and one of 4 800 rays: no whole number of waves, more than one turn of 1 024 lanes
    (20, (8, 8), 1, 50.0, 1, 5, 2, 0.05, "lattice"),
    (20, (60, 80), 1, 50.0, 1, 5, 2, 0.05, "lattice"),
]


@pytest.mark.parametrize("g,cam,stride,range_m,n,k,chunk,occ,kind", CASES)
def test_kernel_equals_oracle(g, cam, stride, range_m, n, k, chunk, occ, kind):
    cfg = _cfg(cam[0], cam[1], g)
    scene = S.make_scenes(n, g, seed=2)
    tri = torch.zeros(n, g ** 3, dtype=torch.int8) if occ is None else _random_tri(n, g, occ, seed=g + n)
    poses = _lattice_poses(cfg, n, k, seed=g) if kind == "lattice" else _outside_poses(n, k)
    _, gain, c2w = _run(cfg, scene, tri, poses, stride, range_m, chunk)
    want = _oracle(cfg, scene, tri, c2w, stride, range_m)
    print("gain sum", gain.sum(axis=(0, 1)), "oracle", want.sum(axis=(0, 1)))
    assert np.array_equal(gain, want)
    assert gain[..., 0].max() > 0 or occ is not None


def _closed_env(n=8, h=60, w=80, g=20, max_len=20, seed=1, collision=None, eval_env=True):
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv
    cfg = _cfg(h, w, g)
    scene = S.make_scenes(n, g, seed=seed)
    feed = RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg)
    cls = ReplayFeedEvalEnv if eval_env else ReplayFeedEnv
    return cls(cfg, scene, feed, DEV, max_episode_length=max_len, collision=collision), cfg, scene


def test_rollout_grids_equal_oracle_and_camera_equals_renderer():
    """The grids of a real closed-loop rollout after 1, 5 and 20 steps; c2w_out bit-equal to the renderer's camera."""
    from gennbv_amd.eval.baselines import RandomLatticePolicy
    n, k = 4, 4
    env, cfg, scene = _closed_env(n=n, max_len=50, eval_env=False)
    pol = RandomLatticePolicy(cfg, n, seed=3)
    obs = env.reset()
    poses = _lattice_poses(cfg, n, k, seed=9)
    for step in range(1, 21):
        obs, _, _, _ = env.step(pol(obs)[0])
        if step in (1, 5, 20):
            tri = obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]
            _, gain, c2w = _run(cfg, scene, tri, poses, 4, 50.0, chunk=3)
            want = _oracle(cfg, scene, tri.cpu(), c2w, 4, 50.0)
            assert np.array_equal(gain, want), step
            assert want[..., 2].sum() > 0 and want[..., 0].sum() > 0
    feed = env.feed
    for j in range(k):
        cam = feed.render(poses[:, j].contiguous().to(DEV))[3].cpu().numpy()
        assert np.array_equal(cam.view(np.uint32), c2w[:, j].view(np.uint32)), j


def test_outputs_overwritten_deterministic_strided_and_fp32():
    from gennbv_amd.ops.view_gain import ViewGain
    g, n, k = 20, 5, 7
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=4)
    tri = _random_tri(n, g, 0.03, seed=1).to(DEV)
    poses = _lattice_poses(cfg, n, k, seed=5).to(DEV)
    vg = ViewGain(n, k, cfg, scene.range_gt, scene.voxel_size, device=DEV, with_c2w=True, chunk=3)
    vg.gain.fill_(-12345)
    vg.c2w.fill_(float("nan"))
    a = vg(tri, poses).clone()
    assert not bool((a == -12345).any()) and not bool(torch.isnan(vg.c2w).any())
    assert torch.equal(vg(tri, poses), a)
    big = torch.full((n, g ** 3 + 13), 1, dtype=torch.int8, device=DEV)  # rows inside a larger buffer, unaligned stride
    big[:, 5:5 + g ** 3] = tri
    assert torch.equal(vg(big[:, 5:5 + g ** 3], poses), a)
    assert torch.equal(vg(tri.float(), poses), a)
    assert torch.equal(vg(tri.view(n, g, g, g), poses), a)
    for chunk in (1, 7):
        assert torch.equal(ViewGain(n, k, cfg, scene.range_gt, scene.voxel_size, device=DEV, chunk=chunk)(tri, poses), a)


def test_refusals():
    from gennbv_amd import _lib
    from gennbv_amd.ops.view_gain import ViewGain
    scene = S.make_scenes(2, 20, seed=1)
    cfg = _cfg(60, 80, 20)
    with pytest.raises(_lib.GennbvHipError):
        ViewGain(2, 4, _cfg(60, 80, 128), scene.range_gt, scene.voxel_size, device=DEV)
    with pytest.raises(_lib.GennbvHipError):
        ViewGain(2, 4, cfg, scene.range_gt, scene.voxel_size, device="cpu")
    vg = ViewGain(2, 4, cfg, scene.range_gt, scene.voxel_size, device=DEV)
    with pytest.raises(_lib.GennbvHipError):
        vg(torch.zeros(2, 8000, dtype=torch.int8), torch.zeros(2, 4, 6))
    tri, poses = torch.zeros(2, 8000, dtype=torch.int8, device=DEV), torch.zeros(2, 4, 6, device=DEV)
    vg(tri, poses)
    lib = _lib.load()
    for field, bad in (("stride", 0), ("range", 0.0), ("range", float("inf")), ("k", 0), ("g", 128)):
        a = _lib.GnbvViewGain()
        C.memmove(C.byref(a), C.byref(vg._args), C.sizeof(a))
        setattr(a, field, bad)
        assert lib.gnbv_view_gain(C.byref(a), None) == 1, field  # hipErrorInvalidValue


def _oracle_backend(env, cfg, scene, k, stride=4):
    """The same decision with the oracle's gains: the device operator only supplies the camera matrices."""
    from gennbv_amd.ops.view_gain import ViewGain
    vg = ViewGain(env.num_envs, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, device=DEV, with_c2w=True)

    def backend(tri, poses):
        vg(tri, poses)
        want = _oracle(cfg, scene, tri.to(torch.int8).cpu(), vg.c2w.cpu().numpy(), stride, abs(cfg.depth_sense_dist))
        return torch.from_numpy(want).to(tri.device)
    return backend


def test_greedy_policy_chooses_the_oracle_policy_actions():
    from gennbv_amd.eval.baselines import GreedyGainPolicy
    k = 8
    env_a, cfg, scene = _closed_env(n=4, eval_env=False)
    env_b, _, _ = _closed_env(n=4, eval_env=False)
    pa = GreedyGainPolicy(env_a, k=k, seed=7)
    pb = GreedyGainPolicy(env_b, k=k, seed=7, gain_backend=_oracle_backend(env_b, cfg, scene, k))
    oa, ob = env_a.reset(), env_b.reset()
    for step in range(5):
        a, b = pa(oa)[0], pb(ob)[0]
        assert torch.equal(a, b), step
        oa, ob = env_a.step(a)[0], env_b.step(b)[0]
        assert torch.equal(oa, ob)


def _final_coverage(policy, env):
    """Mean over envs of env.coverage_ratio on each env's done step, and mean_AUC.  The post-step kernel writes
    coverage_ratio before it resets the env's counters, so the done step still shows the finished episode's value; it is read
    in the evaluation's callback."""
    from gennbv_amd.eval import evaluate_policy_grid_obs
    n = env.num_envs
    final, contact = {}, {}

    def cb(loc, _):
        i = loc["i"]
        if bool(loc["done"]) and i not in final:
            final[i] = float(env.coverage_ratio[i])
            contact[i] = int(env.collision_buf[i]) if env.collision_buf is not None else 0
    _, lens, auc, _ = evaluate_policy_grid_obs(policy, env, n_eval_episodes=n, callback=cb)
    assert len(final) == n
    return float(np.mean(list(final.values()))), float(auc.mean()), lens, contact


@pytest.mark.parametrize("seed", [1, 2])
def test_greedy_beats_random_coverage_closed_loop(seed):
    from gennbv_amd.eval.baselines import GreedyGainPolicy, RandomLatticePolicy
    env_g, cfg, _ = _closed_env()
    env_r, _, _ = _closed_env()
    cg, ag, _, _ = _final_coverage(GreedyGainPolicy(env_g, k=32, weights=(1, 4), seed=seed), env_g)
    cr, ar, _, _ = _final_coverage(RandomLatticePolicy(cfg, env_r.num_envs, seed), env_r)
    print(f"seed {seed}: final coverage greedy {cg:.4f} random {cr:.4f}; mean_AUC greedy {ag:.4f} random {ar:.4f}")
    assert cg > cr


def test_greedy_avoids_collisions_random_does_not():
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.eval.baselines import GreedyGainPolicy, RandomLatticePolicy
    hit_random = 0
    for seed in (1, 2):
        env_g, cfg, _ = _closed_env(collision=CollisionBody())
        env_r, _, _ = _closed_env(collision=CollisionBody())
        _, _, lens_g, contact_g = _final_coverage(GreedyGainPolicy(env_g, k=32, seed=seed), env_g)
        _, _, _, contact_r = _final_coverage(RandomLatticePolicy(cfg, env_r.num_envs, seed), env_r)
        assert all(v == 0 for v in contact_g.values()), contact_g
        assert not bool(env_g.collision_buf.any())
        hit_random += sum(v != 0 for v in contact_r.values())
    assert hit_random >= 1

"""GPU: surface voxelization of a MeshScene (gnbv_voxelize_surface, csrc/voxelize.hip) against make_scenes' analytic box
grids and an fp64 brute-force separating-axis oracle (tests/voxelize_oracle.py), and closed-loop envs built from
triangles alone (MeshScene.ground_truth / surface_points)."""
import math

import numpy as np
import pytest
import torch

from tests import voxelize_oracle as VO
from gennbv_amd import _lib
from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.mesh_scene import MeshScene, box_triangles, random_rotation, sphere_triangles

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# voxel edge per grid size for the oracle scenes: dyadic, so every voxel face is an exact fp32 number and a triangle can
# lie exactly on one
DYADIC = {20: 0.75, 64: 0.25, 128: 0.125}


def _range_for(g, n):
    """range_gt [n,6] with voxel edge DYADIC[g]: x, y symmetric about 0, z from 0 (the reference frame)."""
    v = DYADIC[g]
    h = 0.5 * v * (g - 1)
    return torch.tensor([[h, -h, h, -h, v * (g - 1), 0.0]] * n, dtype=torch.float32)


def _faces(rng_row, vox_row, g):
    return VO.voxel_bounds(rng_row.numpy(), vox_row.numpy(), g)[2]  # [3, g+1] float64


def _rotated_env(gen, n_boxes=3):
    t = []
    for _ in range(n_boxes):
        half = 0.5 + torch.rand(3, generator=gen, dtype=torch.float64) * 2.0
        b = box_triangles(-half[None], half[None]).double() @ random_rotation(gen).T
        centre = torch.cat([(torch.rand(2, generator=gen, dtype=torch.float64) - 0.5) * 9.0,
                            2.5 + torch.rand(1, generator=gen, dtype=torch.float64) * 3.0])
        t.append((b + centre).float())
    c = [float(x) for x in (torch.rand(3, generator=gen) - 0.5) * torch.tensor([8.0, 8.0, 2.0]) + torch.tensor([0.0, 0.0, 3.5])]
    t.append(sphere_triangles(c, 1.0 + float(torch.rand(1, generator=gen)) * 1.5, 10, 20))
    return torch.cat(t)


def _degenerate_env(gen, faces):
    """Slivers, zero-area triangles (points, segments, a repeated vertex) and small random triangles."""
    t = []
    for _ in range(40):
        a = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * torch.tensor([10.0, 10.0, 0.0]) + torch.tensor([0, 0, 4.0])
        a[2] += float(torch.rand(1, generator=gen)) * 4.0
        d = torch.randn(3, generator=gen, dtype=torch.float64)
        t.append(torch.stack([a, a + 3.0 * d, a + 3.0 * d + 1e-4 * torch.randn(3, generator=gen, dtype=torch.float64)]))  # sliver
        t.append(torch.stack([a, a, a]))  # point
        t.append(torch.stack([a, a + d, a + 2.5 * d]))  # collinear segment
        t.append(torch.stack([a, a + d, a]))  # repeated vertex
        t.append(a + 0.4 * torch.randn(3, 3, generator=gen, dtype=torch.float64))
    # a point exactly on a voxel corner, a segment exactly along a voxel edge
    fx, fy, fz = faces
    p = torch.tensor([fx[5], fy[7], fz[3]], dtype=torch.float64)
    t.append(torch.stack([p, p, p]))
    q = torch.tensor([fx[9], fy[4], fz[2]], dtype=torch.float64)
    t.append(torch.stack([q, q + torch.tensor([0.0, 0.0, fz[6] - fz[2]], dtype=torch.float64), q]))
    return torch.stack(t).float()


def _boundary_env(faces, g):
    """Triangles lying exactly in voxel face planes, vertices on voxel corners, an axis-aligned box on voxel faces."""
    fx, fy, fz = (torch.from_numpy(f) for f in faces)
    k = g // 4
    t = [
        torch.tensor([[fx[k], fy[k], fz[k]], [fx[2 * k], fy[k], fz[k]], [fx[k], fy[2 * k], fz[k]]]),  # in a z plane
        torch.tensor([[fx[k + 1], fy[k], fz[2]], [fx[k + 1], fy[3 * k], fz[2]], [fx[k + 1], fy[k], fz[k + 2]]]),  # in an x plane
        torch.tensor([[fx[2], fy[2 * k + 1], fz[1]], [fx[3 * k], fy[2 * k + 1], fz[1]], [fx[2], fy[2 * k + 1], fz[3 * k]]]),  # y plane
        # a tilted triangle with all three vertices on voxel corners
        torch.tensor([[fx[3], fy[3], fz[3]], [fx[3 * k], fy[5], fz[4]], [fx[6], fy[3 * k], fz[2 * k]]]),
    ]
    lo = torch.tensor([fx[2 * k], fy[2 * k], fz[2]])
    hi = torch.tensor([fx[3 * k], fy[3 * k - 1], fz[k + 3]])
    t.append(box_triangles(lo[None].float(), hi[None].float()).double())
    return torch.cat([x.double().reshape(-1, 3, 3) for x in t]).float()


def _outside_env(rng_row):
    """Triangles partly outside the range (through a side, below z = 0, across the whole grid) and wholly outside it."""
    h, zt = float(rng_row[0]), float(rng_row[4])
    t = torch.tensor([
        [[h - 1.0, 0.0, 2.0], [h + 3.0, 1.0, 2.5], [h + 3.0, -1.0, 3.0]],  # through the +x side
        [[0.0, 0.0, -1.0], [2.0, 0.0, 1.0], [0.0, 2.0, 1.0]],  # through the floor
        [[-3 * h, -3 * h, 0.3 * zt], [3 * h, -3 * h, 0.6 * zt], [0.0, 3 * h, 0.45 * zt]],  # across the whole grid
        [[3 * h, 3 * h, 1.0], [4 * h, 3 * h, 1.0], [3 * h, 4 * h, 2.0]],  # wholly outside
        [[0.0, 0.0, 3 * zt], [1.0, 0.0, 3 * zt], [0.0, 1.0, 3 * zt]],  # above
    ])
    return t


def _oracle_scene(g, n_rot, seed):
    """Envs: n_rot rotated-box + sphere envs, then degenerate, boundary-plane, outside-the-range and empty envs."""
    gen = torch.Generator().manual_seed(seed)
    rng = _range_for(g, n_rot + 4)
    vox = torch.full((n_rot + 4, 3), DYADIC[g], dtype=torch.float32)
    faces = _faces(rng[0], vox[0], g)
    tris = [_rotated_env(gen) for _ in range(n_rot)]
    tris += [_degenerate_env(gen, faces), _boundary_env(faces, g), _outside_env(rng[0]), torch.zeros(0, 3, 3)]
    ids = [torch.ones(t.shape[0], dtype=torch.int32) for t in tris]
    return MeshScene.from_triangles(tris, ids, device=DEV), rng, vox


def _voxelize(mesh, rng, vox, g):
    grid = torch.full((mesh.num_envs, g, g, g), float("nan"), device=DEV)
    mesh.voxelize_into(grid, rng.to(DEV), vox.to(DEV))
    torch.cuda.synchronize()
    return grid


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [20, 64, 128])
def test_box_scenes_equal_make_scenes(g):
    n = 8 if g < 128 else 4
    sc = S.make_scenes(n, g, seed=11 + g)
    gt = MeshScene.from_boxes(sc, device=DEV).ground_truth(g, range_gt=sc.range_gt)
    assert gt.grid_gt.shape == (n, g, g, g) and gt.grid_gt.dtype == torch.float32
    assert torch.equal(gt.range_gt.cpu(), sc.range_gt) and torch.equal(gt.voxel_size.cpu(), sc.voxel_size)
    assert torch.equal(gt.env_origins.cpu(), sc.env_origins) and gt.boxes_min.shape == (n, 0, 3)
    got = gt.grid_gt.cpu()
    excluded = 0
    for e in range(n):
        t = VO.tau(sc.range_gt[e].numpy())
        faces = _faces(sc.range_gt[e], sc.voxel_size[e], g)
        keep = torch.ones(g, g, g, dtype=torch.bool)
        valid = (sc.boxes_min[e] <= sc.boxes_max[e]).all(-1)
        for k in torch.nonzero(valid).flatten().tolist():
            for a in range(3):
                for plane in (float(sc.boxes_min[e, k, a]), float(sc.boxes_max[e, k, a])):
                    near = np.abs(faces[a] - plane) <= t  # voxel faces within tau of the box face plane
                    bad = torch.from_numpy(near[:-1] | near[1:])
                    shape = [1, 1, 1]
                    shape[a] = g
                    keep &= ~bad.reshape(shape)
        excluded += int((~keep).sum())
        diff = (got[e] != sc.grid_gt[e]) & keep
        assert not diff.any(), f"env {e}: {int(diff.sum())} voxels differ from make_scenes"
    print(f"G={g}: {excluded} voxels within tau of a box-face plane excluded")
    assert torch.equal(gt.num_valid_voxel_gt.cpu(), got.sum(dim=(1, 2, 3)).clamp(min=1.0))


@pytest.mark.parametrize("g,n_rot", [(20, 3), (64, 2)])
def test_oracle_contract(g, n_rot):
    mesh, rng, vox = _oracle_scene(g, n_rot, seed=g)
    grid = _voxelize(mesh, rng, vox, g).cpu()
    assert not torch.isnan(grid).any(), "a voxel was not written"
    assert torch.all((grid == 0) | (grid == 1))
    for e in range(mesh.num_envs):
        t = VO.tau(rng[e].numpy())
        sep = VO.separation(mesh.env_triangles(e)[0].cpu(), rng[e].numpy(), vox[e].numpy(), g, reach=2 * t)
        fn, fp_far, fp_near = VO.check(grid[e], sep, t)
        print(f"G={g} env {e}: {int(grid[e].sum())} voxels, {fn} false negatives, {fp_far} false positives beyond tau, "
              f"{fp_near} within tau")
        assert fn == 0 and fp_far == 0
    assert int(grid[-1].sum()) == 0  # the empty env
    assert grid[n_rot + 1].sum() > 0 and grid[n_rot + 2].sum() > 0  # boundary-plane and outside-the-range envs mark voxels


def test_oracle_contract_one_env_at_128():
    g = 128
    gen = torch.Generator().manual_seed(128)
    rng = _range_for(g, 1)
    vox = torch.full((1, 3), DYADIC[g], dtype=torch.float32)
    faces = _faces(rng[0], vox[0], g)
    tris = torch.cat([_rotated_env(gen), _boundary_env(faces, g), _outside_env(rng[0])])
    mesh = MeshScene.from_triangles([tris], [torch.ones(tris.shape[0], dtype=torch.int32)], device=DEV)
    grid = _voxelize(mesh, rng, vox, g).cpu()
    assert not torch.isnan(grid).any()
    t = VO.tau(rng[0].numpy())
    sep = VO.separation(tris, rng[0].numpy(), vox[0].numpy(), g, reach=2 * t)
    fn, fp_far, fp_near = VO.check(grid[0], sep, t)
    print(f"G=128: {int(grid[0].sum())} voxels, {fn} false negatives, {fp_far} beyond tau, {fp_near} within tau")
    assert fn == 0 and fp_far == 0


def test_deterministic_and_every_voxel_written():
    g = 64
    mesh, rng, vox = _oracle_scene(g, 3, seed=5)
    a = _voxelize(mesh, rng, vox, g)
    b = torch.full_like(a, float("nan"))
    b[::2] = -7.0  # any prior content is overwritten
    mesh.voxelize_into(b, rng.to(DEV), vox.to(DEV))
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and not torch.isnan(b).any()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_bad_arguments_and_bad_voxel_size():
    g = 16
    mesh, rng, vox = _oracle_scene(20, 1, seed=1)
    n = mesh.num_envs
    lib = _lib.load()
    import ctypes as C
    sc = mesh.c_struct()
    grid = torch.zeros(n, g, g, g, device=DEV)
    r, v = rng.to(DEV), vox.to(DEV)
    st = _lib.stream_ptr(DEV)
    for bad_g in (0, 1, 1025):
        assert lib.gnbv_voxelize_surface(C.byref(sc), r.data_ptr(), v.data_ptr(), bad_g, grid.data_ptr(), st) != 0
    assert lib.gnbv_voxelize_surface(None, r.data_ptr(), v.data_ptr(), g, grid.data_ptr(), st) != 0
    assert lib.gnbv_voxelize_surface(C.byref(sc), r.data_ptr(), v.data_ptr(), g, None, st) != 0
    # a non-positive voxel size on the device: that env's grid is NaN, the others are voxelized as usual
    v_bad = v.clone()
    v_bad[1, 2] = 0.0
    v_bad[2, 0] = -0.5
    out = torch.zeros(n, g, g, g, device=DEV)
    mesh.voxelize_into(out, r, v_bad)
    ref = _voxelize(mesh, rng, vox, g)
    assert torch.isnan(out[1]).all() and torch.isnan(out[2]).all()
    keep = [e for e in range(n) if e not in (1, 2)]
    assert torch.equal(out[keep], ref[keep])


# ---------------------------------------------------------------------------------------------------------------
def _mesh_env(n=8, h=48, w=64, g=20, max_len=6, seed=3, eval_env=False):
    """A closed-loop env from triangles alone: spheres and rotated boxes, ground truth from the voxelizer."""
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    gen = torch.Generator().manual_seed(seed)
    tris = [_rotated_env(gen) for _ in range(n)]
    mesh = MeshScene.from_triangles(tris, [torch.ones(t.shape[0], dtype=torch.int32) for t in tris], device=DEV)
    gt = mesh.ground_truth(g)
    feed = RenderFeed(mesh, cfg)
    if eval_env:
        return ReplayFeedEvalEnv(cfg, gt, feed, DEV, max_episode_length=max_len, pc_gt=mesh.surface_points(4000, seed=1)), cfg, gt
    return ReplayFeedEnv(cfg, gt, feed, DEV, max_episode_length=max_len), cfg, gt


def test_closed_loop_hits_lie_in_the_ground_truth():
    from gennbv_amd import utils as U
    n, g = 8, 32
    env, cfg, gt = _mesh_env(n=n, h=96, w=128, g=g, max_len=100)
    kinv = S.inverse_intrinsics(cfg.camera_height, cfg.camera_width, cfg.horizontal_fov)
    hits = torch.zeros(n, g ** 3, dtype=torch.bool, device=DEV)
    gen = torch.Generator().manual_seed(4)
    env.reset()
    for _ in range(12):
        env.step(S.sample_actions(n, cfg, gen).to(DEV))
        depth_raw, seg_raw, _, c2w = env.feed.last
        d, s = U.post_process_depth(depth_raw, seg_raw, cfg.depth_sense_dist)
        pts = U.back_projection_fg(d, s, c2w, kinv)
        for e, idx in enumerate(U.scanned_pts_to_idx_3D(pts, gt.range_gt, gt.voxel_size, g)):
            if len(idx):
                hits[e, (idx[:, 0] * g + idx[:, 1]) * g + idx[:, 2]] = True
        assert (env.coverage_ratio <= 1.0).all()
    inside = hits & (gt.grid_gt.reshape(n, -1) > 0)
    share = float(inside.sum()) / max(int(hits.sum()), 1)
    print(f"closed loop: {int(hits.sum())} distinct hit voxels, {share:.6f} of them in grid_gt")
    assert int(hits.sum()) > 100 * n
    assert share >= 0.999


def test_closed_loop_yaw_orbit_raises_coverage():
    n = 8
    env, cfg, _ = _mesh_env(n=n, max_len=50)
    env.reset()
    unit, low = cfg.action_unit, cfg.clip_pose_low
    covs = [env.coverage_ratio.clone()]
    for k in range(4):
        th = k * math.pi / 2
        x, y = 8.0 * math.cos(th), 8.0 * math.sin(th)  # on the scene's border, 10.1 m up, 45 deg down
        yaw = (th + math.pi) % (2 * math.pi)
        a = [round((x - low[0]) / unit[0]), round((y - low[1]) / unit[1]), 50, 0, 9, round(yaw / unit[5]) % 12]
        env.step(torch.tensor([a] * n, dtype=torch.int64, device=DEV))
        covs.append(env.coverage_ratio.clone())
    for prev, cov in zip(covs[1:], covs[2:]):
        assert (cov >= prev).all()
    assert (covs[1] > 0).all() and (covs[-1] > covs[1]).all(), [c.tolist() for c in covs]
    assert (covs[-1] <= 1.0).all()


def test_ppo_learns_on_a_triangle_only_env():
    from gennbv_amd.network.hybrid_encoder import Hybrid_Encoder
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from gennbv_amd.sb3.ppo_grid_obs import PPO_Grid_Obs
    env, cfg, _ = _mesh_env(n=16, h=64, w=64, g=20, max_len=8)
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


def test_eval_env_scores_against_surface_points():
    n, L = 6, 4
    env, cfg, _ = _mesh_env(n=n, max_len=L, eval_env=True)
    assert all(p.shape == (4000, 3) for p in env.pc_gt)
    gen = torch.Generator().manual_seed(2)
    env.reset()
    for _ in range(L + 1):
        *_, acc = env.step(S.sample_actions(n, cfg, gen).to(DEV))
    assert sorted(acc) == sorted(str(e) for e in range(n))
    assert all(np.isfinite(v) and v >= 0 for v in acc.values())

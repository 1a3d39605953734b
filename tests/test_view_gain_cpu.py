"""CPU: the view-gain oracle's own sanity, LatticeCandidates, and GreedyGainPolicy's scoring with the oracle injected as the
gain backend (the injection point exists for tests; the product path has no CPU fallback)."""
import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import view_gain_oracle as VO

G, H, W = 16, 24, 32
CFG = TaskConfig(camera_width=W, camera_height=H, grid_size=G)


def _scene(n=1):
    return S.make_scenes(n, G, seed=1)


def _c2w(poses):
    return S.camera_to_world(torch.as_tensor(poses, dtype=torch.float32).view(-1, 6)).float().numpy()


def _gain(tri, poses, stride=2, range_m=50.0):
    sc = _scene()
    kinv = S.inverse_intrinsics(H, W, CFG.horizontal_fov).numpy()
    return VO.view_gain_env(tri, _c2w(poses), sc.range_gt[0].numpy(), sc.voxel_size[0].numpy(), kinv, H, W, stride, range_m)


INSIDE = [[0.0, 0.0, 5.0, 0.0, 0.0, 0.0], [1.0, -2.0, 3.0, 0.0, 0.5, 2.0]]  # sources inside the grid


def test_all_free_grid_gives_zero():
    assert np.array_equal(_gain(-np.ones((G, G, G), np.int8), INSIDE), np.zeros((2, 3), np.int32))


def test_all_unknown_grid_counts_the_distinct_ray_voxels():
    sc = _scene()
    kinv = S.inverse_intrinsics(H, W, CFG.horizontal_fov).numpy()
    got = _gain(np.zeros((G, G, G), np.int8), INSIDE)
    for j, c2w in enumerate(_c2w(INSIDE)):
        lin, valid = VO.ray_voxels(c2w, sc.range_gt[0].numpy(), sc.voxel_size[0].numpy(), kinv, H, W, 2, 50.0, G)
        assert got[j, 0] == np.unique(lin[valid]).size > 0
        assert got[j, 1] == 0 and got[j, 2] == 0


def test_occupied_plane_blocks_every_ray():
    tri = np.zeros((G, G, G), np.int8)
    tri[12] = 1  # the plane x index 12, between a source at x index 7 looking along +x and its targets
    got = _gain(tri, [[0.0, 0.0, 5.0, 0.0, 0.0, 0.0]])
    assert got[0, 2] == VO.lattice_count(H, W, 2)
    assert got[0, 1] == got[0, 0] > 0


@pytest.mark.parametrize("h,w,s", [(60, 80, 1), (60, 80, 4), (240, 320, 8), (5, 7, 3), (3, 3, 8), (400, 400, 7)])
def test_lattice_count_formula(h, w, s):
    us, vs = VO.lattice(h, w, s)
    assert VO.lattice_count(h, w, s) == len(us) * len(vs)
    assert (len(us) == 0 or us[-1] < w) and (len(vs) == 0 or vs[-1] < h)


def test_lattice_candidates_are_seeded_and_in_bounds():
    from gennbv_amd.eval.baselines import LatticeCandidates
    a, b, c = (LatticeCandidates(CFG, 9, s) for s in (3, 3, 4))
    x, y, z = a.sample(5), b.sample(5), c.sample(5)
    assert x.shape == (5, 9, 6) and x.dtype == torch.int64
    assert torch.equal(x, y) and not torch.equal(x, z)
    assert not torch.equal(a.sample(5), x) and torch.equal(a.sample(5), [b.sample(5), b.sample(5)][1])
    lo, up = torch.tensor(CFG.clip_pose_idx_low), torch.tensor(CFG.clip_pose_idx_up)
    for lc in (a, LatticeCandidates(CFG, 9, 1, look_at_scene=True)):
        s = lc.sample(50)
        assert bool((s >= lo).all()) and bool((s <= up).all())
    assert torch.equal(a.poses(x), S.poses_from_actions(x, CFG).float())


def test_choose_scores_breaks_ties_low_and_masks_contacts():
    from gennbv_amd.eval.baselines import choose
    gain = torch.tensor([[[10, 0, 0], [2, 2, 1], [2, 2, 1], [0, 3, 1]],   # scores 10, 10, 10, 12 -> 3
                         [[4, 1, 0], [8, 0, 0], [0, 2, 0], [1, 0, 0]],   # scores 8, 8, 8, 1 -> 0 (tie: lowest)
                         [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]], dtype=torch.int32)
    assert choose(gain, (1, 4)).tolist() == [3, 0, 0]
    contact = torch.tensor([[0, 0, 0, 1], [1, 0, 0, 0], [1, 1, 0, 4]], dtype=torch.uint8)
    assert choose(gain, (1, 4), contact).tolist() == [0, 1, 2]
    assert choose(gain, (1, 4), torch.ones(3, 4, dtype=torch.uint8)).tolist() == [0, 0, 0]  # all collide: -1 everywhere
    assert choose(gain, (1, 0)).tolist() == [0, 1, 0]


class _Mesh:
    def collide(self, poses, body, out=None):
        out.copy_((poses[:, 2] < 3.0).to(torch.uint8))  # "everything below 3 m collides"
        return out


class _Env:
    def __init__(self, n, collision):
        self.cfg, self.num_envs, self.device = CFG, n, torch.device("cpu")
        self.collision, self.collision_mesh = collision, _Mesh()


def test_greedy_policy_with_the_oracle_backend():
    from gennbv_amd.eval.baselines import GreedyGainPolicy, LatticeCandidates, choose
    n, k = 2, 6
    sc = _scene(n)
    kinv = S.inverse_intrinsics(H, W, CFG.horizontal_fov).numpy()

    def backend(tri, poses):
        c2w = S.camera_to_world(poses.view(-1, 6)).float().view(n, k, 4, 4).numpy()
        return torch.from_numpy(VO.view_gain(tri.to(torch.int8).numpy(), c2w, sc.range_gt.numpy(), sc.voxel_size.numpy(), kinv, H, W, 4, 50.0))
    obs = torch.zeros(n, CFG.obs_dim)
    grid = torch.zeros(n, G, G, G)
    grid[:, 6:10, 6:10, 0:6] = 1.0
    grid[:, :, :, 12:] = -1.0
    obs[:, CFG.state_dim:CFG.state_dim + CFG.grid_dim] = grid.view(n, -1)
    for collision in (None, object()):
        pol = GreedyGainPolicy(_Env(n, collision), k=k, seed=5, gain_backend=backend)
        actions, _, _ = pol.policy(obs, deterministic=True)
        cand = LatticeCandidates(CFG, k, 5).sample(n)
        gain = pol.last_gain
        score = gain[..., 0].long() + 4 * gain[..., 1].long()
        assert int(score.max()) > 0
        if collision is not None:
            hit = S.poses_from_actions(cand, CFG)[..., 2] < 3.0
            assert bool(hit.any()) and not bool(hit.all(1).any())
            score = torch.where(hit, torch.full_like(score, -1), score)
        want = torch.stack([cand[e, int(torch.nonzero(score[e] == score[e].max())[0])] for e in range(n)])
        assert torch.equal(actions, want)
        assert actions.dtype == torch.int64 and actions.shape == (n, 6)


def test_random_policy_speaks_the_evaluation_protocol():
    from gennbv_amd.eval.baselines import RandomLatticePolicy
    p = RandomLatticePolicy(CFG, 3, seed=2)
    a, x, y = p.policy(torch.zeros(3, 4), deterministic=True)
    assert a.shape == (3, 6) and a.dtype == torch.int64 and x is None and y is None
    assert bool((a <= torch.tensor(CFG.clip_pose_idx_up)).all()) and bool((a >= 0).all())
    assert not torch.equal(p.policy(torch.zeros(3, 4))[0], a)


def test_view_gain_refuses_cpu_and_large_grids():
    from gennbv_amd import _lib
    from gennbv_amd.ops.view_gain import ViewGain
    sc = _scene()
    with pytest.raises(_lib.GennbvHipError):
        ViewGain(1, 4, CFG, sc.range_gt, sc.voxel_size, device="cpu")

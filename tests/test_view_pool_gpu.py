"""GPU: gnbv_view_cover_masks (csrc/viewcover.hip) against gnbv_view_cover, one candidate at a time; ViewPool and
PoolCoverPolicy (ops/view_pool.py, eval/baselines.py) in the closed loop.  Every comparison is `==` on integers.
(The scene and env builders follow tests/test_view_cover_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import cover_greedy_oracle as CG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANGE = [5.0, -5.0, 5.0, -5.0, 8.0, 0.0]  # the explicit voxel frame of the hand-made meshes
H, W = 60, 80


def _cfg(g, h=H, w=W):
    return TaskConfig(camera_width=w, camera_height=h, grid_size=g)


def _u32(bits):
    return np.ascontiguousarray(bits.cpu().numpy()).view(np.uint32)


def _bool_to_bits(mask, words):
    """bool [N, g^3] -> int32 [N, words] on the device"""
    out = np.zeros((mask.shape[0], words * 4), np.uint8)
    p = np.packbits(mask.astype(np.uint8), axis=1, bitorder="little")
    out[:, :p.shape[1]] = p
    return torch.from_numpy(out.view(np.int32).copy()).to(DEV)


def _look_at_poses(cfg, n, k, seed):
    from gennbv_amd.eval.baselines import LatticeCandidates
    lc = LatticeCandidates(cfg, k, seed, look_at_scene=True)
    a = lc.sample(n)
    return a, lc.poses(a)


def _mixed_mesh(n):
    """A box under a sphere, a UV sphere, no triangles at all[, a randomly rotated box]: the first n of them."""
    from gennbv_amd.env.mesh_scene import MeshScene, box_triangles, random_rotation, sphere_triangles
    gen = torch.Generator().manual_seed(5)
    sph = sphere_triangles([0.5, -0.3, 3.0], 2.0, 12, 24)
    half = torch.tensor([[1.5, 1.0, 2.0]], dtype=torch.float64)
    rot = (box_triangles(-half, half).double() @ random_rotation(gen).T + torch.tensor([0.0, 0.5, 3.5], dtype=torch.float64)).float()
    box = box_triangles(torch.tensor([[-2.0, -1.0, 0.0]]), torch.tensor([[1.0, 2.0, 2.5]]))
    top = sphere_triangles([0.0, 0.5, 4.0], 1.2, 8, 16)
    one = lambda m, v: torch.full((m,), v, dtype=torch.int32)
    tris = [torch.cat([box, top]), torch.zeros(0, 3, 3), sph, rot][:n]
    ids = [torch.cat([one(12, 1), one(top.shape[0], 2)]), torch.zeros(0, dtype=torch.int32), one(sph.shape[0], 1), one(12, 2)][:n]
    return MeshScene.from_triangles(tris, ids, device=DEV)


def _mesh_and_frame(kind, n, g):
    from gennbv_amd.env.mesh_scene import MeshScene
    if kind == "boxes":
        sc = S.make_scenes(n, g, seed=3)
        return MeshScene.from_boxes(sc, device=DEV), sc.range_gt, sc.voxel_size
    mesh = _mixed_mesh(n)
    rng, vox = mesh.grid_spec(g, torch.tensor([RANGE] * n))
    return mesh, rng, vox


# ("mixed", 128): two windows of the bit set
@pytest.mark.parametrize("kind,g,n", [("boxes", 20, 3), ("mixed", 33, 3), ("boxes", 64, 3), ("mixed", 128, 2)])
def test_masks_equal_view_cover_of_each_candidate_alone(kind, g, n):
    from gennbv_amd import _lib
    from gennbv_amd.ops.view_cover import ViewCover
    from gennbv_amd.ops.view_pool import ViewPool
    k = 5
    cfg = _cfg(g)
    mesh, rng, vox = _mesh_and_frame(kind, n, g)
    assert mesh.num_envs == n
    poses = _look_at_poses(cfg, n, k, seed=g)[1].to(DEV)
    one, all_k = ViewCover(mesh, cfg, rng, vox, 1), ViewCover(mesh, cfg, rng, vox, k)
    words = one.words
    gen = np.random.RandomState(g)
    gt = _bool_to_bits(gen.rand(n, g ** 3) < 0.6, words)
    # the reference, computed once: each candidate alone through gnbv_view_cover; a mid-episode scanned set from two other views
    want = torch.stack([one.accumulate(poses[:, j:j + 1].contiguous(), gt, torch.zeros_like(gt)) for j in range(k)], 1)
    earlier = torch.cat([_look_at_poses(cfg, n, 2, seed=g + 1)[1].to(DEV), poses[:, :1]], 1).contiguous()  # (candidate 0 adds nothing)
    scanned = ViewCover(mesh, cfg, rng, vox, 3).accumulate(earlier, gt, torch.zeros_like(gt))
    cover = all_k(poses, gt, scanned).clone()
    union = all_k.accumulate(poses, gt, torch.zeros_like(gt))
    assert int(cover[..., 0].sum()) > 0 and bool((cover[..., 0] < cover[..., 1]).any())
    if kind == "mixed":
        assert int(cover[1].sum()) == 0  # the env without triangles: all-zero masks

    small = 64 if g < 128 else 4096  # a forced small window: 4 windows at 20^3, 128 at 64^3, 16 at 128^3
    for chunk, window, batch in ((0, 0, 64), (1, 0, 2), (2, 0, 64), (0, small, 3)):
        pool = ViewPool(mesh, cfg, rng, vox, gt, poses, batch=batch, chunk=chunk, window=window)
        tag = (kind, g, chunk, window, batch)
        assert pool.masks.shape == (n, k, words) and torch.equal(pool.masks, want), tag
        assert torch.equal(pool.union_bits(), union), tag
        m = _u32(pool.masks)
        pad = np.unpackbits(m.view(np.uint8), axis=-1, bitorder="little")[..., g ** 3:]
        assert pad.shape[-1] == words * 32 - g ** 3 and not pad.any(), tag
        assert np.array_equal(CG.popcount(m & ~_u32(scanned)[:, None, :]), cover[..., 0].cpu().numpy()), tag
        assert np.array_equal(CG.popcount(m), cover[..., 1].cpu().numpy()), tag
        assert torch.equal(pool.gains(scanned), cover[..., 0]) and torch.equal(pool.gains(None), cover[..., 1]), tag

    # cover and seen_bits from the same call, into garbage-prefilled masks
    lib, sc = _lib.load(), mesh.c_struct()
    a = _lib.GnbvViewCover()
    C.memmove(C.byref(a), C.byref(all_k._args), C.sizeof(a))
    masks = torch.full((n, k, words), -12345, dtype=torch.int32, device=DEV)
    cover_b, seen_b = torch.full_like(cover, -1), torch.zeros_like(gt)
    a.poses, a.gt_bits, a.scanned_bits, a.cover, a.seen_bits = poses.data_ptr(), gt.data_ptr(), scanned.data_ptr(), cover_b.data_ptr(), seen_b.data_ptr()
    st = _lib.stream_ptr(torch.device(DEV))
    assert lib.gnbv_view_cover_masks(C.byref(sc), C.byref(a), masks.data_ptr(), st) == 0
    assert torch.equal(masks, want) and torch.equal(cover_b, cover) and torch.equal(seen_b, union)
    a.seen_bits = None  # cover alone
    masks.fill_(-777)
    cover_b.fill_(-1)
    assert lib.gnbv_view_cover_masks(C.byref(sc), C.byref(a), masks.data_ptr(), st) == 0
    assert torch.equal(masks, want) and torch.equal(cover_b, cover)
    # refusals: a NULL or misaligned mask row, and what gnbv_view_cover refuses
    assert lib.gnbv_view_cover_masks(C.byref(sc), C.byref(a), None, st) == 1
    assert lib.gnbv_view_cover_masks(C.byref(sc), C.byref(a), masks.data_ptr() + 4, st) == 1
    a.g = 129
    assert lib.gnbv_view_cover_masks(C.byref(sc), C.byref(a), masks.data_ptr(), st) == 1
    torch.cuda.synchronize()
    assert torch.equal(masks, want)  # nothing was launched


def _closed_env(n=4, g=20, max_len=50, seed=1, eval_env=False, collision=None):
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv
    cfg = _cfg(g)
    base = S.make_scenes(n, g, seed=seed)
    feed = RenderFeed(MeshScene.from_boxes(base, device=DEV), cfg)
    env = (ReplayFeedEvalEnv if eval_env else ReplayFeedEnv)(cfg, base, feed, DEV, max_episode_length=max_len, collision=collision)
    return env, cfg, base


def test_pool_policy_predicts_the_step_it_takes():
    from gennbv_amd.eval.baselines import PoolCoverPolicy, choose
    from gennbv_amd.ops.view_cover import ViewCover
    n, p = 4, 24
    env, cfg, _ = _closed_env(n=n)
    pol = PoolCoverPolicy(env, pool_size=p, seed=7)
    u = env.updater
    vc = ViewCover(env.feed.mesh, cfg, u.range_gt, u.voxel_size_gt, p, inv_intrinsics=u.inv_intri_host)
    rows = torch.arange(n, device=DEV)
    obs = env.reset()
    total = 0
    for step in range(6):
        a = pol(obs)[0]
        gain, choice = pol.last_gain.clone(), pol.last_choice.clone()
        cover = vc(pol.pool.poses, u.gt_bits, u.scanned_bits)  # the same poses, traced again
        assert torch.equal(gain, cover[..., 0].max(1).values) and torch.equal(choice.long(), choose(cover, (1, 0)))
        assert torch.equal(a, pol.pool_actions[rows, choice.long()]) and a.dtype == torch.int64
        before = u.coverage_count.clone()
        obs, _, dones, _ = env.step(a)
        assert not bool(dones.any())  # no env was reset: every env's prediction holds
        inc = u.coverage_count - before
        print("step", step, "predicted", gain.tolist(), "realised", inc.tolist())
        assert torch.equal(inc.to(torch.int32), gain)
        total += int(inc.sum())
    assert total > 0


def test_persistent_bounds_change_nothing_across_episode_resets():
    from gennbv_amd.eval.baselines import PoolCoverPolicy
    n, p = 4, 24
    env_a, _, _ = _closed_env(n=n, max_len=5)
    env_b, _, _ = _closed_env(n=n, max_len=5)
    pol_a = PoolCoverPolicy(env_a, pool_size=p, seed=3, persistent_bounds=True)
    pol_b = PoolCoverPolicy(env_b, pool_size=p, seed=3, persistent_bounds=False)
    obs_a, obs_b = env_a.reset(), env_b.reset()
    finished = 0
    for step in range(12):
        a, b = pol_a(obs_a)[0], pol_b(obs_b)[0]
        assert torch.equal(a, b), step
        assert torch.equal(pol_a.last_gain, pol_b.last_gain) and torch.equal(pol_a.last_choice, pol_b.last_choice), step
        obs_a, _, done_a, _ = env_a.step(a)
        obs_b, _, done_b, _ = env_b.step(b)
        assert torch.equal(done_a, done_b) and torch.equal(env_a.updater.scanned_bits, env_b.updater.scanned_bits)
        finished += int(done_a.sum())
    assert finished >= 2 * n  # every env restarted at least twice


def test_plan_replayed_in_the_env_pays_the_planned_gains():
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.eval.baselines import PoolCoverPolicy
    n, p, rounds = 4, 24, 6
    env, cfg, _ = _closed_env(n=n, collision=CollisionBody())
    pol = PoolCoverPolicy(env, pool_size=p, seed=5)
    assert pol.pool.contact is not None and pol.avoid_collisions
    env.reset()
    u = env.updater
    start = u.scanned_bits.clone()
    choice, gain, covered = (t.clone() for t in pol.plan(rounds))
    again = pol.plan(rounds, lazy=False)
    assert all(torch.equal(x, y) for x, y in zip((choice, gain, covered), again))  # lazy and exhaustive: the same plan
    assert torch.equal(u.scanned_bits, start)  # the plan does not touch the env's set
    contact = pol.pool.contact.cpu().numpy()
    want = CG.batch_exhaustive(_u32(pol.pool.masks), _u32(start), contact, rounds)
    assert np.array_equal(choice.cpu().numpy(), want[0]) and np.array_equal(gain.cpu().numpy(), want[1])
    assert np.array_equal(_u32(covered), want[2])
    rows = torch.arange(n, device=DEV)
    for t in range(rounds):
        before = u.coverage_count.clone()
        _, _, dones, _ = env.step(pol.pool_actions[rows, choice[:, t].long()])
        assert not bool(dones.any())  # surface ground truth: the coverage threshold cannot fire; no planned view collides
        inc = (u.coverage_count - before).to(torch.int32)
        print("round", t, "planned", gain[:, t].tolist(), "paid", inc.tolist())
        assert torch.equal(inc, gain[:, t])
    assert torch.equal(u.scanned_bits & u.gt_bits, covered)
    assert int(gain.sum()) > 0 and not bool((contact[np.arange(n)[:, None], choice.cpu().numpy()] != 0).any())


def _final_coverage(policy, env):
    """Mean over envs of env.coverage_ratio on each env's done step, and mean_AUC (tests/test_view_cover_gpu.py)."""
    from gennbv_amd.eval import evaluate_policy_grid_obs
    n = env.num_envs
    final = {}

    def cb(loc, _):
        i = loc["i"]
        if bool(loc["done"]) and i not in final:
            final[i] = float(env.coverage_ratio[i])
    _, _, auc, _ = evaluate_policy_grid_obs(policy, env, n_eval_episodes=n, callback=cb)
    assert len(final) == n
    return float(np.mean(list(final.values()))), float(auc.mean())


def test_pool_policy_beats_random_coverage_closed_loop():
    from gennbv_amd.eval.baselines import GreedyGainPolicy, OracleGainPolicy, PoolCoverPolicy, RandomLatticePolicy
    seed = 1
    envs = [_closed_env(n=8, max_len=20, eval_env=True) for _ in range(4)]
    cfg = envs[0][1]
    cp, ap = _final_coverage(PoolCoverPolicy(envs[0][0], pool_size=256, seed=seed), envs[0][0])
    cr, ar = _final_coverage(RandomLatticePolicy(cfg, 8, seed), envs[1][0])
    co, ao = _final_coverage(OracleGainPolicy(envs[2][0], k=32, seed=seed), envs[2][0])
    cg, ag = _final_coverage(GreedyGainPolicy(envs[3][0], k=32, weights=(1, 4), seed=seed), envs[3][0])
    print(f"final coverage pool(256) {cp:.4f} oracle {co:.4f} greedy {cg:.4f} random {cr:.4f}; "
          f"mean_AUC pool {ap:.4f} oracle {ao:.4f} greedy {ag:.4f} random {ar:.4f}")  # oracle and greedy: reported, not asserted
    assert cp > cr

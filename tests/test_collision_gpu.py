"""GPU: collision termination -- gnbv_collide_cylinder against the fp64 CPU oracle, gnbv_env_post_step_contacts, and the
closed-loop env with a CollisionBody (ReplayFeedEnv, ReplayFeedEvalEnv, PPO_Grid_Obs)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests.collision_oracle import GROUND, INSIDE, SURFACE, CollisionOracle, hand_cases
from tests.envstep_util import PostState as _PostState, contact_oracle_cls as _contact_oracle_cls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, H = 0.1, 0.02
f32 = np.float32


def _mesh(tris, ids):
    from gennbv_amd.env.mesh_scene import MeshScene
    return MeshScene.from_triangles([torch.as_tensor(t, dtype=torch.float32) for t in tris],
                                    [torch.as_tensor(i, dtype=torch.int32) for i in ids], device=DEV)


def _collide(mesh, poses, r=R, h=H, ground=False):
    from gennbv_amd.env.collision import CollisionBody
    p = torch.as_tensor(poses, dtype=torch.float32)
    if p.device.type != "cuda":
        p = p.to(DEV)
    return mesh.collide(p, CollisionBody(r, h, ground)).cpu().numpy()


def _test_scenes(seed=0):
    """Per env (triangles, ids): box scenes, randomly rotated boxes, spheres, degenerate triangles beside a box, empty."""
    from gennbv_amd.env.mesh_scene import box_triangles, random_rotation, sphere_triangles
    gen = torch.Generator().manual_seed(seed)
    tris, ids = [], []
    sc = S.make_scenes(6, 20, seed=seed + 1)
    for e in range(6):
        ok = (sc.boxes_min[e] <= sc.boxes_max[e]).all(-1)
        k = torch.nonzero(ok).flatten()
        tris.append(box_triangles(sc.boxes_min[e, k], sc.boxes_max[e, k]))
        ids.append((k.int() + 1).repeat_interleave(12))
    for e in range(4):  # rotated boxes
        parts, pid = [], []
        for b in range(4):
            half = 0.3 + 1.5 * torch.rand(3, generator=gen, dtype=torch.float64)
            q = random_rotation(gen)
            c = torch.cat([(torch.rand(2, generator=gen, dtype=torch.float64) - 0.5) * 10, 1.0 + 4 * torch.rand(1, generator=gen, dtype=torch.float64)])
            t = box_triangles(-half[None], half[None]).double()
            parts.append((t @ q.T + c).float())
            pid.append(torch.full((12,), b + 1, dtype=torch.int32))
        tris.append(torch.cat(parts))
        ids.append(torch.cat(pid))
    for e in range(2):  # spheres
        s1 = sphere_triangles((0.0, 0.0, 3.0), 1.5)
        s2 = sphere_triangles((3.0, -2.0, 2.0), 0.7, 8, 16)
        tris.append(torch.cat([s1, s2]))
        ids.append(torch.cat([torch.full((s1.shape[0],), 1), torch.full((s2.shape[0],), 2)]).int())
    # degenerate triangles (segments, points, slivers) beside a closed box
    box = box_triangles(torch.tensor([[1.0, 1.0, 0.0]]), torch.tensor([[2.5, 2.0, 1.5]]))
    p = (torch.rand(30, 3, generator=gen) - 0.5) * 6 + torch.tensor([0.0, 0.0, 3.0])
    d = (torch.rand(30, 3, generator=gen) - 0.5)
    segs = torch.stack([p, p + d, p + d], 1)
    pts = torch.stack([p, p, p], 1)
    sliv = torch.stack([p, p + d, p + 2 * d], 1)
    tris.append(torch.cat([box, segs, pts, sliv]))
    ids.append(torch.cat([torch.full((12,), 1), torch.full((90,), 5)]).int())
    tris.append(torch.zeros(0, 3, 3))
    ids.append(torch.zeros(0, dtype=torch.int32))
    return tris, ids


def _near_surface_poses(tris, k, gen, lattice):
    """k poses near random triangles of one env: a point on the triangle offset along its normal by [-0.15, 0.15] m."""
    rs = np.random.RandomState(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen)))
    t = np.asarray(tris, np.float64)
    out = np.zeros((k, 6), f32)
    if t.shape[0]:
        j = rs.randint(0, t.shape[0], k)
        u, v = rs.rand(k), rs.rand(k)
        flip = u + v > 1
        u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
        q = t[j]
        pt = q[:, 0] + u[:, None] * (q[:, 1] - q[:, 0]) + v[:, None] * (q[:, 2] - q[:, 0])
        nrm = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
        ln = np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1), rs.randn(k, 3) / math.sqrt(3))
        out[:, :3] = pt + nrm * rs.uniform(-0.15, 0.15, (k, 1))
    else:
        out[:, :3] = rs.uniform(-3, 3, (k, 3))
    if lattice:  # every lattice pitch / yaw of the task, roll 0
        cfg = TaskConfig()
        pk, yk = rs.randint(0, 13, k), rs.randint(0, 13, k)
        out[:, 4] = (pk.astype(f32) * f32(cfg.action_unit[4]) + f32(cfg.clip_pose_low[4])).astype(f32)
        out[:, 5] = (yk.astype(f32) * f32(cfg.action_unit[5]) + f32(cfg.clip_pose_low[5])).astype(f32)
    else:
        out[:, 3:6] = rs.uniform(-math.pi, math.pi, (k, 3))
    return out


def _compare(oracle, mesh, env_idx, poses_np, codes, r=R, h=H, ground=False, min_robust=0.97):
    want, robust = oracle.robust_codes(env_idx, poses_np, r, h, ground)
    bad = np.nonzero(robust & (want != codes))[0]
    assert bad.size == 0, [(int(env_idx[i]), poses_np[i].tolist(), int(codes[i]), int(want[i])) for i in bad[:5]]
    assert robust.mean() >= min_robust, robust.mean()
    return want


def test_hand_cases_on_the_kernel():
    for name, tris, ids, pose, r, h, ground, expected in hand_cases():
        mesh = _mesh([tris], [ids])
        assert int(_collide(mesh, [pose], float(f32(r)), float(f32(h)), ground)[0]) == expected, name


def test_kernel_matches_oracle_on_20k_placements():
    tris, ids = _test_scenes()
    mesh = _mesh(tris, ids)
    oracle = CollisionOracle.from_mesh(mesh)
    n = mesh.num_envs
    gen = torch.Generator().manual_seed(11)
    k = 240  # placements per env per batch, half of them with the ground
    counts = np.zeros(3, np.int64)
    total = 0
    for batch in range(6):
        lattice = batch % 2 == 1
        per_env = [_near_surface_poses(tris[e].numpy(), k, gen, lattice) for e in range(n)]
        for ground in (False, True):
            env_idx, ps, got = [], [], []
            for c in range(k // 2):  # one pose per env per call, row stride 8
                i = c * 2 + int(ground)
                buf = torch.zeros(n, 8, dtype=torch.float32)
                buf[:, :6] = torch.from_numpy(np.stack([per_env[e][i] for e in range(n)]))
                buf[:, 6:] = float("nan")  # never read
                code = _collide(mesh, buf.to(DEV)[:, :6], ground=ground)
                env_idx.append(np.arange(n))
                ps.append(buf[:, :6].numpy())
                got.append(code)
            env_idx, ps, got = np.concatenate(env_idx), np.concatenate(ps), np.concatenate(got)
            want = _compare(oracle, mesh, env_idx, ps, got, ground=ground)
            total += got.size
            counts += [(want & SURFACE != 0).sum(), (want & INSIDE != 0).sum(), (want & GROUND != 0).sum()]
    assert total >= 20000, total
    assert (counts >= 200).all(), counts


def test_edge_cases():
    tris, ids = _test_scenes(seed=4)
    mesh = _mesh(tris, ids)
    oracle = CollisionOracle.from_mesh(mesh)
    n = mesh.num_envs
    rs = np.random.RandomState(5)
    # bodies exactly on cell boundaries (cell corners of each env's grid), random axes
    lo, size, res = mesh.cell_lo.cpu().numpy(), mesh.cell_size.cpu().numpy(), mesh.cell_res.cpu().numpy()
    for rep in range(40):
        p = np.zeros((n, 6), f32)
        p[:, 3:6] = rs.uniform(-math.pi, math.pi, (n, 3))
        ijk = rs.randint(0, np.maximum(res, 1) + 1)
        p[:, :3] = (lo + ijk.astype(f32) * size).astype(f32)
        _compare(oracle, mesh, np.arange(n), p, _collide(mesh, p, ground=bool(rep % 2)), ground=bool(rep % 2), min_robust=0.9)
    # bodies outside the env's cell grid: free (the ground bit aside)
    p = np.zeros((n, 6), f32)
    p[:, 0] = 60.0 + rs.uniform(0, 5, n)
    p[:, 2] = rs.uniform(-0.5, 0.5, n)
    p[:, 4] = 0.3
    for g in (False, True):
        code = _collide(mesh, p, ground=g)
        assert np.array_equal(code, oracle.codes(np.arange(n), p, R, H, g))
        assert ((code & (SURFACE | INSIDE)) == 0).all()
    # big body overlapping many cells (more than 64: the chunked candidate walk)
    p = np.zeros((n, 6), f32)
    p[:, :3] = rs.uniform(-2, 2, (n, 3)).astype(f32) + f32([0, 0, 2])
    _compare(oracle, mesh, np.arange(n), p, _collide(mesh, p, 3.0, 2.5), 3.0, 2.5, min_robust=0.8)
    # the env without triangles
    assert tris[-1].shape[0] == 0
    p = _near_surface_poses(tris[0].numpy(), n, torch.Generator().manual_seed(1), False)
    p[-1, 2] = 0.01
    assert _collide(mesh, p)[-1] == 0 and _collide(mesh, p, ground=True)[-1] == GROUND
    # two calls byte-equal; a strided pose view equals the contiguous copy
    big = torch.from_numpy(rs.uniform(-1, 1, (n, 9)).astype(f32)).to(DEV)
    big[:, :3] *= 5
    big[:, 2] += 3
    a1 = _collide(mesh, big[:, :6])
    a2 = _collide(mesh, big[:, :6])
    a3 = _collide(mesh, big[:, :6].contiguous())
    assert a1.tobytes() == a2.tobytes() == a3.tobytes()
    # non-positive or non-finite bodies are refused by the C entry point as well
    from gennbv_amd import _lib
    sc, ob = mesh.c_struct(), mesh.objects_c_struct()
    out = torch.zeros(n, dtype=torch.uint8, device=DEV)
    lib = _lib.load()
    for r, h in ((0.0, 0.02), (0.1, -0.01), (float("nan"), 0.02)):
        assert lib.gnbv_collide_cylinder(C.byref(sc), C.byref(ob), big.data_ptr(), 9, r, h, 0, out.data_ptr(), None) != 0
    assert lib.gnbv_collide_cylinder(C.byref(sc), C.byref(ob), big.data_ptr(), 5, 0.1, 0.02, 0, out.data_ptr(), None) != 0


@pytest.mark.parametrize("n", [1, 5, 257])
def test_env_counts(n):
    from gennbv_amd.env.mesh_scene import MeshScene
    scene = S.make_scenes(n, 20, seed=n)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    oracle = CollisionOracle.from_mesh(mesh)
    gen = torch.Generator().manual_seed(n)
    codes, poses = [], []
    for rep in range(max(1, 600 // n)):
        p = np.stack([_near_surface_poses(mesh.env_triangles(e)[0].cpu().numpy(), 1, gen, rep % 2 == 0)[0] for e in range(n)])
        poses.append(p)
        codes.append(_collide(mesh, p, ground=True))
    _compare(oracle, mesh, np.tile(np.arange(n), len(poses)), np.concatenate(poses), np.concatenate(codes), ground=True, min_robust=0.95)


# ---------------------------------------------------------------------------
# post-step with contacts
# ---------------------------------------------------------------------------
def test_post_step_contacts_null_and_zero_equal_the_plain_kernel_and_random_contacts_equal_the_oracle():
    from gennbv_amd import _lib
    lib = _lib.load()
    n, L = 300, 7
    cfg = TaskConfig(grid_size=4)
    base = _PostState(n, cfg, L, seed=1)
    plain, null, zero = base.clone(), base.clone(), base.clone()
    zeros = torch.zeros(n, dtype=torch.uint8, device=DEV)
    g = [torch.Generator().manual_seed(2) for _ in range(3)]
    resets = 0
    for s in range(35):
        for st, gg in zip((plain, null, zero), g):
            st.advance(gg)
        _lib.check(lib.gnbv_env_post_step(C.byref(plain.struct()), None), "plain")
        _lib.check(lib.gnbv_env_post_step_contacts(C.byref(null.struct()), None, None), "null")
        _lib.check(lib.gnbv_env_post_step_contacts(C.byref(zero.struct()), zeros.data_ptr(), None), "zero")
        ref = plain.snapshot()
        assert null.snapshot() == ref and zero.snapshot() == ref, f"step {s}"
        resets += int(plain.dones.sum())
    assert resets > n

    # random contacts vs the oracle restatement (rewards, dones, time-outs, ratios, prev_ratio, episode lengths)
    Oracle = _contact_oracle_cls()
    st = _PostState(n, cfg, L, seed=3)
    g = torch.Generator().manual_seed(4)
    o = Oracle(cfg, np.eye(3, dtype=f32), np.zeros((n, 6), f32), np.ones((n, 3), f32), np.zeros((n, 4, 4, 4), f32),
               st.num_valid.cpu().numpy(), max_episode_length=L)
    o.episode_length_buf = st.episode_length_buf.cpu().numpy().copy()
    seen = 0
    for s in range(35):
        st.advance(g)
        o.episode_length_buf += 1
        contact = (torch.rand(n, generator=g) < 0.15).to(torch.uint8) * torch.randint(1, 8, (n,), generator=g).to(torch.uint8)
        c_dev = contact.to(DEV)
        _lib.check(lib.gnbv_env_post_step_contacts(C.byref(st.struct()), c_dev.data_ptr(), None), "contacts")
        o.contact = contact.numpy()
        rew, reset, time_out, ratio = o._reward_done(st.coverage_count.cpu().numpy())
        assert st.rewards.cpu().numpy().tobytes() == rew.tobytes(), f"step {s}"
        assert np.array_equal(st.dones.cpu().numpy().astype(bool), reset) and np.array_equal(st.step_time_out.cpu().numpy().astype(bool), time_out)
        assert st.coverage_ratio.cpu().numpy().tobytes() == ratio.tobytes()
        o.prev_ratio = np.where(reset, f32(0), ratio).astype(f32)
        o.episode_length_buf[reset] = 0
        assert st.prev_ratio.cpu().numpy().tobytes() == o.prev_ratio.tobytes()
        assert np.array_equal(st.episode_length_buf.cpu().numpy(), o.episode_length_buf)
        seen += int((reset & ~time_out & (o.contact != 0)).sum())
    assert seen > 100


# ---------------------------------------------------------------------------
# the env
# ---------------------------------------------------------------------------
def _closed_env(n=8, h=48, w=64, g=20, max_len=6, seed=3, eval_env=False, body=None):
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=seed)
    feed = RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg)
    cls = ReplayFeedEvalEnv if eval_env else ReplayFeedEnv
    return cls(cfg, scene, feed, DEV, max_episode_length=max_len, collision=CollisionBody() if body is None else body), cfg, scene


def _random_actions(cfg, n, gen):
    return torch.stack([torch.randint(0, int(u) + 1, (n,), generator=gen) for u in cfg.clip_pose_idx_up], -1).to(DEV)


def test_closed_loop_with_collisions_equals_the_oracle_env():
    n, steps, L = 8, 36, 40  # (episodes end by collisions, not by the time limit)
    env, cfg, scene = _closed_env(n=n, max_len=L)
    assert env.collision_buf.shape == (n,) and env.collision_mesh is env.feed.mesh
    gen = torch.Generator().manual_seed(1)
    acts = [_random_actions(cfg, n, gen) for _ in range(steps)]
    outs = [env.reset().cpu().numpy()]
    frames = [tuple(None if x is None else x.cpu().numpy() for x in env.feed.last)]
    codes = [env.collision_buf.cpu().numpy()]
    rews, dones = [], []
    for a in acts:
        o, r, d, _ = env.step(a)
        outs.append(o.cpu().numpy())
        rews.append(r.cpu().numpy())
        dones.append(d.cpu().numpy())
        frames.append(tuple(None if x is None else x.cpu().numpy() for x in env.feed.last))
        codes.append(env.collision_buf.cpu().numpy())
    Oracle = _contact_oracle_cls()
    upd = env.updater
    o = Oracle(cfg, upd.inv_intri_host.numpy(), upd.range_gt.cpu().numpy(), upd.voxel_size_gt.cpu().numpy(), upd.grid_gt.cpu().numpy(),
               env.num_valid_voxel_gt.cpu().numpy(), max_episode_length=L)
    o.collider = (CollisionOracle.from_mesh(env.feed.mesh), R, H, False)
    obs0 = o.reset(*frames[0])
    assert obs0.tobytes() == outs[0].tobytes()
    assert np.array_equal(o.contact, codes[0])
    s_term = f32(cfg.scale_termination * cfg.dt)
    assert s_term > 0
    by = {SURFACE: 0, INSIDE: 0}
    for k, a in enumerate(acts):
        obs, rew, reset, info = o.step(a.cpu().numpy(), *frames[k + 1])
        assert np.array_equal(o.contact, codes[k + 1]), f"step {k}: collision codes"
        assert obs.tobytes() == outs[k + 1].tobytes(), f"step {k}: observation"
        assert rew.tobytes() == rews[k].tobytes(), f"step {k}: rewards"
        assert np.array_equal(reset, dones[k]), f"step {k}: dones"
        for bit in by:
            hit = ((codes[k + 1] & bit) != 0) & ~o.time_out
            # (the rewards are bit-identical to the oracle's, whose sum holds this termination term)
            assert dones[k][hit].all() and (o.term[hit] == s_term).all(), f"step {k}: a collision must end the episode with the reward"
            by[bit] += int(hit.sum())
    assert by[SURFACE] >= 1 and by[INSIDE] >= 1, by


def _inside_action(cfg, mesh, e, want=INSIDE):
    """A lattice action whose pose lies in env e's solids (code `want`), found with the oracle."""
    o = CollisionOracle.from_mesh(mesh)
    unit, low = np.array(cfg.action_unit, f32), np.array(cfg.clip_pose_low, f32)
    rs = np.random.RandomState(e)
    a = np.stack([rs.randint(0, int(u) + 1, 4000) for u in cfg.clip_pose_idx_up], -1)
    p = (a.astype(f32) * unit + low).astype(f32)
    c = o.codes(np.full(len(a), e), p, R, H)
    return a[np.nonzero(c == want)[0][0]]


def test_eval_env_ends_the_episode_at_the_collision_and_scores_it():
    n, L = 4, 20
    env, cfg, _ = _closed_env(n=n, max_len=L, eval_env=True)
    env.reset()
    free = torch.tensor([cfg.init_action] * n, dtype=torch.int64, device=DEV)
    _, _, d, _, acc = env.step(free)  # the init pose: free, no episode ends
    assert not d.any() and acc == {}
    a = free.clone()
    a[1] = torch.from_numpy(_inside_action(cfg, env.feed.mesh, 1)).to(DEV)
    _, _, d, _, acc = env.step(a)
    assert d.cpu().tolist() == [False, True, False, False]
    assert int(env.collision_buf[1]) == INSIDE
    assert list(acc) == ["1"] and np.isfinite(acc["1"]) and acc["1"] >= 0
    assert float(env.episode_info()["rew_termination"]) > 0  # the ended episode's sums, logged at its reset


def test_open_loop_feed_needs_a_collision_mesh():
    from gennbv_amd import _lib
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.replay_feed import ReplayFeed, ReplayFeedEnv
    n = 4
    cfg = TaskConfig(camera_width=64, camera_height=48, grid_size=16)
    scene = S.make_scenes(n, 16, seed=2)
    feed = ReplayFeed.synthetic(scene, cfg, 2, seed=1)
    feed = ReplayFeed(*[None if x is None else x.to(DEV) for x in (feed.depth_raw, feed.seg_raw, feed.rgba, feed.c2w)])
    with pytest.raises(_lib.GennbvHipError):
        ReplayFeedEnv(cfg, scene, feed, DEV, collision=CollisionBody())
    mesh = MeshScene.from_boxes(scene, device=DEV)
    env = ReplayFeedEnv(cfg, scene, feed, DEV, max_episode_length=50, collision=CollisionBody(), collision_mesh=mesh)
    env.reset()
    a = torch.tensor([cfg.init_action] * n, dtype=torch.int64, device=DEV)
    a[2] = torch.from_numpy(_inside_action(cfg, mesh, 2)).to(DEV)
    _, _, d, _ = env.step(a)
    assert d.cpu().tolist() == [False, False, True, False] and int(env.collision_buf[2]) == INSIDE


def test_ppo_learns_on_the_closed_loop_env_with_collisions():
    from gennbv_amd.network.hybrid_encoder import Hybrid_Encoder
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from gennbv_amd.sb3.ppo_grid_obs import PPO_Grid_Obs
    L = 8
    env, cfg, _ = _closed_env(n=16, h=64, w=64, g=20, max_len=L)
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
    lens = [float(e["episode_length"]) for e in algo.ep_info_buffer if e is not None and float(e["episode_length"]) > 0]
    assert lens and min(lens) < L, lens  # collisions end episodes before the time limit

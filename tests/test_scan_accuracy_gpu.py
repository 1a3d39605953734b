"""GPU: the reconstruction-accuracy metric on the device (gennbv_amd/eval/scan_accumulator.py, csrc/scan.hip) against the host
path (unique_rounded_points + reconstruction_accuracy_cm) and the fp64 oracle; the eval env's `accuracy="device"` path against
its default; and the stale ratios_accuracy regression of repeated evaluations on both paths."""

import numpy as np
import pytest
import torch

from gennbv_amd import _lib
from gennbv_amd import utils as U
from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from gennbv_amd.eval import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENSE = -50.0


def _acc(pc_gt, h, w, kinv, cap=None):
    from gennbv_amd.eval import ScanAccumulator
    return ScanAccumulator(len(pc_gt), pc_gt, h, w, kinv, SENSE, capacity_per_env=cap, device=DEV)


def _host_points(frame, kinv):
    """The host path's per-env foreground points of one frame (A1 + A2 standalone kernels)."""
    depth_raw, seg_raw, c2w = frame
    d, s = U.post_process_depth(depth_raw, seg_raw, SENSE)
    return U.back_projection_fg(d, s, c2w, kinv)


def _poses_c2w(n, gen, spread=4.0, offset=(0.0, 0.0, 0.0)):
    poses = torch.zeros(n, 6)
    poses[:, :3] = (torch.rand(n, 3, generator=gen) - 0.5) * spread + torch.tensor(offset)
    poses[:, 4] = (torch.rand(n, generator=gen) - 0.5) * 1.0
    poses[:, 5] = (torch.rand(n, generator=gen) - 0.5) * 6.0
    return S.camera_to_world(poses).to(DEV, torch.float32).contiguous()


def _frame(n, h, w, gen, dmin=1.0, dmax=6.0, fg=0.7, spread=4.0, offset=(0.0, 0.0, 0.0)):
    depth = -(dmin + (dmax - dmin) * torch.rand(n, h, w, generator=gen))
    seg = torch.where(torch.rand(n, h, w, generator=gen) < fg, 255.0, 0.0)
    return depth.to(DEV), seg.to(DEV), _poses_c2w(n, gen, spread, offset)


def _ulps(a, b):
    ia = np.array([a], dtype=np.float32).view(np.int32)[0]
    ib = np.array([b], dtype=np.float32).view(np.int32)[0]
    return abs(int(ia) - int(ib))


def _check_scores(acc, frames_per_env, pc_gt, oracle=True):
    """Every scored env against reconstruction_accuracy_cm of the same points (<= 2 fp32 ulps: the scanned side is summed in
    Morton order) and against the fp64 oracle (1e-4 relative)."""
    from oracle import oracle as orc
    res = acc.results()
    for e, pts in frames_per_env.items():
        cloud = torch.cat(pts, 0)
        ref = float(M.reconstruction_accuracy_cm(cloud, pc_gt[e]))
        assert _ulps(res[e], ref) <= 2, (e, res[e], ref)
        if oracle:
            xr = M.unique_rounded_points(cloud).double().cpu().numpy()
            o = 100.0 * orc.chamfer_distance_ref(xr, pc_gt[e].double().cpu().numpy())
            assert abs(res[e] - o) <= 1e-4 * abs(o) + 1e-9, (e, res[e], o)
    return res


# ---------------------------------------------------------------------------
# the set
# ---------------------------------------------------------------------------
def test_set_equals_unique_rounded_points():
    n, h, w = 4, 24, 32
    gen = torch.Generator().manual_seed(0)
    kinv = S.inverse_intrinsics(h, w, 90.0)
    acc = _acc([torch.zeros(1, 3)] * n, h, w, kinv)
    f0 = _frame(n, h, w, gen)
    d, s, c = (x.clone() for x in f0)
    # special depths in foreground pixels: NaN -> 0, -inf -> 0, < -50 -> 50 (clamp), +inf only under background
    s[:, 0, :8] = 255.0
    d[:, 0, 0], d[:, 0, 1], d[:, 0, 2], d[:, 0, 3] = float("nan"), float("-inf"), -70.0, -50.0
    s[:, 1, 0], d[:, 1, 0] = 0.0, float("inf")
    s[:, 1, 1] = float("nan")  # NaN seg: background
    s[3] = 0.0  # env 3: background only
    f1 = (d, s, c)
    # half-centimetre ties and negative coordinates: axis-aligned camera, depths on exact half-cm values
    tie = torch.zeros(n, 4, 4, device=DEV)
    tie[:, :3, :3] = torch.eye(3, device=DEV)
    tie[:, 3, 3] = 1.0
    tie[:, :3, 3] = torch.tensor([-2.375, -0.125, -3.0], device=DEV)
    f2 = (-(torch.randint(0, 64, (n, h, w), generator=gen).float() * 0.25 + 0.125).to(DEV), f0[1].clone(), tie)  # z = d - 3: x.125 / x.375
    f2[1][3] = 0.0
    episodes = [[f1, f2, f1], [f2, f0, _frame(n, h, w, gen)], [_frame(n, h, w, gen, spread=30.0)]]
    for ep, frames in enumerate(episodes):
        pts = {e: [] for e in range(n)}
        for f in frames:
            acc.add_frame(*f)
            for e, p in enumerate(_host_points(f, kinv)):
                pts[e].append(p)
        counts = acc.counts.cpu()
        for e in range(n):
            ref = M.unique_rounded_points(torch.cat(pts[e], 0))
            got = acc.points(e)
            assert int(counts[e]) == ref.shape[0]
            assert got.shape == ref.shape and torch.equal(got.view(torch.int32), ref.view(torch.int32)), (ep, e)
        if ep == 0:
            assert int(counts[3]) == 0
            acc.score(torch.ones(n, dtype=torch.bool, device=DEV))
            assert acc.scored.cpu().tolist() == [1, 1, 1, 0]  # a background-only env produces no score
        acc.clear(torch.ones(n, dtype=torch.uint8, device=DEV))
        assert acc.counts.cpu().tolist() == [0] * n


# ---------------------------------------------------------------------------
# accuracy
# ---------------------------------------------------------------------------
def _run_case(pc_gt, frames, h, w, kinv, oracle=True):
    pc_gt = [p.to(DEV, torch.float32) for p in pc_gt]
    n = len(pc_gt)
    acc = _acc(pc_gt, h, w, kinv)
    pts = {e: [] for e in range(n)}
    for f in frames:
        acc.add_frame(*f)
        for e, p in enumerate(_host_points(f, kinv)):
            pts[e].append(p)
    acc.score(torch.ones(n, dtype=torch.uint8, device=DEV))
    res = _check_scores(acc, {e: p for e, p in pts.items() if sum(x.shape[0] for x in p)}, pc_gt, oracle)
    # scoring the same state again gives the same bits
    first = acc.accuracy_cm.clone()
    acc.scored.zero_()
    acc.score(torch.ones(n, dtype=torch.uint8, device=DEV))
    assert torch.equal(first.view(torch.int32), acc.accuracy_cm.view(torch.int32))
    return res


def test_accuracy_small_cases():
    h, w = 16, 16
    gen = torch.Generator().manual_seed(1)
    kinv = S.inverse_intrinsics(h, w, 90.0)
    n = 5
    f = _frame(n, h, w, gen, dmin=2.0, dmax=2.02)
    d, s, c = f
    s = s.clone()
    s[0] = 0.0
    s[0, 7, 7] = 255.0  # env 0: one scanned point
    s[1] = 0.0
    s[1, 4:10, 4:10] = 255.0  # env 1: a cloud of a few cm (one leaf)
    pts = _host_points((d, s, c), kinv)
    x1 = M.unique_rounded_points(pts[1])
    x2 = M.unique_rounded_points(pts[2])
    pc = [torch.tensor([[0.3, -0.2, 1.0]]),                                                 # 1-point GT
          x1[:20].cpu() + 0.004,                                                            # one leaf, near the scan
          torch.cat([x2.cpu() + torch.tensor([0.005, 0.0, 0.0]), x2.cpu() - torch.tensor([0.005, 0.0, 0.0])]),  # exact ties
          torch.cat([x2.cpu()[:50]] * 3),                                                   # duplicate GT points
          (torch.rand(300, 3, generator=gen) - 0.5) * 0.5 + torch.tensor([40.0, 0.0, 0.0])]  # scan far outside the GT box
    _run_case(pc, [(d, s, c)], h, w, kinv)


def test_accuracy_scene_sizes_and_far_queries():
    h, w = 32, 40
    gen = torch.Generator().manual_seed(2)
    kinv = S.inverse_intrinsics(h, w, 90.0)
    n = 4
    frames = [_frame(n, h, w, gen, dmin=0.5, dmax=16.0, spread=16.0) for _ in range(3)]
    # 16 m scenes; a whole-scene GT cloud against one frame (most GT points metres from the scan); a lattice GT whose points
    # lie on the leaves' boundaries and at exact distances from the 1 cm keys
    lat = torch.stack(torch.meshgrid(*[torch.arange(-7.68, 7.69, 1.28)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pc = [(torch.rand(2000, 3, generator=gen) - 0.5) * 16.0,
          (torch.rand(2500, 3, generator=gen) - 0.5) * torch.tensor([16.0, 16.0, 4.0]),
          lat,
          (torch.rand(1000, 3, generator=gen) - 0.5) * 32.0]
    _run_case(pc, frames[:1], h, w, kinv)
    _run_case(pc, frames, h, w, kinv)


# ---------------------------------------------------------------------------
# masked batch semantics
# ---------------------------------------------------------------------------
def test_masked_first_episode_kept_and_no_sync():
    n, h, w = 4, 16, 20
    gen = torch.Generator().manual_seed(3)
    kinv = S.inverse_intrinsics(h, w, 90.0)
    pc = [((torch.rand(500, 3, generator=gen) - 0.5) * 6.0).to(DEV) for _ in range(n)]
    acc = _acc(pc, h, w, kinv)
    f0, f1 = _frame(n, h, w, gen), _frame(n, h, w, gen)
    m0 = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device=DEV)
    m1 = torch.tensor([1, 1, 0, 0], dtype=torch.bool, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc.add_frame(*f0)
        acc.score(m0)
        acc.clear(m0)
        acc.add_frame(*f1)
        acc.score(m1)
        acc.clear(m1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    p0, p1 = _host_points(f0, kinv), _host_points(f1, kinv)
    assert acc.scored.cpu().tolist() == [1, 1, 1, 0]
    # env 0: its first episode (frame 0) is kept; env 1: frames 0 + 1; env 2: frame 0; env 3 unscored
    _check_scores(acc, {0: [p0[0]], 1: [p0[1], p1[1]], 2: [p0[2]]}, pc, oracle=False)
    assert set(acc.results()) == {0, 1, 2}


def test_overflow_and_out_of_range_raise():
    n, h, w = 2, 16, 16
    gen = torch.Generator().manual_seed(4)
    kinv = S.inverse_intrinsics(h, w, 90.0)
    pc = [torch.zeros(4, 3)] * n
    acc = _acc(pc, h, w, kinv, cap=64)
    f = _frame(n, h, w, gen, fg=1.0)
    acc.add_frame(*f)  # 256 distinct keys per env into 64 slots
    acc.score(torch.ones(n, dtype=torch.uint8, device=DEV))
    assert acc.scored.cpu().tolist() == [0, 0]
    with pytest.raises(_lib.GennbvHipError):
        acc.results()
    with pytest.raises(_lib.GennbvHipError):
        acc.points(0)
    acc2 = _acc(pc, h, w, kinv)
    far = _frame(n, h, w, gen, offset=(2.0e4, 0.0, 0.0))  # |rint(100 x)| >= 2^20
    acc2.add_frame(*far)
    with pytest.raises(_lib.GennbvHipError):
        acc2.results()
    acc3 = _acc(pc, h, w, kinv)
    d, s, c = _frame(n, h, w, gen, fg=1.0)
    d = d.clone()
    d[1, 3, 3] = float("inf")  # +inf depth under the foreground: non-finite point
    acc3.add_frame(d, s, c)
    with pytest.raises(_lib.GennbvHipError):
        acc3.results()


# ---------------------------------------------------------------------------
# the env
# ---------------------------------------------------------------------------
def _same_dicts(a, b):
    assert set(a) == set(b), (dict(a), dict(b))
    for k in a:
        assert _ulps(a[k], b[k]) <= 2, (k, a[k], b[k])


def _lockstep(env_h, env_d, acts):
    oh, od = env_h.reset(), env_d.reset()
    assert torch.equal(oh[0], od[0]) and oh[4] == {} and od[4] == {}
    ended = 0
    for a in acts:
        oh, od = env_h.step(a), env_d.step(a)
        for i in range(3):
            assert torch.equal(oh[i], od[i]), i
        ended += int(oh[2].sum())
        _same_dicts(oh[4], od[4])
    assert ended > 0
    return ended


def test_env_device_path_equals_host_path_replay_feed():
    from gennbv_amd.env.replay_feed import ReplayFeed
    from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv
    n, h, w, g, L = 3, 48, 64, 16, 3
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=6)
    feed = ReplayFeed.synthetic(scene, cfg, 4, seed=6)
    mk = lambda acc: ReplayFeedEvalEnv(cfg, scene, ReplayFeed(feed.depth_raw.to(DEV), feed.seg_raw.to(DEV), feed.rgba.to(DEV), feed.c2w.to(DEV)),
                                       DEV, max_episode_length=L, **({} if acc == "host" else {"accuracy": acc}))  # noqa: E731
    gen = torch.Generator().manual_seed(0)
    acts = [S.sample_actions(n, cfg, gen).to(DEV) for _ in range(9)]
    _lockstep(mk("host"), mk("device"), acts)


def _closed_env(accuracy, n=6, h=40, w=48, g=20, L=8, seed=3):
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=seed)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=L, pc_gt=mesh.surface_points(3000),
                            collision=CollisionBody(), accuracy=accuracy)
    return env, cfg


def _random_actions(cfg, n, gen):
    return torch.stack([torch.randint(0, int(u) + 1, (n,), generator=gen) for u in cfg.clip_pose_idx_up], -1).to(DEV)


def test_env_device_path_equals_host_path_closed_loop_with_collisions():
    env_h, cfg = _closed_env("host")
    env_d, _ = _closed_env("device")
    gen = torch.Generator().manual_seed(5)
    acts = [_random_actions(cfg, env_h.num_envs, gen) for _ in range(20)]
    _lockstep(env_h, env_d, acts)


class _SeededPolicy:
    def __init__(self, cfg, n, seed):
        self.cfg, self.n, self.gen = cfg, n, torch.Generator().manual_seed(seed)

    def policy(self, obs, deterministic=True):
        return _random_actions(self.cfg, self.n, self.gen), None, None


@pytest.mark.parametrize("accuracy", ["host", "device"])
def test_second_evaluation_reports_its_own_accuracies(accuracy):
    from gennbv_amd.eval import evaluate_policy_grid_obs
    env, cfg = _closed_env(accuracy)
    n = env.num_envs
    r1 = evaluate_policy_grid_obs(_SeededPolicy(cfg, n, 11), env, n_eval_episodes=n, return_AUC=False)
    r2 = evaluate_policy_grid_obs(_SeededPolicy(cfg, n, 12), env, n_eval_episodes=n, return_AUC=False)
    fresh, _ = _closed_env(accuracy)
    r3 = evaluate_policy_grid_obs(_SeededPolicy(cfg, n, 12), fresh, n_eval_episodes=n, return_AUC=False)
    assert r2[0] == r3[0] and r2[1] == r3[1]
    assert r2[3] == r3[3], (r1[3], r2[3], r3[3])
    assert r1[3] != r2[3]
    if accuracy == "device":
        host, _ = _closed_env("host")
        r4 = evaluate_policy_grid_obs(_SeededPolicy(cfg, n, 12), host, n_eval_episodes=n, return_AUC=False)
        assert r4[0] == r2[0] and r4[1] == r2[1] and len(r4[3]) == len(r2[3])
        assert all(_ulps(a, b) <= 2 for a, b in zip(r4[3], r2[3])), (r4[3], r2[3])

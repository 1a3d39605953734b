"""GPU: the swept flight path -- gnbv_sweep_sphere (csrc/sweep.hip) against the fp64 CPU oracle (tests/sweep_oracle.py),
MeshScene.sweep / sweep_candidates, the closed-loop env with CollisionBody(sweep=True) and the planners that avoid blocked
flights.  Wherever the oracle's answer is robust (the same at R -+ 1e-6 m) the kernel must give it bit for bit, and at least
99 % of every comparison's items must be robust."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import sweep_oracle as SO
from tests import test_collision_gpu as TC
from tests import test_view_pool_gpu as TP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
PATH, PATH_GROUND = SO.PATH, SO.PATH_GROUND
MIN_ROBUST = 0.99


def _body(ground=False, sweep=True, **kw):
    from gennbv_amd.env.collision import CollisionBody
    return CollisionBody(TC.R, TC.H, ground, sweep, **kw)


def _dev(x):
    return torch.as_tensor(np.asarray(x, f32)).to(DEV)


def _check(oracle, env_idx, a, b, got, body, episode_length=None):
    """got [M] against the oracle on its robust items; -> (want, robust)."""
    want, robust = oracle.robust_codes(env_idx, a, b, body.path_radius, body.ground, episode_length)
    bad = np.nonzero(robust & (want != got))[0]
    assert bad.size == 0, [(int(env_idx[i]), a[i].tolist(), b[i].tolist(), int(got[i]), int(want[i])) for i in bad[:5]]
    assert robust.mean() >= MIN_ROBUST, robust.mean()
    return want, robust


def _lattice_poses(cfg, n, k, rs):
    a = np.stack([rs.randint(int(lo), int(u) + 1, (n, k)) for lo, u in zip(cfg.clip_pose_idx_low, cfg.clip_pose_idx_up)], -1)
    return (a.astype(f32) * np.array(cfg.action_unit, f32) + np.array(cfg.clip_pose_low, f32)).astype(f32)


def _grazing_flights(tris, k, rs):
    """k flights near one env's surface: midpoint = a surface point offset along the normal by U(-0.1, 0.4), random direction,
    half-length U(0, 1)."""
    t = np.asarray(tris, np.float64)
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
        mid = pt + nrm * rs.uniform(-0.1, 0.4, (k, 1))
    else:
        mid = rs.uniform(-3, 3, (k, 3)) + [0, 0, 3]
    d = rs.randn(k, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    half = rs.uniform(0, 1, (k, 1))
    return (mid - d * half).astype(f32), (mid + d * half).astype(f32)


@pytest.fixture(scope="module")
def scenes():
    tris, ids = TC._test_scenes()
    mesh = TC._mesh(tris, ids)
    return tris, mesh, SO.SweepOracle.from_mesh(mesh)


# ---------------------------------------------------------------------------
# 1. hand cases
# ---------------------------------------------------------------------------
def test_hand_cases_on_the_kernel():
    from gennbv_amd.env.collision import CollisionBody
    for name, tris, a, b, radius, ground, expected in SO.hand_cases():
        mesh = TC._mesh([tris], [np.ones(len(tris), np.int32)])
        body = CollisionBody(ground=ground, sweep=True, sweep_radius=radius)
        got = mesh.sweep(_dev([a]), _dev([b]), body)
        assert got.dtype == torch.uint8 and got.shape == (1,)
        assert int(got[0]) == expected, name


# ---------------------------------------------------------------------------
# 2. kernel vs oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ground", [False, True])
def test_kernel_matches_oracle_on_grazing_and_lattice_flights(scenes, ground):
    tris, mesh, oracle = scenes
    n, k = mesh.num_envs, 48
    cfg = TaskConfig()
    body = _body(ground)
    rs = np.random.RandomState(21 + int(ground))
    env_idx = np.repeat(np.arange(n), k)
    blocked, free, grounded, total = np.zeros(n, np.int64), np.zeros(n, np.int64), 0, 0
    for kind in ("grazing", "lattice"):
        if kind == "grazing":
            ab = [_grazing_flights(tris[e].numpy(), k, rs) for e in range(n)]
            a, b = np.stack([x[0] for x in ab]), np.stack([x[1] for x in ab])
        else:
            a, b = _lattice_poses(cfg, n, k, rs), _lattice_poses(cfg, n, k, rs)
        got = mesh.sweep_candidates(_dev(a), _dev(b), body).cpu().numpy()
        assert got.shape == (n, k) and (got & ~np.uint8(PATH | PATH_GROUND) == 0).all()
        want, robust = _check(oracle, env_idx, a.reshape(n * k, -1), b.reshape(n * k, -1), got.reshape(-1), body)
        hit = ((want & PATH) != 0) & robust
        blocked += np.bincount(env_idx[hit], minlength=n)
        free += np.bincount(env_idx[~hit & robust], minlength=n)
        grounded += int(((want & PATH_GROUND) != 0).sum())
        total += int(robust.sum())
    assert blocked.sum() >= 0.1 * total and free.sum() >= 0.1 * total, (blocked, free, total)
    for e in (10, 11):  # the two sphere envs: flights inside, through and outside a dense curved mesh
        assert blocked[e] >= 1 and free[e] >= 1, (e, blocked, free)
    assert blocked[n - 1] == 0  # the env without triangles
    assert (grounded > 0) == ground


# ---------------------------------------------------------------------------
# 3. the interface
# ---------------------------------------------------------------------------
def test_interface_cases(scenes):
    tris, mesh, oracle = scenes
    n, k = mesh.num_envs, 6
    cfg = TaskConfig()
    body = _body()
    rs = np.random.RandomState(3)
    a, b = _lattice_poses(cfg, n, k, rs), _lattice_poses(cfg, n, k, rs)
    a[:, :, 2] += 0.5
    ta, tb = _dev(a), _dev(b)
    ref = mesh.sweep_candidates(ta, tb, body)
    assert bool(ref.any()) and not bool(ref.all())
    # broadcast starts (item stride 0) equal per-item starts holding the same rows
    start = ta[:, 0].contiguous()
    per_item = start[:, None, :].expand(n, k, 6).contiguous()
    want = mesh.sweep_candidates(per_item, tb, body)
    assert torch.equal(mesh.sweep_candidates(start, tb, body), want)
    assert torch.equal(mesh.sweep_candidates(start[:, None, :].expand(n, k, 6), tb, body), want)  # an expanded view: stride 0 too
    # rows inside a wider NaN-padded buffer; xyz alone; a preallocated out
    wa = torch.full((n, k, 9), float("nan"), device=DEV)
    wb = torch.full((n, k, 11), float("nan"), device=DEV)
    wa[..., :3], wb[..., :3] = ta[..., :3], tb[..., :3]
    out = torch.full((n, k), 255, dtype=torch.uint8, device=DEV)
    assert mesh.sweep_candidates(wa[..., :3], wb[..., :3], body, out=out) is out
    assert torch.equal(out, ref)
    assert torch.equal(mesh.sweep_candidates(wa[..., :6], wb[..., :4], body), ref)
    # K = 1, and sweep == sweep_candidates[:, 0]
    for j in (0, 3):
        one = mesh.sweep_candidates(ta[:, j:j + 1], tb[:, j:j + 1], body)
        assert torch.equal(one, ref[:, j:j + 1])
        assert torch.equal(mesh.sweep_candidates(ta[:, j:j + 1].contiguous(), tb[:, j:j + 1].contiguous(), body), ref[:, j:j + 1])
        got = mesh.sweep(ta[:, j], tb[:, j], body)
        assert got.shape == (n,) and torch.equal(got, ref[:, j])
    o1 = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    assert mesh.sweep(ta[:, 2], tb[:, 2], body, out=o1) is o1 and torch.equal(o1, ref[:, 2])
    # a NaN or inf endpoint gives 0 and disturbs no neighbour
    bad_a, bad_b = ta.clone(), tb.clone()
    bad_a[1, 2, 0] = float("nan")
    bad_b[2, 3, 2] = float("inf")
    bad_b[3, 0, 1] = float("-inf")
    got = mesh.sweep_candidates(bad_a, bad_b, _body(ground=True))
    want = mesh.sweep_candidates(ta, tb, _body(ground=True)).clone()
    want[1, 2] = want[2, 3] = want[3, 0] = 0
    assert torch.equal(got, want)
    # two calls are byte-equal
    assert torch.equal(mesh.sweep_candidates(ta, tb, body), ref)


def test_episode_length_gates_exactly_the_first_pose(scenes):
    tris, mesh, oracle = scenes
    n, k = mesh.num_envs, 5
    body = _body(ground=True)
    rs = np.random.RandomState(5)
    ab = [_grazing_flights(tris[e].numpy(), k, rs) for e in range(n)]
    ta, tb = _dev(np.stack([x[0] for x in ab])), _dev(np.stack([x[1] for x in ab]))
    ref = mesh.sweep_candidates(ta, tb, body)
    length = torch.tensor([(0, 1, 2, 7)[e % 4] for e in range(n)], dtype=torch.int64, device=DEV)
    got = mesh.sweep_candidates(ta, tb, body, episode_length=length)
    flown = (length > 1)[:, None]
    assert torch.equal(got, torch.where(flown, ref, torch.zeros_like(ref)))
    assert bool(ref[~flown[:, 0]].any()) and bool(got[flown[:, 0]].any())  # something was gated, something was not
    got1 = mesh.sweep(ta[:, 0], tb[:, 0], body, episode_length=length)
    assert torch.equal(got1, got[:, 0])
    # gated items leave an accumulated buffer alone
    buf = torch.full((n, k), 3, dtype=torch.uint8, device=DEV)
    mesh.sweep_candidates(ta, tb, body, episode_length=length, out=buf, accumulate=True)
    assert torch.equal(buf, got | 3)


def test_accumulate_onto_the_cylinder_codes(scenes):
    tris, mesh, oracle = scenes
    n, k = mesh.num_envs, 16
    cfg = TaskConfig()
    body = _body(ground=True)
    rs = np.random.RandomState(6)
    poses = _dev(_lattice_poses(cfg, n, k, rs))
    near = [TC._near_surface_poses(tris[e].numpy(), k, torch.Generator().manual_seed(e), True) for e in range(n)]
    poses[:, ::2] = _dev(np.stack(near))[:, ::2]  # half of them near a surface: cylinder codes too
    start = _dev(_lattice_poses(cfg, n, 1, rs))[:, 0]
    cyl = mesh.collide_candidates(poses, body)
    path = mesh.sweep_candidates(start, poses, body)
    buf = cyl.clone()
    assert mesh.sweep_candidates(start, poses, body, out=buf, accumulate=True) is buf
    assert torch.equal(buf, cyl | path)
    assert bool((cyl & 7).any()) and bool((path & PATH).any()) and bool((path & PATH_GROUND).any())
    assert bool(((cyl != 0) & (path != 0)).any())  # both kinds of bits in one byte somewhere


def test_the_piece_walk_loses_nothing_against_the_exhaustive_list():
    """A scene binned with 64 cells per axis and 8 cells per triangle against the same triangles in ONE cell (where every
    flight that touches the grid lists every triangle)."""
    from gennbv_amd.env.mesh_scene import MeshScene
    tris, ids = TC._test_scenes(seed=2)
    tl = [torch.as_tensor(t, dtype=torch.float32) for t in tris]
    il = [torch.as_tensor(i, dtype=torch.int32) for i in ids]
    fine = MeshScene.from_triangles(tl, il, device=DEV, cells_per_triangle=8, max_cells_per_axis=64)
    one = MeshScene.from_triangles(tl, il, device=DEV, max_cells_per_axis=1)
    assert int(fine.cell_res.max()) >= 16 and int(one.cell_res.max()) == 1
    n, k = fine.num_envs, 48
    cfg = TaskConfig()
    rs = np.random.RandomState(8)
    ab = [_grazing_flights(tris[e].numpy(), k // 2, rs) for e in range(n)]
    a = np.concatenate([np.stack([x[0] for x in ab]), _lattice_poses(cfg, n, k // 2, rs)[..., :3]], 1)
    b = np.concatenate([np.stack([x[1] for x in ab]), _lattice_poses(cfg, n, k // 2, rs)[..., :3]], 1)
    a[:, -1], b[:, -1] = [-9.5, -9.0, 0.3], [9.5, 9.0, 9.7]  # the long diagonal across every env
    for ground in (False, True):
        body = _body(ground)
        got_fine = fine.sweep_candidates(_dev(a), _dev(b), body)
        got_one = one.sweep_candidates(_dev(a), _dev(b), body)
        assert torch.equal(got_fine, got_one)
        assert bool((got_fine & PATH).any()) and not bool((got_fine & PATH).all())


# ---------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------
def test_refusals_by_return_code():
    from gennbv_amd import _lib
    from gennbv_amd.env.mesh_scene import MeshScene
    mesh = MeshScene.from_boxes(S.make_scenes(2, 20, seed=1), device=DEV)
    lib = _lib.load()
    sc = mesh.c_struct()
    a = torch.zeros(2, 4, 6, device=DEV)
    b = torch.ones(2, 4, 6, device=DEV)
    out = torch.zeros(2, 4, dtype=torch.uint8, device=DEV)
    length = torch.full((2,), 5, dtype=torch.int64, device=DEV)

    def call(scene=C.byref(sc), f=a.data_ptr(), fe=24, fi=6, t=b.data_ptr(), k=4, ts=6, radius=0.1, ground=0, ln=length.data_ptr(),
             acc=0, o=out.data_ptr()):
        return lib.gnbv_sweep_sphere(scene, f, fe, fi, t, k, ts, radius, ground, ln, acc, o, None)
    assert call() == 0 and call(ln=None) == 0 and call(fi=0) == 0 and call(acc=1) == 0
    for kw in (dict(scene=None), dict(f=None), dict(t=None), dict(o=None), dict(k=0), dict(k=-1), dict(ts=2), dict(fe=2), dict(fi=2),
               dict(fi=-6), dict(radius=0.0), dict(radius=-0.1), dict(radius=float("nan")), dict(radius=float("inf")), dict(acc=2)):
        assert call(**kw) == 1, kw  # hipErrorInvalidValue
    torch.cuda.synchronize()
    cpu_mesh = MeshScene.from_boxes(S.make_scenes(2, 20, seed=1), device="cpu")
    with pytest.raises(_lib.GennbvHipError):
        cpu_mesh.sweep_candidates(torch.zeros(2, 6), torch.zeros(2, 4, 6), _body())
    with pytest.raises(_lib.GennbvHipError):
        cpu_mesh.sweep(torch.zeros(2, 6), torch.zeros(2, 6), _body())
    with pytest.raises(_lib.GennbvHipError):
        mesh.sweep_candidates(torch.zeros(2, 6), torch.zeros(2, 4, 6), _body())  # poses on the host
    with pytest.raises(_lib.GennbvHipError):
        mesh.sweep(torch.zeros(2, 6, device=DEV), torch.zeros(2, 6), _body())


# ---------------------------------------------------------------------------
# 5. the env
# ---------------------------------------------------------------------------
def test_closed_loop_env_ends_episodes_on_blocked_flights():
    n, steps, L = 8, 36, 40
    body = _body()
    env, cfg, _ = TC._closed_env(n=n, max_len=L, body=body)
    plain, _, _ = TC._closed_env(n=n, max_len=L, body=_body(sweep=False))
    mesh = env.collision_mesh
    oracle = SO.SweepOracle.from_mesh(mesh)
    gen = torch.Generator().manual_seed(1)
    acts = [TC._random_actions(cfg, n, gen) for _ in range(steps)]
    idx = np.arange(n)

    obs, obs_p = env.reset(), plain.reset()
    assert torch.equal(obs, obs_p)
    assert torch.equal(env.collision_buf, mesh.collide(env.poses, body))  # the reset pose is set, not flown to
    prev = env.poses.clone()
    same = True  # no path bit has fired yet: the env without sweep must agree bit for bit
    path_only = 0
    robust_n = total_n = 0
    for s, a in enumerate(acts):
        # an episode's first step: the post-step kernel zeroed the count when the episode before ended, the pose is forced
        first = (env.episode_length_buf == 0).cpu().numpy()
        obs, rew, done, _ = env.step(a)
        code = env.collision_buf.cpu().numpy()
        cur = env.poses.clone()
        pose_code = mesh.collide(cur, body).cpu().numpy()
        want, robust = oracle.robust_codes(idx, prev.cpu().numpy(), cur.cpu().numpy(), body.path_radius, False)
        flown = ~first
        assert np.array_equal(code[first], pose_code[first]), f"step {s}: first steps"
        ok = flown & robust
        assert np.array_equal(code[ok], (pose_code | want)[ok]), f"step {s}: flown steps"
        robust_n, total_n = robust_n + int(robust[flown].sum()), total_n + int(flown.sum())
        d = done.cpu().numpy()
        assert d[code != 0].all(), f"step {s}: a non-zero code ends the episode"
        path_only += int((((code & PATH) != 0) & ((code & 7) == 0)).sum())
        if same:
            obs_p, rew_p, done_p, _ = plain.step(a)
            assert torch.equal(obs, obs_p), f"step {s}: observations before the first path bit"
            if (code & (PATH | PATH_GROUND)).any():
                same = False
                assert np.array_equal(plain.collision_buf.cpu().numpy(), code & 7)
            else:
                assert torch.equal(rew, rew_p) and torch.equal(done, done_p), f"step {s}"
                assert torch.equal(env.collision_buf, plain.collision_buf)
        prev = cur
    assert total_n > 0 and robust_n >= MIN_ROBUST * total_n
    assert path_only >= 1  # an episode ended on a path bit alone (bits 1, 2 and 4 clear)
    assert not same


# ---------------------------------------------------------------------------
# 6. the planners
# ---------------------------------------------------------------------------
def _planner_env(n, sweep=True):
    return TP._closed_env(n=n, collision=_body(sweep=sweep))


def _check_decision(oracle, env, body, from_poses, cand_poses, contact, chosen, tag):
    """cand_poses [n,k,6], contact [n,k] (the policy's buffer), chosen [n] candidate indices."""
    n, k = contact.shape
    idx = np.repeat(np.arange(n), k)
    a = np.repeat(from_poses.cpu().numpy(), k, 0)
    b = cand_poses.cpu().numpy().reshape(n * k, -1)
    want, robust = oracle.robust_codes(idx, a, b, body.path_radius, body.ground)
    want, robust = want.reshape(n, k), robust.reshape(n, k)
    assert robust.mean() >= MIN_ROBUST
    cyl = env.collision_mesh.collide_candidates(cand_poses.contiguous(), body).cpu().numpy()
    got = contact.cpu().numpy()
    assert np.array_equal(got[robust], (cyl | want)[robust]), tag
    blocked = (cyl | want) != 0
    every = (blocked | ~robust).all(1)  # (an env where nothing is surely free may pick anything)
    c = chosen.cpu().numpy()
    rows = np.arange(n)
    assert (~blocked[rows, c] | ~robust[rows, c] | every).all(), tag
    return int(blocked.sum()), int((want != 0).sum())


@pytest.mark.parametrize("kind", ["greedy", "oracle"])
def test_candidate_planners_never_fly_a_blocked_path(kind):
    from gennbv_amd.eval.baselines import GreedyGainPolicy, LatticeCandidates, OracleGainPolicy
    n, k, steps = 8, 32, 5
    env, cfg, _ = _planner_env(n)
    body = env.collision
    oracle = SO.SweepOracle.from_mesh(env.collision_mesh)
    pol = GreedyGainPolicy(env, k=k, seed=7) if kind == "greedy" else OracleGainPolicy(env, k=k, seed=7)
    assert pol.avoid_collisions and pol.sweep
    twin = LatticeCandidates(cfg, k, 7)  # the same seeded generator: the policy's candidates, step for step
    obs = env.reset()
    blocked = paths = 0
    for step in range(steps):
        start = env.poses.clone()
        act = pol(obs)[0]
        cand = twin.sample(n, DEV)
        match = (cand == act[:, None, :]).all(-1)
        assert bool(match.any(1).all())
        chosen = match.float().argmax(1)
        nb, npth = _check_decision(oracle, env, body, start, twin.poses(cand), pol._contact, chosen, f"{kind} step {step}")
        blocked, paths = blocked + nb, paths + npth
        obs = env.step(act)[0]
    assert paths > 0 and blocked < n * k * steps  # flights were blocked, and not all of them


def test_pool_planner_never_flies_a_blocked_path_with_and_without_persistent_bounds():
    from gennbv_amd.eval.baselines import PoolCoverPolicy
    n, p, steps = 8, 64, 5
    env_a, cfg, _ = _planner_env(n)
    env_b, _, _ = _planner_env(n)
    body = env_a.collision
    oracle = SO.SweepOracle.from_mesh(env_a.collision_mesh)
    pol_a = PoolCoverPolicy(env_a, pool_size=p, seed=3, persistent_bounds=True)
    pol_b = PoolCoverPolicy(env_b, pool_size=p, seed=3, persistent_bounds=False)
    assert pol_a.sweep and pol_b.sweep
    static = pol_a.pool.contact.clone()
    obs_a, obs_b = env_a.reset(), env_b.reset()
    paths = 0
    for step in range(steps):
        start = env_a.poses.clone()
        act_a, act_b = pol_a(obs_a)[0], pol_b(obs_b)[0]
        assert torch.equal(act_a, act_b), step
        assert torch.equal(pol_a.last_choice, pol_b.last_choice) and torch.equal(pol_a.last_gain, pol_b.last_gain)
        _, npth = _check_decision(oracle, env_a, body, start, pol_a.pool.poses, pol_a._contact, pol_a.last_choice.long(), f"pool step {step}")
        paths += npth
        assert torch.equal(pol_a._contact & 7, static)  # the static contact is a copy, the pool's own is untouched
        assert torch.equal(pol_a.pool.contact, static)
        obs_a, obs_b = env_a.step(act_a)[0], env_b.step(act_b)[0]
        assert torch.equal(obs_a, obs_b)
    assert paths > 0
    # the offline plan keeps the static contact
    choice, _, _ = pol_a.plan(4)
    assert not bool(static.gather(1, choice.long()).any()) or bool(static.all(1).any())


def test_without_sweep_the_planners_launch_no_path_test():
    from gennbv_amd.eval.baselines import GreedyGainPolicy, OracleGainPolicy, PoolCoverPolicy
    n, k, steps = 8, 32, 5
    makers = (lambda e: GreedyGainPolicy(e, k=k, seed=7), lambda e: OracleGainPolicy(e, k=k, seed=7),
              lambda e: PoolCoverPolicy(e, pool_size=64, seed=3))
    for make in makers:
        runs = []
        for rep in range(2):
            env, _, _ = _planner_env(n, sweep=False)
            pol = make(env)
            assert pol.avoid_collisions and not pol.sweep
            obs = env.reset()
            acts = []
            for _ in range(steps):
                a = pol(obs)[0]
                contact = pol.pool.contact if isinstance(pol, PoolCoverPolicy) else pol._contact
                assert not bool((contact & (PATH | PATH_GROUND)).any())
                acts.append(a.clone())
                obs = env.step(a)[0]
            assert env._prev_poses is None  # the env kept no copy of the poses either
            runs.append(torch.stack(acts))
        assert torch.equal(runs[0], runs[1])

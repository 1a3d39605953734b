"""GPU: plan-then-fly -- gnbv_tour_route (csrc/tour.hip) against the Python oracle (tests/tour_oracle.py) on every int,
FlightField.pairwise_mm against Dijkstra on every u32, and PoolCoverPolicy.plan_route / TourPolicy flown in a wall scene."""
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.flight import FlightLattice, pack_bits
from tests import tour_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
INF = TO.INF


def _u32(t):
    from gennbv_amd.ops.flight_field import field_u32
    return field_u32(t)


def _bits(a):
    """uint32 numpy -> the int32 tensor of the same bits on the device."""
    return torch.as_tensor(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(DEV)


# ---------------------------------------------------------------------------
# 1. the tour kernel
# ---------------------------------------------------------------------------
def _matrices(n, p, seed, side=7):
    """[n,p,p] u32: rounded distances between integer points on a coarse lattice (many ties)."""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, side, (n, p, 3)).astype(np.float64) * 100.0
    return np.rint(np.linalg.norm(pts[:, :, None] - pts[:, None], axis=-1)).astype(np.uint32), rng


def _cut_off(D, rng, frac=0.2):
    """No route between the start and some points of every env (symmetric); their other entries stay finite."""
    n, p = D.shape[:2]
    for e in range(n):
        for j in range(1, p):
            if rng.random() < frac:
                D[e, 0, j] = D[e, j, 0] = INF
    return D


def _check(D, count=None, max_moves=None):
    from gennbv_amd.ops.tour import route_tour
    n, p = D.shape[:2]
    want = TO.route_batch(D, count, max_moves)
    c = None if count is None else torch.as_tensor(np.asarray(count, np.int32)).to(DEV)
    res = route_tour(_bits(D), c, max_moves)
    got = (res.order.cpu().numpy(), res.routed.cpu().numpy(), res.length_mm.cpu().numpy(), res.status.cpu().numpy())
    assert res.order.dtype == torch.int32 and res.length_mm.dtype == torch.int64 and got[0].shape == (n, p)
    for name, g, w in zip(("order", "routed", "length_mm", "status"), got, want):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())
    return want


@pytest.mark.parametrize("p,n", [(1, 1), (2, 1), (3, 1), (3, 70), (33, 70), (64, 3), (65, 3), (128, 1), (128, 3)])
def test_route_equals_the_oracle_on_every_int(p, n):
    """Both LDS instances (p <= 64: 256 lanes; above: 1024) and their seam, one and many workgroups; per-env count over 1 .. p,
    points cut off from the start, and (n = 70) a count of 0 and of p + 1."""
    D, rng = _matrices(n, p, seed=100 * p + n)
    order, routed, length, status = _check(D)  # every point, every env
    assert (routed == p).all() and (status == 0).all()
    _cut_off(D, rng)
    count = np.array([1 + (e * 7 + p - 1) % p for e in range(n)], np.int32)  # env 0: count = p
    if n == 70:
        count[:min(p, 70)] = np.arange(1, min(p, 70) + 1)  # every count from 1 to p (p <= 70)
        count[-1], count[-2] = 0, p + 1
    order, routed, length, status = _check(D, count)
    if n == 70:
        assert status[-1] == 4 and status[-2] == 4 and routed[-1] == 1 and (order[-2] == np.arange(p)).all()
        assert (status[:-2] == 0).all()
    if p >= 33:
        big = (count > 8) & (count <= p)
        assert (routed[big] < count[big]).any()  # some point was cut off and sits in the tail


@pytest.mark.parametrize("p", [33, 65])
def test_move_cap_at_zero_one_and_default(p):
    D, _ = _matrices(8, p, seed=p)
    free = _check(D)
    zero = _check(D, max_moves=0)
    one = _check(D, max_moves=1)
    assert (zero[3] == 2).any() and (one[3] == 2).any() and (free[3] == 0).all()
    assert (free[2] <= one[2]).all() and (one[2] <= zero[2]).all() and (free[2] < zero[2]).any()


@pytest.mark.parametrize("p", [5, 64, 65, 128])
def test_all_equal_matrix_fires_every_tie_rule(p):
    D = np.full((2, p, p), 700, np.uint32)
    D[:, np.arange(p), np.arange(p)] = 0
    order, routed, length, status = _check(D, np.array([p, max(p - 3, 1)], np.int32))
    assert (order == np.arange(p)).all() and length[0] == 700 * (p - 1) and (status == 0).all()


@pytest.mark.parametrize("p", [33, 128])
def test_missing_leg_inside_the_route_set_sets_bit_one(p):
    D, rng = _matrices(3, p, seed=7 * p)
    for e in range(3):
        a, b = 1 + e, p - 1 - e
        D[e, a, b] = D[e, b, a] = INF  # both reachable from the start
    D[2, 0, 5] = D[2, 5, 0] = INF  # env 2 also has a cut-off point
    order, routed, length, status = _check(D)
    assert (status & 1).all() and routed.tolist() == [p, p, p - 1]


# ---------------------------------------------------------------------------
# 2. pairwise flight costs
# ---------------------------------------------------------------------------
def _body(**kw):
    from gennbv_amd.env.collision import CollisionBody
    return CollisionBody(sweep=True, **kw)


def _lattice(dims, unit=(0.2, 0.3, 0.25), low=(-1.0, 2.0, 0.1)):
    cfg = TaskConfig(clip_pose_low=list(low) + [0.0, 0.0, 0.0], clip_pose_idx_up=[d - 1 for d in dims] + [0, 12, 12],
                     action_unit=list(unit) + [0.0, 0.1, 0.1])
    lat = FlightLattice(cfg, stride=1)
    assert lat.dims == tuple(dims)
    return lat


def _field(lat, blocked, mode):
    """A FlightField over given masks (bool [N, M]); no mesh is consulted."""
    from gennbv_amd.ops.flight_field import FlightField
    stub = types.SimpleNamespace(device=torch.device(DEV), num_envs=blocked.shape[0])
    return FlightField(stub, lat, _body(), mode=mode, blocked=pack_bits(torch.as_tensor(blocked).to(DEV), lat.words))


SEALED_NODE = 157  # (4, 3, 2) of 9 x 7 x 5: an interior node
P_PAIR = 6


@pytest.fixture(scope="module")
def pair_case():
    """9 x 7 x 5 (M = 315), 7 envs: three random masks (env 1 with a free node behind a closed shell), empty, all blocked, two
    more random ones; 6 points per env a little off their nodes -- a blocked node, the sealed node, two points on one node,
    a NaN point -- and per-env counts."""
    lat = _lattice((9, 7, 5))
    m, rs = lat.num_nodes, np.random.RandomState(5)
    blocked = np.stack([rs.rand(m) < 0.1, rs.rand(m) < 0.3, rs.rand(m) < 0.5, np.zeros(m, bool), np.ones(m, bool), rs.rand(m) < 0.3,
                        rs.rand(m) < 0.3])
    idx = lat.node_index()
    blocked[1, np.abs(idx - idx[SEALED_NODE]).max(1) == 1] = True
    blocked[1, SEALED_NODE] = False
    nodes = np.stack([rs.choice(m, P_PAIR, replace=False) for _ in range(7)])
    for e in (0, 2, 5, 6):
        free = np.nonzero(~blocked[e])[0]
        nodes[e, :4] = rs.choice(free, 4, replace=False)  # mostly free nodes ...
        nodes[e, 4] = np.nonzero(blocked[e])[0][3]        # ... and a blocked one
    free1 = np.nonzero(~blocked[1] & (np.arange(m) != SEALED_NODE))[0]
    nodes[1] = np.concatenate([rs.choice(free1, 4, replace=False), [SEALED_NODE], free1[:1]])
    nodes[3, 5] = nodes[3, 0]  # two points on one node
    pts = np.zeros((7, P_PAIR, 6), f32)
    off = rs.uniform(-0.45, 0.45, (7, P_PAIR, 3))
    pts[..., :3] = lat.node_positions()[nodes] + off * lat.h
    pts[6, 2, 1] = np.nan
    assert np.array_equal(lat.nearest_np(pts)[np.isfinite(pts[..., :3]).all(-1)], nodes[np.isfinite(pts[..., :3]).all(-1)])
    count = np.array([6, 6, 5, 6, 3, 1, 6], np.int32)
    return lat, blocked, pts, count, TO.pairwise(lat, blocked, pts), TO.pairwise(lat, blocked, pts, count)


@pytest.mark.parametrize("mode", [1, 2])
def test_pairwise_mm_equals_dijkstra_on_every_u32(pair_case, mode):
    lat, blocked, pts, count, want_all, want_count = pair_case
    stub, node = TO.stubs_mm(lat, pts)
    assert ((want_all != INF) & ~np.eye(P_PAIR, dtype=bool)).sum() > 40 and (stub > 0).any()
    ff = _field(lat, blocked, mode)
    src = torch.as_tensor(pts[:, 0]).to(DEV)
    ff.update(src)
    before = (ff.field.clone(), ff.source.clone(), ff.status.clone(), ff.launches)
    points = torch.as_tensor(pts).to(DEV)
    got = _u32(ff.pairwise_mm(points))
    assert np.array_equal(got, want_all), np.argwhere(got != want_all)[:5].tolist()
    # symmetric, diagonal 0 (for every point that has a node)
    assert np.array_equal(got, got.transpose(0, 2, 1))
    diag = got[:, np.arange(P_PAIR), np.arange(P_PAIR)]
    assert (diag[node >= 0] == 0).all()
    # a non-finite point: its whole row and column
    assert (got[6, 2] == INF).all() and (got[6, :, 2] == INF).all()
    # the sealed node is cut off, a blocked node has no route, two points on one node are their stubs apart
    assert (got[1, 4, [0, 1, 2, 3, 5]] == INF).all() and (got[0, 4, [0, 1, 2, 3, 5]] == INF).all()
    assert got[3, 0, 5] == stub[3, 0] + stub[3, 5]
    # a row equals a fresh field from that point, queried at every point, plus the stubs
    for s in (0, 3):
        fresh = _u32(_field(lat, blocked, mode).update(points[:, s]).cost_mm(points)).astype(np.int64)
        row = np.where(fresh == INF, INF, fresh + stub[:, s:s + 1] + stub)
        row[:, s] = np.where(node[:, s] >= 0, 0, INF)
        assert np.array_equal(got[:, s].astype(np.int64), row)
    # counts: rows and columns at or above count[e] hold 0xFFFFFFFF
    gotc = _u32(ff.pairwise_mm(points, torch.as_tensor(count).to(DEV)))
    assert np.array_equal(gotc, want_count)
    assert (gotc[4, 3:] == INF).all() and (gotc[4, :, 3:] == INF).all() and gotc[5, 0, 0] == 0
    # a wider row stride gives the same matrix
    wide = torch.zeros(7, P_PAIR, 9, device=DEV)
    wide[..., :6] = points
    assert np.array_equal(_u32(ff.pairwise_mm(wide[..., :6])), want_all)
    # the env's own field is untouched, bit for bit
    assert torch.equal(ff.field, before[0]) and torch.equal(ff.source.view(torch.int32), before[1].view(torch.int32))
    assert torch.equal(ff.status, before[2]) and ff.launches == before[3]
    ff.check()
    # and the tour kernel routes on it: the same ints as the oracle on the oracle's matrix
    from gennbv_amd.ops.tour import route_tour
    res = route_tour(ff.pairwise_mm(points, torch.as_tensor(count).to(DEV)), torch.as_tensor(count).to(DEV))
    want = TO.route_batch(want_count, count)
    assert np.array_equal(res.order.cpu().numpy(), want[0]) and np.array_equal(res.length_mm.cpu().numpy(), want[2])
    assert np.array_equal(res.routed.cpu().numpy(), want[1]) and np.array_equal(res.status.cpu().numpy(), want[3])


# ---------------------------------------------------------------------------
# 3. plan_route and TourPolicy in a wall scene
# ---------------------------------------------------------------------------
N_ENVS, POOL, ROUNDS, SEED = 3, 24, 6, 7
# (pool size, rounds, seed) for which every kept view has a route from the init pose and no episode ends while the plan is flown
# (both asserted below); in the second case one round of env 1 has gain 0 and is dropped: 5 views, the tail repeats the last
WALL_CASES = [(POOL, ROUNDS, SEED), (20, 6, 9)]


def _wall_scene(n):
    """Per env: a wall x in [1.9, 2.1], |y| <= 5, z up to 12 (above the lattice: the way round is past its ends in y), and a
    closed hollow room round (-4, 0, 5.1): six slabs, inner half-width 1.5."""
    from gennbv_amd.env.mesh_scene import MeshScene, box_triangles
    c, a, t = np.array([-4.0, 0.0, 5.1]), 1.5, 0.2
    lo, hi = [[1.9, -5.0, 0.0]], [[2.1, 5.0, 12.0]]
    for ax in range(3):
        for sgn in (-1, 1):
            l, h = c - (a + t), c + (a + t)
            if sgn < 0:
                h[ax] = c[ax] - a
            else:
                l[ax] = c[ax] + a
            lo.append(l.tolist())
            hi.append(h.tolist())
    tris = box_triangles(torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32))
    ids = torch.arange(1, 8, dtype=torch.int32).repeat_interleave(12)
    return MeshScene.from_triangles([tris] * n, [ids] * n, device=DEV)


def _wall_env(n, flight):
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.ops.flight_field import FlightField
    cfg = TaskConfig(camera_width=64, camera_height=48, grid_size=20)
    mesh = _wall_scene(n)
    scene = mesh.ground_truth(20, torch.tensor([[8.0, -8.0, 8.0, -8.0, 12.0, 0.0]] * n))
    body = _body()
    field = FlightField(mesh, FlightLattice(cfg, stride=2), body) if flight else None
    return ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=30, collision=body, flight=field), cfg


def _kept(plan, contact):
    """The plan's kept views on the host, in plan order: gain > 0 and no static contact."""
    choice, gain = plan.choice.cpu().numpy(), plan.gain.cpu().numpy()
    return [[int(j) for j, g in zip(choice[e], gain[e]) if g > 0 and contact[e, j] == 0] for e in range(choice.shape[0])]


def _rows(a):
    return sorted(tuple(int(v) for v in r) for r in a)


def _fly(env, actions, steps):
    """reset, then `steps` steps of actions [N, T, 6]; no episode may end on the way."""
    env.reset()
    for t in range(steps):
        _, _, done, _ = env.step(actions[:, min(t, actions.shape[1] - 1)].contiguous())
        assert not bool(done.any()), (t, env.collision_buf.tolist())


@pytest.mark.parametrize("pool_size,rounds,seed", WALL_CASES)
def test_plan_route_and_tour_policy_fly_the_plan_in_a_wall_scene(pool_size, rounds, seed):
    from gennbv_amd.eval.baselines import PoolCoverPolicy, TourPolicy
    n, ROUNDS = N_ENVS, rounds
    env, cfg = _wall_env(n, flight=True)
    pool = PoolCoverPolicy(env, pool_size=pool_size, seed=seed)
    obs = env.reset()
    launches = env.flight.launches
    tour = TourPolicy(env, pool, ROUNDS)
    assert env.flight.launches == launches  # the plan ran on a private field
    plan = tour.last_plan
    contact = pool.pool.contact.cpu().numpy()
    kept = _kept(plan, contact)
    views = plan.views.cpu().numpy()
    acts = plan.actions.cpu().numpy()
    pool_actions = pool.pool_actions.cpu().numpy()
    assert plan.actions.shape == (n, ROUNDS, 6) and plan.actions.dtype == torch.int64
    assert min(len(k) for k in kept) >= 3  # a plan worth routing
    if seed == 9:
        assert [len(k) for k in kept] == [6, 5, 6] and plan.gain[1, 5] == 0
    length, plan_length, status = plan.length_mm.cpu().numpy(), plan.plan_length_mm.cpu().numpy(), plan.status.cpu().numpy()
    print("views", views.tolist(), "length_mm", length.tolist(), "plan_length_mm", plan_length.tolist(), "status", status.tolist())
    for e in range(n):
        # the routed views are the plan's kept views, as a set; never a view in contact; the tail repeats the last one
        assert views[e] == len(kept[e])
        assert _rows(acts[e, :views[e]]) == _rows(pool_actions[e, kept[e]])
        assert (acts[e, views[e]:] == acts[e, views[e] - 1]).all()
        assert plan_length[e] == -1 or length[e] <= plan_length[e]
    assert (status == 0).all() and (plan_length >= 0).all() and (length < plan_length).any()
    # the oracle on the same matrix (pairwise_mm has its own test against Dijkstra) gives the same route
    init = S.poses_from_actions(torch.tensor([cfg.init_action] * n), cfg).float().numpy()
    pool_poses = pool.pool.poses.cpu().numpy()
    pts = np.zeros((n, ROUNDS + 1, 3), f32)
    count = np.array([1 + len(k) for k in kept], np.int32)
    for e in range(n):
        pts[e, 0] = init[e, :3]
        pts[e, 1:count[e]] = pool_poses[e, kept[e], :3]
    D = _u32(env.flight.pairwise_mm(torch.as_tensor(pts).to(DEV), torch.as_tensor(count).to(DEV)))
    want = TO.route_batch(D, count)
    assert np.array_equal(want[2], length) and np.array_equal(want[1], views + 1)
    for e in range(n):
        assert np.array_equal(acts[e, :views[e]], pool_actions[e, np.array(kept[e])[want[0][e, 1:want[1][e]] - 1]])
        assert plan_length[e] == TO.path_length(D[e], list(range(count[e])))
    # fly the tour; in a second env fly the same views in gain order: coverage is a union, so it does not depend on the order
    steps = int(views.max())
    obs = env.reset()
    for t in range(steps):
        a = tour(obs)[0]
        assert torch.equal(a, plan.actions[:, min(t, ROUNDS - 1)])
        obs, _, done, _ = env.step(a)
        assert not bool(done.any()), (t, env.collision_buf.tolist())
    flown = env.flight_length.cpu().numpy()
    print("flown m", flown.tolist())
    for e in range(n):
        assert flown[e] <= length[e] * 1e-3 + 1e-3, (e, float(flown[e]), int(length[e]))
    env.flight.check()
    env2, _ = _wall_env(n, flight=True)
    gain_order = torch.stack([torch.as_tensor(pool_actions[e, kept[e] + [kept[e][-1]] * (ROUNDS - len(kept[e]))]) for e in range(n)]).to(DEV)
    assert torch.equal(plan.plan_actions, gain_order)  # RoutePlan.plan_actions is that order
    _fly(env2, gain_order, steps)
    assert torch.equal(env.updater.scanned_bits, env2.updater.scanned_bits)
    assert bool((env.updater.scanned_bits != 0).any())
    gain_flown = env2.flight_length.cpu().numpy()
    print("gain-order flown m", gain_flown.tolist())
    # after an episode ends the policy starts the same tour again: t == 0 returns a valid action, t == 1 the first view
    env.episode_length_buf.zero_()
    assert torch.equal(tour(obs)[0], plan.actions[:, 0])
    env.episode_length_buf.fill_(ROUNDS + 5)
    assert torch.equal(tour.predict(obs)[0], plan.actions[:, ROUNDS - 1])


def test_plan_route_without_a_flight_field_runs_on_euclid_mm():
    from gennbv_amd.eval.baselines import PoolCoverPolicy, TourPolicy
    n = N_ENVS
    env, cfg = _wall_env(n, flight=False)
    assert env.flight is None
    pool = PoolCoverPolicy(env, pool_size=POOL, seed=SEED)
    env.reset()
    tour = TourPolicy(env, pool, ROUNDS)
    plan = tour.last_plan
    kept = _kept(plan, pool.pool.contact.cpu().numpy())
    views = plan.views.cpu().numpy()
    assert views.tolist() == [len(k) for k in kept]  # every straight leg has a length: nothing is cut off
    init = S.poses_from_actions(torch.tensor([cfg.init_action] * n), cfg).float().numpy()
    pool_poses = pool.pool.poses.cpu().numpy()
    pts = np.zeros((n, ROUNDS + 1, 3), f32)
    count = np.array([1 + len(k) for k in kept], np.int32)
    for e in range(n):
        pts[e, 0] = init[e, :3]
        pts[e, 1:count[e]] = pool_poses[e, kept[e], :3]
    D = TO.euclid(pts, count)
    want = TO.route_batch(D, count)
    assert np.array_equal(plan.length_mm.cpu().numpy(), want[2]) and (plan.status.cpu().numpy() == 0).all()
    gain_len = np.array([TO.path_length(D[e], list(range(count[e]))) for e in range(n)])
    assert np.array_equal(plan.plan_length_mm.cpu().numpy(), gain_len) and (want[2] <= gain_len).all()
    acts, pool_actions = plan.actions.cpu().numpy(), pool.pool_actions.cpu().numpy()
    for e in range(n):
        order = want[0][e, 1:want[1][e]] - 1
        assert np.array_equal(acts[e, :views[e]], pool_actions[e, np.array(kept[e])[order]])
    # plan_route from the env's current pose and scanned set (the defaults) also runs
    again = pool.plan_route(ROUNDS)
    assert again.actions.shape == (n, ROUNDS, 6) and (again.status.cpu().numpy() == 0).all()
    from gennbv_amd import _lib
    with pytest.raises(_lib.GennbvHipError):
        pool.plan_route(128)

"""GPU: the belief free set -- gnbv_flight_blocked_tri (csrc/flightmap.hip) against the numpy oracle (tests/flightmap_oracle.py) on
every u32, padding included, in both modes, both grid forms and every flag combination; BeliefFlightField; the env that flies
the map's route and lets the true mesh judge it, against a host re-enactment; and MapGreedyPolicy."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import PI, TaskConfig
from gennbv_amd.env.flight import FlightLattice
from tests import flightmap_oracle as MO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
INVALID = 1  # hipErrorInvalidValue
RHO = 0.23
N_ENVS = 6
FLAGS = [(u, o, gr) for u in (0, 1) for o in (0, 1) for gr in (0, 1)]


def _lattice():
    """9 x 7 x 5, M = 315 (a tail word), unequal spacing: x in [-1, 0.6], y in [2, 3.8], z in [0.1, 1.1]."""
    cfg = TaskConfig(clip_pose_low=[-1.0, 2.0, 0.1, 0.0, 0.0, 0.0], clip_pose_idx_up=[8, 6, 4, 0, 12, 12],
                     action_unit=[0.2, 0.3, 0.25, 0.0, 0.1, 0.1])
    lat = FlightLattice(cfg, stride=1)
    assert lat.dims == (9, 7, 5) and lat.num_nodes == 315 and lat.words == 10
    return lat


def _frames(g):
    """range_gt [6,6] (max, min per axis: voxel centres) and voxel_size [6,3] of the six envs, anisotropic: envs 0-3 and 5 hold the
    whole lattice and its balls, env 4 is far smaller than the lattice."""
    big_lo, big_hi = np.array([-1.4, 1.6, -0.3]), np.array([1.0, 4.2, 1.5])
    small_lo, small_hi = np.array([-0.5, 2.5, 0.3]), np.array([0.1, 3.0, 0.7])
    rng, vox = np.zeros((N_ENVS, 6), f32), np.zeros((N_ENVS, 3), f32)
    for e in range(N_ENVS):
        lo, hi = (small_lo, small_hi) if e == 4 else (big_lo - 0.01 * e, big_hi + 0.013 * e)
        v = (hi - lo) / g
        vox[e] = v
        rng[e, 1::2] = lo + 0.5 * v
        rng[e, 0::2] = hi - 0.5 * v
    return rng, vox


@functools.lru_cache(maxsize=None)
def _case(g):
    """The six grids int8 [6,G,G,G]: random thirds of -1 / 0 / 1 (with the extremes -128 and 127), all free, all unknown, all
    occupied, the small grid (random thirds), the containing grid (sparse: 2.5 % occupied, 1.5 % unknown, so that nodes of
    both answers occur under every flag)."""
    rs = np.random.RandomState(g)
    tri = rs.randint(-1, 2, (N_ENVS, g, g, g)).astype(np.int8)
    tri[1], tri[2], tri[3] = -1, 0, 1
    u = rs.rand(g, g, g)
    tri[5] = np.where(u < 0.025, 1, np.where(u < 0.04, 0, -1))
    ext = rs.rand(N_ENVS, g, g, g) < 0.3
    tri = np.where(ext & (tri < 0), -128, np.where(ext & (tri > 0), 127, tri)).astype(np.int8)
    assert (tri == -128).any() and (tri == 127).any() and (tri == 0).any()
    rng, vox = _frames(g)
    return tri, rng, vox


@functools.lru_cache(maxsize=None)
def _want(g, unknown_blocks, outside_blocks, ground):
    """The oracle's words, computed once per (grid, flags) and shared by every test."""
    tri, rng, vox = _case(g)
    lat = _lattice()
    w = MO.blocked_words(tri, rng, vox, lat.dims, lat.lo, lat.h, RHO, bool(unknown_blocks), bool(outside_blocks), bool(ground))
    w.setflags(write=False)
    return w


def _launch(lat, tri_t, g, rng_t, vox_t, rho, flags, mode, out=None):
    """gnbv_flight_blocked_tri at the C ABI: tri_t int8 or float32 [N, >= G^3] with any row stride -> (return code, words)."""
    from gennbv_amd import _lib
    lib = _lib.load()
    n = tri_t.shape[0]
    if out is None:
        out = torch.full((n, lat.words), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    lo, h = (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)
    i8 = tri_t.dtype == torch.int8
    row = int(tri_t.stride(0)) if n > 1 else g ** 3
    nx, ny, nz = lat.dims
    err = lib.gnbv_flight_blocked_tri(tri_t.data_ptr() if i8 else None, row if i8 else 0, None if i8 else tri_t.data_ptr(), 0 if i8 else row,
                                      g, rng_t.data_ptr(), vox_t.data_ptr(), n, nx, ny, nz, lo, h, float(rho), *[int(f) for f in flags],
                                      out.data_ptr(), mode, None)
    torch.cuda.synchronize()
    return err, out.cpu().numpy().view(np.uint32)


def _forms(tri, g):
    """The two grid forms on the device: int8 rows with a padded row stride, fp32 rows inside an observation-shaped buffer."""
    n, g3 = tri.shape[0], g ** 3
    i8 = torch.full((n, g3 + 5), 77, dtype=torch.int8, device=DEV)
    i8[:, :g3] = torch.as_tensor(tri.reshape(n, g3)).to(DEV)
    obs = torch.full((n, 7 + g3 + 3), 5.0, dtype=torch.float32, device=DEV)  # [state | grid | rgb]: everything round the grid > 0
    obs[:, 7:7 + g3] = torch.as_tensor(tri.reshape(n, g3).astype(f32)).to(DEV)
    return {"i8": i8[:, :g3], "f32": obs[:, 7:7 + g3]}


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("g", [12, 8])
@pytest.mark.parametrize("mode", [1, 2])
def test_blocked_bits_equal_the_oracle_on_every_u32(g, mode):
    tri, rng, vox = _case(g)
    lat = _lattice()
    forms = _forms(tri, g)
    rng_t, vox_t = torch.as_tensor(rng).to(DEV), torch.as_tensor(vox).to(DEV)
    for flags in FLAGS:
        want = _want(g, *flags)
        for name, t in forms.items():
            err, got = _launch(lat, t, g, rng_t, vox_t, RHO, flags, mode)
            assert err == 0
            assert np.array_equal(got, want), (flags, name, np.argwhere(got != want)[:5].tolist())
    # the cases reach what they are there for
    plain = MO.pack_words(np.zeros((1, 315), bool))[0]
    w = _want(g, 0, 0, 0)
    assert (w[1] == plain).all() and (w[2] == plain).all()          # all free, all unknown: nothing blocks
    assert (_want(g, 1, 0, 0)[2] == 0xFFFFFFFF).all() and (w[3] == 0xFFFFFFFF).all()  # unknown by flag; all occupied
    assert (w[:, -1] >> np.uint32(315 - 9 * 32) == (1 << 5) - 1).all()  # padding bits set
    out = _want(g, 0, 1, 0)
    bits = lambda words: int(sum(bin(int(x)).count("1") for x in words))  # noqa: E731
    assert bits(out[4]) > 5 + 315 * 0.8 and bits(out[1]) == 5  # most nodes leave the small grid; none the large ones
    assert 5 + 10 < bits(w[4]) < 320 - 10 and 5 + 10 < bits(w[5]) < 320 - 10  # both answers occur
    assert bits(w[5]) + 10 < bits(_want(g, 1, 0, 0)[5]) < 320 - 10
    gr = _want(g, 0, 0, 1)
    assert bits(gr[1]) == 5 + 63  # z = 0.1 - rho <= 0: the lowest layer


@pytest.mark.parametrize("g", [12, 8])
def test_mode_0_equals_both_and_unknown_blocks_is_a_superset(g):
    tri, rng, vox = _case(g)
    lat = _lattice()
    t = _forms(tri, g)["i8"]
    rng_t, vox_t = torch.as_tensor(rng).to(DEV), torch.as_tensor(vox).to(DEV)
    for flags in ((0, 0, 0), (1, 1, 1)):
        got = [_launch(lat, t, g, rng_t, vox_t, RHO, flags, mode) for mode in (0, 1, 2)]
        assert all(err == 0 for err, _ in got)
        assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][1], got[2][1]) and np.array_equal(got[0][1], _want(g, *flags))
    for o in (0, 1):
        for gr in (0, 1):
            _, without = _launch(lat, t, g, rng_t, vox_t, RHO, (0, o, gr), 0)
            _, with_unknown = _launch(lat, t, g, rng_t, vox_t, RHO, (1, o, gr), 0)
            assert (without & ~with_unknown == 0).all() and (with_unknown != without).any()


def test_the_lds_limit():
    """G = 109 is the largest grid whose bits fit LDS (more than a launch may ask for without the attribute), 110 the first that
    does not: mode 1 is refused by the return code before anything is launched, modes 0 and 2 read the grid in place."""
    from gennbv_amd import _lib
    cap = int(_lib.load().gnbv_flightmap_lds_max_grid())
    assert cap == 109
    lat = _lattice()
    rs = np.random.RandomState(3)
    for g in (cap, cap + 1):
        tri = rs.randint(-1, 2, (1, g, g, g)).astype(np.int8)
        tri[rs.rand(1, g, g, g) < 0.9998] = -1  # very sparse (a ball holds thousands of voxels): both answers occur
        rng, vox = _frames(g)
        rng, vox = rng[:1], vox[:1]
        want = MO.blocked_words(tri, rng, vox, lat.dims, lat.lo, lat.h, RHO, True, False, False)
        assert 5 + 30 < sum(bin(int(x)).count("1") for x in want[0]) < 320 - 30
        rng_t, vox_t = torch.as_tensor(rng).to(DEV), torch.as_tensor(vox).to(DEV)
        forms = {"i8": torch.as_tensor(tri.reshape(1, -1)).to(DEV), "f32": torch.as_tensor(tri.reshape(1, -1).astype(f32)).to(DEV)}
        for name, t in forms.items():
            for mode in (0, 1, 2):
                err, got = _launch(lat, t, g, rng_t, vox_t, RHO, (1, 0, 0), mode)
                if mode == 1 and g > cap:
                    assert err == INVALID and (got == 0x5A5A5A5A).all()  # nothing was launched
                else:
                    assert err == 0 and np.array_equal(got, want), (g, name, mode)


# ---------------------------------------------------------------------------
# 2. BeliefFlightField
# ---------------------------------------------------------------------------
def _body(**kw):
    from gennbv_amd.env.collision import CollisionBody
    return CollisionBody(sweep=True, **kw)


def test_belief_field_refresh_update_and_pairwise():
    from gennbv_amd import _lib
    from gennbv_amd.ops.flight_field import BeliefFlightField, field_u32
    from tests import flight_oracle as FO
    g = 12
    tri, rng, vox = _case(g)
    lat = _lattice()
    body = _body(sweep_radius=0.05, ground=True)
    margin = 0.02
    ff = BeliefFlightField(N_ENVS, lat, body, torch.as_tensor(rng), torch.as_tensor(vox), g, unknown="blocked", margin=margin, device=DEV)
    assert ff.belief and ff.rho == lat.inflated_radius(body) + margin
    assert (field_u32(ff.blocked_map) == 0xFFFFFFFF).all()  # nothing is flyable before the first refresh
    want = MO.blocked_words(tri, rng, vox, lat.dims, lat.lo, lat.h, ff.rho, True, False, True)
    forms = _forms(tri, g)
    for t in forms.values():
        ff.blocked_map.fill_(0)
        assert ff.refresh(t) is ff
        assert np.array_equal(field_u32(ff.blocked_map), want)
    with pytest.raises(_lib.GennbvHipError):
        ff.refresh(forms["i8"].cpu())
    with pytest.raises(_lib.GennbvHipError):
        ff.refresh(forms["i8"].to(torch.int32))
    # update(): the drone's own node is flyable whatever the map says; a NaN pose is left alone; blocked_map stays pure
    nodes = np.array([0, 100, 157, 314, 31, 32])
    poses = np.zeros((N_ENVS, 6), f32)
    poses[:, :3] = lat.node_positions()[nodes] + 0.3 * lat.h * np.array([1, -1, 1])
    poses[4, 1] = np.nan
    ff.update(torch.as_tensor(poses).to(DEV))
    assert np.array_equal(field_u32(ff.blocked_map), want)
    got = field_u32(ff.blocked)
    cleared = want.copy()
    for e in (0, 1, 2, 3, 5):
        cleared[e, nodes[e] >> 5] &= ~np.uint32(1 << (nodes[e] & 31))
    assert np.array_equal(got, cleared) and (cleared != want).any()  # (env 3 is all occupied: its own node was blocked)
    blocked = FO.unpack_bits(got.view(np.int32), lat.num_nodes)
    field = field_u32(ff.field)
    for e in range(N_ENVS):
        ref = FO.dijkstra(blocked[e], lat.dims, lat.cost, -1 if e == 4 else int(nodes[e]))
        assert np.array_equal(field[e], ref), e
    assert (field[3] != 0xFFFFFFFF).sum() == 1  # alone in an occupied world
    # pairwise_mm shares `blocked`
    pts = torch.as_tensor(poses[:, None, :].repeat(2, 1)).to(DEV)
    pts[:, 1, :3] = torch.as_tensor(lat.node_positions()[[8, 8, 8, 8, 8, 8]].astype(f32)).to(DEV)
    mm = field_u32(ff.pairwise_mm(pts))
    assert (mm[[0, 1, 2, 5], 0, 0] == 0).all() and np.array_equal(mm[:, 0, 1], mm[:, 1, 0])
    ff.check()
    with pytest.raises(_lib.GennbvHipError):
        BeliefFlightField(1, lat, body, torch.as_tensor(rng[:1]), torch.as_tensor(vox[:1]), 110, map_mode=1, device=DEV)


# ---------------------------------------------------------------------------
# 3. the env flies the map's route, the truth judges it
# ---------------------------------------------------------------------------
ENV_N, ENV_G = 4, 20


def _env_cfg():
    """The default task's volume on a coarser pose lattice (0.5 m): the stride-2 flight lattice has 17 x 17 x 11 nodes, which
    the node loop of the oracle walks in a fraction of a second."""
    return TaskConfig(camera_width=80, camera_height=60, grid_size=ENV_G, clip_pose_idx_up=[32, 32, 20, 0, 12, 12],
                      action_unit=[0.5, 0.5, 0.5, 0.0, PI / 12.0, PI / 6.0], init_action=[16, 16, 20, 0, 12, 0])


def _belief_env(unknown, max_len=4, seed=2, **kw):
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.ops.flight_field import BeliefFlightField
    cfg = _env_cfg()
    scene = S.make_scenes(ENV_N, ENV_G, seed=seed)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = _body()
    lat = FlightLattice(cfg, stride=2)
    assert lat.dims == (17, 17, 11)
    flight = BeliefFlightField(ENV_N, lat, body, scene.range_gt, scene.voxel_size, ENV_G, unknown=unknown, device=DEV, **kw)
    env = ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=max_len, collision=body, flight=flight)
    return env, cfg, scene, mesh, lat, body


def _probe(env, lat, body):
    """A copy of the env's field as it stands: what the pilot knows before the step."""
    from gennbv_amd.ops.flight_field import FlightField
    stub = types.SimpleNamespace(device=torch.device(DEV), num_envs=env.num_envs)
    p = FlightField(stub, lat, body, blocked=env.flight.blocked.clone())
    p.field.copy_(env.flight.field)
    p.source.copy_(env.flight.source)
    return p


@pytest.mark.parametrize("unknown", ["free", "blocked"])
def test_env_flies_the_maps_route_and_the_truth_judges_it(unknown):
    from gennbv_amd.ops.flight_field import field_u32
    env, cfg, scene, mesh, lat, body = _belief_env(unknown)
    n = ENV_N
    rng, vox = scene.range_gt.numpy(), scene.voxel_size.numpy()
    gen = torch.Generator().manual_seed(11)
    obs = env.reset()
    assert env.flight.refreshes == 1 and env.flight.launches == 1 and not env.flight_length.any() and int(env.route_overflow) == 0
    saw = {"routed": 0, "unrouted": 0, "first": 0, "hit": 0, "legs": 0}

    def check_map(obs):
        tri = obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim].reshape(n, ENV_G, ENV_G, ENV_G).cpu().numpy()
        want = MO.blocked_words(tri, rng, vox, lat.dims, lat.lo, lat.h, env.flight.rho, unknown == "blocked", False, False)
        got_map, got = field_u32(env.flight.blocked_map), field_u32(env.flight.blocked)
        assert np.array_equal(got_map, want)
        node = lat.nearest_np(env.poses.cpu().numpy())
        cleared = want.copy()
        for e in range(n):
            cleared[e, node[e] >> 5] &= ~np.uint32(1 << (node[e] & 31))
        assert np.array_equal(got, cleared)  # the source-node bit is clear in `blocked`, untouched in `blocked_map`
        assert torch.equal(env.flight.source, env.poses[:, :3])
    check_map(obs)
    for step in range(7):
        act = torch.stack([torch.randint(0, int(u) + 1, (n,), generator=gen) for u in cfg.clip_pose_idx_up], -1).to(DEV)
        probe = _probe(env, lat, body)
        prev, ep, length_before = env.poses.clone(), env.episode_length_buf.clone() + 1, env.flight_length.clone()
        obs, _, done, _ = env.step(act)
        new = env.poses.clone()
        # --- the host re-enactment: FlightField.path, one MeshScene.sweep per leg, the rule of the env's docstring
        way, length = probe.path(new)
        length = length.cpu().numpy()
        routed = torch.as_tensor(length > 0).to(DEV)
        code = torch.zeros(n, dtype=torch.uint8, device=DEV)
        for j in range(way.shape[1] - 1):
            a, b = way[:, j].contiguous(), way[:, j + 1].contiguous()
            on = torch.as_tensor(j < length - 1).to(DEV)  # (rows past the length are NaN: their code is 0 anyway)
            a, b = torch.where(on[:, None], a, prev[:, :3]), torch.where(on[:, None], b, prev[:, :3])
            code |= torch.where(on, mesh.sweep(a, b, body, ep), torch.zeros_like(code))
        straight_code = mesh.sweep(prev, new, body, ep)
        code = torch.where(routed, code, straight_code)
        first = ep <= 1
        flown = torch.where(routed, probe.cost(new[:, None])[:, 0], (new[:, :3] - prev[:, :3]).norm(dim=-1))
        want_len = torch.where(first, torch.zeros_like(flown), length_before + flown)
        assert torch.equal(env.path_code, code), (step, env.path_code.tolist(), code.tolist())
        assert torch.equal(env.collision_buf & 24, code)  # in full: nothing is dropped
        assert torch.equal(env.collision_buf & 7, mesh.collide(new, body))
        assert torch.equal(env.flight_length, want_len), (step, env.flight_length.tolist(), want_len.tolist())
        assert torch.equal(env.routed, routed & ~first)
        assert not (code[first] != 0).any()  # a first pose is set, not flown to
        assert done[env.collision_buf != 0].all()  # what the truth found ends the episode
        check_map(obs)
        saw["routed"] += int((routed & ~first).sum())
        saw["unrouted"] += int((~routed & ~first).sum())
        saw["first"] += int(first.sum())
        saw["hit"] += int((code != 0).sum())
        saw["legs"] = max(saw["legs"], int(length.max()) - 1)
    assert env.flight.refreshes == 8 and env.flight.launches == 8 and int(env.route_overflow) == 0
    env.flight.check()
    assert saw["first"] >= n  # an episode boundary was crossed
    if unknown == "free":
        assert saw["routed"] >= n and saw["legs"] >= 3  # the optimistic pilot finds routes through what it has not seen
    else:
        assert saw["unrouted"] >= 1  # the conservative one starts inside unknown space: straight flights
    print("belief env", unknown, saw)


def test_belief_env_reads_the_int8_grid_where_it_is_given_and_needs_a_matching_grid():
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.ops.flight_field import BeliefFlightField, field_u32
    env, cfg, scene, mesh, lat, body = _belief_env("free")
    assert env.supports_grid_i8
    grid = torch.zeros(ENV_N, cfg.grid_dim, dtype=torch.int8, device=DEV)
    obs = env.reset(grid_i8_out=grid)
    tri = grid.reshape(ENV_N, ENV_G, ENV_G, ENV_G).cpu().numpy()
    assert np.array_equal(np.sign(tri), np.sign(obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim].reshape(tri.shape).cpu().numpy()))
    assert (tri > 0).any() and (tri < 0).any() and (tri == 0).any()
    want = MO.blocked_words(tri, scene.range_gt.numpy(), scene.voxel_size.numpy(), lat.dims, lat.lo, lat.h, env.flight.rho)
    assert np.array_equal(field_u32(env.flight.blocked_map), want)
    other = BeliefFlightField(ENV_N, lat, body, scene.range_gt, scene.voxel_size, ENV_G + 1, device=DEV)
    with pytest.raises(ValueError):
        ReplayFeedEnv(cfg, scene, env.feed, DEV, collision=body, flight=other)


# ---------------------------------------------------------------------------
# 4. the planner that asks the map alone
# ---------------------------------------------------------------------------
class _NoMesh:
    """Stands in for the collision mesh: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the collision mesh was consulted: {name}")


class _Fixed:
    """LatticeCandidates' protocol over a fixed candidate list."""

    def __init__(self, cfg, actions):
        self.cfg, self.actions = cfg, torch.tensor(actions, dtype=torch.int64)

    def sample(self, num_envs, device="cpu"):
        return self.actions[None].expand(num_envs, -1, -1).contiguous().to(device)

    def poses(self, actions):
        return S.poses_from_actions(actions, self.cfg).float()


def test_map_greedy_asks_the_map_alone():
    from gennbv_amd import _lib
    from gennbv_amd.eval.baselines import GreedyGainPolicy, MapGreedyPolicy
    env, cfg, scene, mesh, lat, body = _belief_env("free", max_len=30)
    n = ENV_N
    obs = env.reset()
    # a map of the planner's own: free everywhere but an occupied slab, x voxels 12 .. 14 (1.7 .. 4.2 m), every y, z voxels 0 .. 9 (up to
    # 5 m): the way to the far side leads over its top
    tri = torch.full((n, ENV_G, ENV_G, ENV_G), -1, dtype=torch.int8, device=DEV)
    tri[:, 12:15, :, :10] = 1
    env.flight.refresh(tri.reshape(n, -1)).update(env.poses)
    inside, free_far, free_near = [22, 16, 4, 0, 6, 0], [30, 16, 10, 0, 6, 0], [10, 16, 10, 0, 6, 0]  # (3, 0, 2.1), (7, 0, 5.1), (-3, 0, 5.1)
    gains = torch.tensor([[300, 0, 0], [200, 0, 0], [100, 0, 0]], dtype=torch.int32, device=DEV)
    pol = MapGreedyPolicy(env, k=3, weights=(1, 0), gain_backend=lambda t, p: gains[None].expand(n, -1, -1))
    pol.cands = _Fixed(cfg, [inside, free_far, free_near])
    real = env.collision_mesh
    env.collision_mesh = _NoMesh()
    try:
        act = pol(obs)[0]
        cost = env.flight.cost(pol.cands.poses(pol.cands.sample(n, DEV)))
        assert torch.isinf(cost[:, 0]).all() and torch.isfinite(cost[:, 1:]).all()
        assert act.tolist() == [free_far] * n and pol._contact.tolist() == [[1, 0, 0]] * n
        # random candidates, the real gain kernel: never an unreachable choice while a reachable one exists
        pol = MapGreedyPolicy(env, k=16, seed=5)
        picked_among_mixed = 0
        for _ in range(3):
            act = pol(obs)[0]
            pose = S.poses_from_actions(act, cfg).float()
            chosen = env.flight.cost(pose[:, None])[:, 0]
            reach = pol._contact == 0
            mixed = reach.any(1) & ~reach.all(1)
            assert torch.isfinite(chosen[reach.any(1)]).all()
            picked_among_mixed += int(mixed.sum())
        assert picked_among_mixed >= 1
    finally:
        env.collision_mesh = real
    # it refuses a mesh-based field, and GreedyGainPolicy keeps its own contact
    from gennbv_amd.ops.flight_field import FlightField
    env.flight = FlightField(real, lat, body)
    with pytest.raises(_lib.GennbvHipError):
        MapGreedyPolicy(env, k=3)
    assert GreedyGainPolicy.contact is not MapGreedyPolicy.contact

"""GPU: collision-free flight between views -- gnbv_flight_field / _query / _path (csrc/flight.hip) against the Dijkstra oracle
(tests/flight_oracle.py) on every u32 and in both modes, MeshScene.flight_blocked against the fp64 brute-force oracles of the
sweep and the collision tests, the soundness of whole routes against the swept sphere, and the env and planners that fly
detours."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.flight import INF_MM, FlightLattice, pack_bits
from tests import collision_oracle as CO
from tests import flight_oracle as FO
from tests import sweep_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
PATH, PATH_GROUND = SO.PATH, SO.PATH_GROUND
MIN_ROBUST = 0.99


def _body(**kw):
    from gennbv_amd.env.collision import CollisionBody
    return CollisionBody(sweep=True, **kw)


def _cfg(up, unit=(0.2, 0.3, 0.25), low=(-1.0, 2.0, 0.1)):
    return TaskConfig(clip_pose_low=list(low) + [0.0, 0.0, 0.0], clip_pose_idx_up=list(up) + [0, 12, 12],
                      action_unit=list(unit) + [0.0, 0.1, 0.1])


def _lattice(dims, **kw):
    lat = FlightLattice(_cfg([d - 1 for d in dims], **kw), stride=1)
    assert lat.dims == tuple(dims)
    return lat


def _field(lat, blocked, mode):
    """A FlightField over given masks (bool [N, M]); no mesh is consulted."""
    from gennbv_amd.ops.flight_field import FlightField
    n = blocked.shape[0]
    stub = types.SimpleNamespace(device=torch.device(DEV), num_envs=n)
    bits = pack_bits(torch.as_tensor(blocked).to(DEV), lat.words)
    return FlightField(stub, lat, _body(), mode=mode, blocked=bits)


def _u32(t):
    from gennbv_amd.ops.flight_field import field_u32
    return field_u32(t)


def _poses(lat, nodes):
    """fp32 poses [N, 6] a little off the given nodes (so the nearest-node rule has work to do)."""
    p = np.zeros((len(nodes), 6), f32)
    p[:, :3] = lat.node_positions()[nodes] + 0.3 * lat.h * np.array([1, -1, 1])
    return p


SEALED_NODE = 157  # (4, 3, 2) of 9 x 7 x 5: an interior node


def _small_case():
    """9 x 7 x 5 (M = 315: a tail word), 7 envs: three random masks, empty, all blocked, source blocked, source pose NaN."""
    lat = _lattice((9, 7, 5))
    m, rs = lat.num_nodes, np.random.RandomState(5)
    blocked = np.stack([rs.rand(m) < 0.1, rs.rand(m) < 0.3, rs.rand(m) < 0.5, np.zeros(m, bool), np.ones(m, bool), rs.rand(m) < 0.3,
                        rs.rand(m) < 0.3])
    src = np.array([17, 200, 314, 0, 100, 150, 42])
    for e in (0, 1, 2, 6):
        blocked[e, src[e]] = False
    blocked[5, src[5]] = True
    idx = lat.node_index()
    blocked[1, np.abs(idx - idx[SEALED_NODE]).max(1) == 1] = True  # a free node behind a closed shell of blocked ones
    blocked[1, SEALED_NODE] = False
    poses = _poses(lat, src)
    poses[6, 1] = np.nan
    want = np.stack([FO.dijkstra(blocked[e], lat.dims, lat.cost, -1 if e == 6 else int(src[e])) for e in range(7)])
    return lat, blocked, src, poses, want


@pytest.fixture(scope="module")
def small_case():
    return _small_case()


# ---------------------------------------------------------------------------
# 1. the field
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_field_equals_dijkstra_on_every_u32(small_case, mode):
    lat, blocked, src, poses, want = small_case
    assert (want[4] == INF_MM).all() and (want[5] == INF_MM).all() and (want[6] == INF_MM).all()
    assert all(((want[e] != INF_MM) & ~blocked[e]).sum() > 30 for e in range(4))
    assert not blocked[1, SEALED_NODE] and want[1, SEALED_NODE] == INF_MM  # a free node that no route reaches
    ff = _field(lat, blocked, mode)
    assert (_u32(ff.field) == INF_MM).all()  # before the first update
    ff.update(torch.as_tensor(poses).to(DEV))
    got = _u32(ff.field)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert not bool(ff.status.any())
    ff.check()
    # a strided pose tensor, and a second update from other poses into the same buffers
    wide = torch.zeros(7, 11, device=DEV)
    wide[:, :6] = torch.as_tensor(poses).to(DEV)
    ff.update(wide[:, :6])
    assert np.array_equal(_u32(ff.field), want)
    src2 = (src + 31) % lat.num_nodes
    ff.update(torch.as_tensor(_poses(lat, src2)).to(DEV))
    want2 = np.stack([FO.dijkstra(blocked[e], lat.dims, lat.cost, int(src2[e])) for e in range(7)])
    assert np.array_equal(_u32(ff.field), want2)


@pytest.mark.parametrize("mode", [1, 2])
def test_field_survives_a_serpentine(mode):
    lat = _lattice((17, 17, 3), unit=(0.4, 0.4, 0.4))
    blocked = FO.serpentine(lat.dims)[None]
    want = FO.dijkstra(blocked[0], lat.dims, lat.cost, 0)
    assert want[16] >= 8 * 16 * 400  # the route snakes through every open column: more than a hundred hops
    ff = _field(lat, blocked, mode)
    ff.update(torch.as_tensor(_poses(lat, [0])).to(DEV))
    assert np.array_equal(_u32(ff.field)[0], want)
    assert int(ff.status[0]) == 0
    nodes, count = ff.path_nodes(torch.as_tensor(_poses(lat, [16])).to(DEV))
    assert nodes[0, :int(count[0])].tolist() == FO.walk(want, lat.dims, lat.cost, 16)


def test_lds_threshold_and_modes():
    from gennbv_amd import _lib
    lib = _lib.load()
    cap = int(lib.gnbv_flight_lds_max_nodes())
    assert cap == (160 * 1024 - 16) // 4
    nx = ny = 36
    nz = cap // (nx * ny)
    rs = np.random.RandomState(9)
    for planes, fits in ((nz, True), (nz + 1, False)):
        lat = _lattice((nx, ny, planes), unit=(0.2, 0.2, 0.2))
        m = lat.num_nodes
        assert (m <= cap) == fits and (not fits or m + nx * ny > cap)
        blocked = (rs.rand(1, m) < 0.3)
        src = int(np.nonzero(~blocked[0])[0][m // 3])
        want = FO.dijkstra(blocked[0], lat.dims, lat.cost, src)
        assert ((want != INF_MM).sum() > m // 2)
        pose = torch.as_tensor(_poses(lat, [src])).to(DEV)
        fields = {}
        for mode in ((0, 1, 2) if fits else (0, 2)):
            ff = _field(lat, blocked, mode)
            ff.field.fill_(7)
            ff.update(pose)
            fields[mode] = _u32(ff.field)[0]
            assert np.array_equal(fields[mode], want), mode
            assert int(ff.status[0]) == 0
        if not fits:  # mode 1 says no: by the op, and by the entry point's return code, before anything is launched
            with pytest.raises(_lib.GennbvHipError):
                _field(lat, blocked, 1)
            ff = _field(lat, blocked, 0)
            ff.field.fill_(7)
            cost, lo, h = (C.c_uint32 * 8)(*lat.cost.tolist()), (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)
            args = (ff.blocked.data_ptr(), 1, nx, ny, planes, cost, pose.data_ptr(), 6, lo, h, ff.field.data_ptr(), ff.status.data_ptr())
            assert lib.gnbv_flight_field(*args, 1, None) == 1  # hipErrorInvalidValue
            assert lib.gnbv_flight_field(*args, 3, None) == 1
            torch.cuda.synchronize()
            assert bool((ff.field == 7).all())


def test_refusals_by_return_code(small_case):
    from gennbv_amd import _lib
    lat, blocked, src, poses, want = small_case
    lib = _lib.load()
    ff = _field(lat, blocked, 0)
    p = torch.as_tensor(poses).to(DEV)
    cost, lo, h = (C.c_uint32 * 8)(*lat.cost.tolist()), (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)
    zero_cost = (C.c_uint32 * 8)(0, 0, 200, 300, 250, 300, 300, 400)
    huge_cost = (C.c_uint32 * 8)(*([2 ** 31] * 8))
    bad_h = (C.c_double * 3)(0.2, 0.0, 0.25)

    def call(b=ff.blocked.data_ptr(), n=7, nx=9, ny=7, nz=5, c=cost, ps=p.data_ptr(), stride=6, lo_=lo, h_=h, f=ff.field.data_ptr(),
             s=ff.status.data_ptr(), mode=0):
        return lib.gnbv_flight_field(b, n, nx, ny, nz, c, ps, stride, lo_, h_, f, s, mode, None)
    assert call() == 0
    for kw in (dict(b=None), dict(ps=None), dict(f=None), dict(s=None), dict(c=None), dict(lo_=None), dict(h_=None), dict(n=0), dict(nx=0),
               dict(nz=1025), dict(stride=2), dict(mode=-1), dict(mode=3), dict(c=zero_cost), dict(c=huge_cost), dict(h_=bad_h)):
        assert call(**kw) == 1, kw
    out = torch.zeros(7, 2, dtype=torch.int32, device=DEV)
    t = torch.zeros(7, 2, 6, device=DEV)
    assert lib.gnbv_flight_query(ff.field.data_ptr(), 7, 9, 7, 5, lo, h, t.data_ptr(), 2, 6, out.data_ptr(), None) == 0
    assert lib.gnbv_flight_query(ff.field.data_ptr(), 7, 9, 7, 5, lo, h, t.data_ptr(), 0, 6, out.data_ptr(), None) == 1
    assert lib.gnbv_flight_query(ff.field.data_ptr(), 7, 9, 7, 5, lo, h, t.data_ptr(), 2, 2, out.data_ptr(), None) == 1
    assert lib.gnbv_flight_query(None, 7, 9, 7, 5, lo, h, t.data_ptr(), 2, 6, out.data_ptr(), None) == 1
    nodes = torch.zeros(7, 4, dtype=torch.int32, device=DEV)
    ln = torch.zeros(7, dtype=torch.int32, device=DEV)
    assert lib.gnbv_flight_path(ff.field.data_ptr(), 7, 9, 7, 5, cost, lo, h, t.data_ptr(), 12, nodes.data_ptr(), 4, ln.data_ptr(), None) == 0
    assert lib.gnbv_flight_path(ff.field.data_ptr(), 7, 9, 7, 5, cost, lo, h, t.data_ptr(), 12, nodes.data_ptr(), 0, ln.data_ptr(), None) == 1
    assert lib.gnbv_flight_path(ff.field.data_ptr(), 7, 9, 7, 5, cost, lo, h, t.data_ptr(), 12, None, 4, ln.data_ptr(), None) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 2. query and path
# ---------------------------------------------------------------------------
def test_query_and_cost(small_case):
    lat, blocked, src, poses, want = small_case
    ff = _field(lat, blocked, 0).update(torch.as_tensor(poses).to(DEV))
    rs = np.random.RandomState(2)
    k = 9
    t = np.zeros((7, k, 6), f32)
    span = lat.h * (np.array(lat.dims) - 1)
    t[..., :3] = lat.lo + span * rs.uniform(-0.2, 1.2, (7, k, 3))  # also outside the lattice: clamped
    t[0, 0, 0], t[1, 1, 2] = np.nan, np.inf
    node = lat.nearest_np(t)
    assert (node[0, 0], node[1, 1]) == (-1, -1)
    want_mm = np.where(node >= 0, np.take_along_axis(want, np.maximum(node, 0), 1), INF_MM).astype(np.uint32)
    tt = torch.as_tensor(t).to(DEV)
    assert np.array_equal(_u32(ff.cost_mm(tt)), want_mm)
    wide = torch.zeros(7, k, 8, device=DEV)  # another row stride
    wide[..., :6] = tt
    assert np.array_equal(_u32(ff.cost_mm(wide[..., :6])), want_mm)
    assert np.array_equal(_u32(ff.cost_mm(tt[:, :1])), want_mm[:, :1])
    got = ff.cost(tt).cpu().numpy()
    fin = want_mm != INF_MM
    assert fin.any() and (~fin).any() and np.isinf(got[~fin]).all() and (got[~fin] > 0).all()
    pos = lat.node_positions()
    stub_t = np.linalg.norm(t[..., :3].astype(np.float64) - pos[np.maximum(node, 0)], axis=-1)
    stub_s = np.linalg.norm(poses[:, :3].astype(np.float64) - pos[src], axis=-1)[:, None]
    ref = want_mm.astype(np.float64) * 1e-3 + stub_t + stub_s
    assert np.allclose(got[fin], ref[fin], rtol=1e-6, atol=0)  # one rounding to fp32
    assert np.array_equal(ff.reachable(tt).cpu().numpy(), fin)


def test_paths_walk_the_field_like_the_oracle(small_case):
    from gennbv_amd import _lib
    lat, blocked, src, poses, want = small_case
    ff = _field(lat, blocked, 0).update(torch.as_tensor(poses).to(DEV))
    rs = np.random.RandomState(4)
    pos = lat.node_positions()
    routed = longest = 0
    for rep in range(6):
        tnode = rs.randint(0, lat.num_nodes, 7)
        if rep == 0:
            tnode[:4] = [np.argmax(np.where(want[e] == INF_MM, 0, want[e])) for e in range(4)]  # the farthest node of each env
        if rep == 1:
            tnode = src.copy()  # the target shares the source's node
        tp = torch.as_tensor(_poses(lat, tnode)).to(DEV)
        nodes, count = ff.path_nodes(tp)
        way, length = ff.path(tp)
        nodes, count, way, length = nodes.cpu().numpy(), count.cpu().numpy(), way.cpu().numpy(), length.cpu().numpy()
        for e in range(7):
            ref = FO.walk(want[e], lat.dims, lat.cost, int(tnode[e]))
            got = nodes[e, :count[e]].tolist()
            assert got == ref, (rep, e)  # the tie-break order is the oracle's
            if not ref:
                assert count[e] == 0 and length[e] == 0 and np.isnan(way[e]).all()
                continue
            routed, longest = routed + 1, max(longest, len(ref))
            assert got[0] == tnode[e] and got[-1] == src[e] and not blocked[e, got].any()
            total = 0
            for a, b in zip(got[:-1], got[1:]):
                d = np.abs(lat.node_index()[a] - lat.node_index()[b])
                assert d.max() == 1  # 26-adjacent
                total += int(lat.cost[FO.cost_index(*d)])
            assert total == want[e, tnode[e]]
            # waypoints: source pose, the nodes source -> target, target pose
            assert length[e] == len(ref) + 2
            assert np.array_equal(way[e, 0], poses[e, :3]) and np.array_equal(way[e, length[e] - 1], tp[e, :3].cpu().numpy())
            assert np.array_equal(way[e, 1:1 + len(ref)], pos[ref[::-1]].astype(f32))
            assert np.isnan(way[e, length[e]:]).all()
    assert routed >= 12 and longest >= 6
    # a buffer that is too short: -needed, and the first max_len nodes
    tnode = np.array([np.argmax(np.where(want[e] == INF_MM, 0, want[e])) for e in range(7)])
    tp = torch.as_tensor(_poses(lat, tnode)).to(DEV)
    full, count = ff.path_nodes(tp)
    short = torch.full((7, 3), -1, dtype=torch.int32, device=DEV)
    ln = torch.zeros(7, dtype=torch.int32, device=DEV)
    cost, lo, h = (C.c_uint32 * 8)(*lat.cost.tolist()), (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)
    _lib.check(_lib.load().gnbv_flight_path(ff.field.data_ptr(), 7, 9, 7, 5, cost, lo, h, tp.data_ptr(), 6, short.data_ptr(), 3, ln.data_ptr(),
                                            None), "gnbv_flight_path")
    count, ln = count.cpu().numpy(), ln.cpu().numpy()
    assert (count[:4] > 3).all()
    assert np.array_equal(ln, np.where(count > 3, -count, count))
    assert torch.equal(short[:4], full[:4, :3])
    assert (ff.path_nodes(tp, max_len=3)[1].cpu().numpy() == count).all()  # the op asks again with the length it was told


# ---------------------------------------------------------------------------
# 3. the free set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ground,seed", [(False, 3), (True, 4)])
def test_blocked_mask_equals_the_brute_force_oracles(ground, seed):
    from gennbv_amd.env.mesh_scene import MeshScene
    n = 2
    mesh = MeshScene.from_boxes(S.make_scenes(n, 20, seed=seed), device=DEV)
    lat = FlightLattice(TaskConfig(), stride=5)
    body = _body(ground=ground)
    m = lat.num_nodes
    bits = mesh.flight_blocked(lat, body, chunk=4096)  # several chunks
    assert bits.dtype == torch.int32 and bits.shape == (n, lat.words)
    got = FO.unpack_bits(bits.cpu().numpy(), m)
    pad = FO.unpack_bits(bits.cpu().numpy(), lat.words * 32)[:, m:]
    assert pad.all()
    assert torch.equal(bits, mesh.flight_blocked(lat, body))  # one chunk
    rho = lat.inflated_radius(body)
    assert rho > body.path_radius + 0.5 * lat.h_norm and f32(rho) >= body.path_radius + 0.5 * lat.h_norm
    nodes = np.zeros((m, 6), f32)
    nodes[:, :3] = lat.node_positions().astype(f32)
    env = np.repeat(np.arange(n), m)
    p = np.tile(nodes, (n, 1))
    path, robust = SO.SweepOracle.from_mesh(mesh).robust_codes(env, p, p, rho, ground)
    pose, robust_pose = CO.CollisionOracle.from_mesh(mesh).robust_codes(env, p, body.radius, body.half_length, False)
    want = ((path & (PATH | PATH_GROUND)) | (pose & 3)) != 0
    robust &= robust_pose
    got = got.reshape(-1)
    bad = np.nonzero(robust & (got != want))[0]
    assert bad.size == 0, [(int(env[i]), p[i, :3].tolist(), bool(got[i]), bool(want[i])) for i in bad[:5]]
    assert robust.mean() >= MIN_ROBUST, robust.mean()
    assert want.any() and not want.all()
    if ground:  # the lowest layer (z = 0.1) is all blocked, the next one (z = 1.1 > rho) is not
        assert got.reshape(n, -1)[:, :17 * 17].all() and not got.reshape(n, -1)[:, 17 * 17:2 * 17 * 17].all()


# ---------------------------------------------------------------------------
# 4. soundness, end to end
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [2, 5])
def test_every_leg_of_every_route_is_free_for_the_swept_sphere(stride):
    from gennbv_amd import _lib
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.ops.flight_field import FlightField
    n, k = 4, 8
    cfg = TaskConfig()
    mesh = MeshScene.from_boxes(S.make_scenes(n, 20, seed=2), device=DEV)
    body = _body()
    lat = FlightLattice(cfg, stride=stride)
    ff = FlightField(mesh, lat, body)
    lds = lat.num_nodes <= int(_lib.load().gnbv_flight_lds_max_nodes())
    assert lds == (stride == 5)  # the default task: stride 2 lands in the global regime, stride 5 in LDS
    rs = np.random.RandomState(stride)

    def lattice_poses(shape):
        a = np.stack([rs.randint(0, int(u) + 1, shape) for u in cfg.clip_pose_idx_up], -1)
        return torch.as_tensor((a.astype(f32) * np.array(cfg.action_unit, f32) + np.array(cfg.clip_pose_low, f32)).astype(f32)).to(DEV)
    legs = routes = detours = 0
    for rep in range(5):
        start = lattice_poses((n,))
        ff.update(start)
        targets = lattice_poses((n, k))
        straight = mesh.sweep_candidates(start, targets, body)
        reach = ff.reachable(targets)
        for j in range(k):
            way, length = ff.path(targets[:, j].contiguous())
            length = length.cpu().numpy()
            assert np.array_equal(length > 0, reach[:, j].cpu().numpy())
            steps = way.shape[1] - 1
            code = mesh.sweep_candidates(way[:, :-1].contiguous(), way[:, 1:].contiguous(), body).cpu().numpy()
            for e in range(n):
                if length[e] == 0:
                    continue
                assert (code[e, :length[e] - 1] == 0).all(), (rep, j, e, way[e, :length[e]].tolist())  # no leg is excluded
                assert steps >= length[e] - 1
                legs, routes = legs + int(length[e]) - 1, routes + 1
                detours += int(straight[e, j] != 0)
    ff.check()
    assert routes >= 20 and legs >= 5 * routes and detours >= 1  # routes were found, also where the straight flight is blocked


# ---------------------------------------------------------------------------
# 5. env and planner
# ---------------------------------------------------------------------------
WALL_ACTION = [60, 40, 50, 0, 6, 0]    # (4, 0, 10.1): behind the wall, seen from the init pose (0, 0, 10.1)
SEALED_ACTION = [20, 40, 25, 0, 6, 0]  # (-4, 0, 5.1): the middle of a closed hollow room
OPEN_ACTION = [40, 50, 50, 0, 6, 0]    # (0, 2, 10.1): open air


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


def _wall_env(n, flight, sweep=True, with_flight_arg=True):
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.ops.flight_field import FlightField
    cfg = TaskConfig(camera_width=64, camera_height=48, grid_size=20)
    mesh = _wall_scene(n)
    scene = mesh.ground_truth(20, torch.tensor([[8.0, -8.0, 8.0, -8.0, 12.0, 0.0]] * n))
    body = _body() if sweep else _body().__class__()
    kw = {}
    if with_flight_arg:
        kw["flight"] = FlightField(mesh, FlightLattice(cfg, stride=2), body) if flight else None
    return ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=30, collision=body, **kw), cfg


class _FixedCandidates:
    """LatticeCandidates' protocol over a fixed candidate list."""

    def __init__(self, cfg, actions, n):
        self.cfg, self.actions, self.n = cfg, torch.tensor(actions, dtype=torch.int64), n

    def sample(self, num_envs, device="cpu"):
        return self.actions[None].expand(num_envs, -1, -1).contiguous().to(device)

    def poses(self, actions):
        return S.poses_from_actions(actions, self.cfg).float()


def _policy(env, cfg, n):
    from gennbv_amd.eval.baselines import GreedyGainPolicy
    gains = torch.tensor([[100, 0, 0], [200, 0, 0], [1, 0, 0]], dtype=torch.int32, device=DEV)  # wall, sealed, open
    pol = GreedyGainPolicy(env, k=3, weights=(1, 0), gain_backend=lambda tri, poses: gains[None].expand(n, -1, -1))
    pol.cands = _FixedCandidates(cfg, [WALL_ACTION, SEALED_ACTION, OPEN_ACTION], n)
    assert pol.avoid_collisions and pol.sweep
    return pol


def test_env_and_planner_fly_round_the_wall():
    from gennbv_amd.ops.flight_field import FlightField
    n = 2
    wall = torch.tensor([WALL_ACTION] * n, device=DEV)
    # --- sweep=True, flight=None: straight-line blocked means unreachable
    env, cfg = _wall_env(n, flight=False)
    assert env.flight is None and env.flight_length is None
    obs = env.reset()
    pol = _policy(env, cfg, n)
    act = pol(obs)[0]
    assert act.tolist() == [OPEN_ACTION] * n
    assert (pol._contact[:, 0] & PATH).all() and (pol._contact[:, 1] & PATH).all() and not pol._contact[:, 2].any()
    assert not (pol._contact & 7).any()  # every candidate's pose itself is free
    _, _, done, _ = env.step(wall)
    assert done.all() and (env.collision_buf == PATH).all()
    # --- with the flight field
    env, cfg = _wall_env(n, flight=True)
    obs = env.reset()
    assert env.flight.launches == 1 and not env.flight_length.any()
    pol = _policy(env, cfg, n)
    act = pol(obs)[0]
    assert act.tolist() == [WALL_ACTION] * n  # the sealed room has the larger gain and stays refused
    assert not pol._contact[:, 0].any() and (pol._contact[:, 1] & PATH).all() and not pol._contact[:, 2].any()
    start = env.poses.clone()
    target = S.poses_from_actions(wall, cfg).float()
    probe = FlightField(env.collision_mesh, env.flight.lattice, env.collision, blocked=env.flight.blocked).update(start)
    assert torch.equal(probe.field, env.flight.field)
    sealed = S.poses_from_actions(torch.tensor([SEALED_ACTION] * n, device=DEV), cfg).float()
    assert torch.isinf(env.flight.cost(sealed[:, None])).all()
    _, _, done, _ = env.step(act)
    assert not done.any() and not env.collision_buf.any()
    assert torch.allclose(env.poses[:, :3], target[:, :3], atol=1e-5)
    want = probe.cost(env.poses[:, None])[:, 0]  # FlightField.cost of the step: the field from the previous pose, the pose flown to
    straight = (env.poses[:, :3] - start[:, :3]).norm(dim=-1)
    assert torch.equal(env.flight_length, want) and (want > straight + 1.0).all() and torch.isfinite(want).all()
    assert env.flight.launches == 2  # one field per step
    assert torch.equal(env.flight.source, env.poses[:, :3])
    # a free straight flight adds its own length
    open_a = torch.tensor([OPEN_ACTION] * n, device=DEV)
    before, here = env.flight_length.clone(), env.poses.clone()
    _, _, done, _ = env.step(open_a)
    # (4, 0) -> (0, 2) crosses the wall: again a detour
    assert not done.any() and (env.flight_length > before + (env.poses[:, :3] - here[:, :3]).norm(dim=-1) + 1.0).all()
    before, here = env.flight_length.clone(), env.poses.clone()
    up = torch.tensor([[40, 60, 50, 0, 6, 0]] * n, device=DEV)  # (0, 4, 10.1): open air all the way
    _, _, done, _ = env.step(up)
    leg = (env.poses[:, :3] - here[:, :3]).norm(dim=-1)
    assert not done.any() and torch.equal(env.flight_length, before + leg)
    # flying into the sealed room has no route: the episode ends on the path bit, and the next episode starts at 0
    _, _, done, _ = env.step(torch.tensor([SEALED_ACTION] * n, device=DEV))
    assert done.all() and (env.collision_buf == PATH).all()
    env.step(open_a)  # the forced init pose: set, not flown to
    assert not env.flight_length.any()
    env.flight.check()


def test_flight_needs_the_sweep_and_none_changes_nothing():
    n = 2
    with pytest.raises(ValueError):
        _wall_env(n, flight=True, sweep=False)
    runs = []
    gen = torch.Generator().manual_seed(3)
    acts = [torch.stack([torch.randint(0, int(u) + 1, (n,), generator=gen) for u in TaskConfig().clip_pose_idx_up], -1).to(DEV)
            for _ in range(10)]
    acts[0] = torch.tensor([WALL_ACTION] * n, device=DEV)  # flown to from the init pose: through the wall
    for with_arg in (True, False):
        env, _ = _wall_env(n, flight=False, with_flight_arg=with_arg)
        env.reset()
        out = []
        for a in acts:
            _, rew, done, _ = env.step(a)
            out.append((env.collision_buf.clone(), rew.clone(), done.clone()))
        runs.append(out)
    for (c0, r0, d0), (c1, r1, d1) in zip(*runs):
        assert torch.equal(c0, c1) and torch.equal(r0, r1) and torch.equal(d0, d1)
    assert any(bool(c.any()) for c, _, _ in runs[0])

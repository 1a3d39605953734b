"""GPU: the cautious map pilot -- gnbv_flight_classify_tri (csrc/flightmap.hip) against the numpy oracle of the blocked bits called
twice and composed, and against two real gnbv_flight_blocked_tri launches; BeliefFlightField(unknown="costly"); the env that
flies the penalised route, against a host re-enactment from the oracle's walk; MapGreedyPolicy's risk budget.  The inputs are
those of tests/test_flightmap_gpu.py and tests/test_sweepmap_gpu.py (their cached cases and oracle words are shared)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gennbv_amd.env.flight import INF_MM
from tests import flight_oracle as FO
from tests import flight_w_oracle as WO
from tests import flightmap_oracle as MO
from tests import sweepmap_oracle as SO
from tests import test_flightmap_gpu as TM
from tests import test_sweepmap_gpu as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
INVALID = 1  # hipErrorInvalidValue
RHO, N_ENVS = TM.RHO, TM.N_ENVS
POISON_B, POISON_C = 0x5A5A5A5A, 0x3C3C3C3C


def _compose(blocked_free, blocked_unknown):
    """The issue's definition: blocked = blocked_tri(unknown_blocks = 0), padding set; costly = blocked_tri(unknown_blocks = 1) &
    ~blocked, padding clear (both inputs have their padding set)."""
    return blocked_free, blocked_unknown & ~blocked_free


def _classify(lat, tri_t, g, rng_t, vox_t, rho, outside, ground, mode):
    """gnbv_flight_classify_tri at the C ABI -> (return code, blocked words, costly words)."""
    from gennbv_amd import _lib
    lib = _lib.load()
    n = tri_t.shape[0]
    out_b = torch.full((n, lat.words), POISON_B, dtype=torch.int32, device=DEV)
    out_c = torch.full((n, lat.words), POISON_C, dtype=torch.int32, device=DEV)
    lo, h = (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)
    i8 = tri_t.dtype == torch.int8
    row = int(tri_t.stride(0)) if n > 1 else g ** 3
    nx, ny, nz = lat.dims
    err = lib.gnbv_flight_classify_tri(tri_t.data_ptr() if i8 else None, row if i8 else 0, None if i8 else tri_t.data_ptr(), 0 if i8 else row,
                                       g, rng_t.data_ptr(), vox_t.data_ptr(), n, nx, ny, nz, lo, h, float(rho), int(outside), int(ground),
                                       out_b.data_ptr(), out_c.data_ptr(), mode, None)
    torch.cuda.synchronize()
    return err, out_b.cpu().numpy().view(np.uint32), out_c.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("g", [12, 8])
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_classes_equal_the_composed_oracle_and_two_real_launches(g, mode):
    tri, rng, vox = TM._case(g)
    lat = TM._lattice()
    forms = TM._forms(tri, g)
    rng_t, vox_t = torch.as_tensor(rng).to(DEV), torch.as_tensor(vox).to(DEV)
    tail_mask = np.uint32((1 << (lat.num_nodes & 31)) - 1)
    for outside in (0, 1):
        for ground in (0, 1):
            want_b, want_c = _compose(TM._want(g, 0, outside, ground), TM._want(g, 1, outside, ground))
            for name, t in forms.items():
                err, got_b, got_c = _classify(lat, t, g, rng_t, vox_t, RHO, outside, ground, mode)
                assert err == 0
                assert np.array_equal(got_b, want_b), (outside, ground, name, np.argwhere(got_b != want_b)[:5].tolist())
                assert np.array_equal(got_c, want_c), (outside, ground, name, np.argwhere(got_c != want_c)[:5].tolist())
                real = [TM._launch(lat, t, g, rng_t, vox_t, RHO, (u, outside, ground), mode) for u in (0, 1)]
                assert real[0][0] == 0 and real[1][0] == 0
                two_b, two_c = _compose(real[0][1], real[1][1])
                assert np.array_equal(got_b, two_b) and np.array_equal(got_c, two_c)
            assert (want_b[:, -1] & ~tail_mask == ~tail_mask).all() and not (want_c[:, -1] & ~tail_mask).any()  # padding: set, clear
            assert not (want_b & want_c).any()
    # the cases reach what they are there for: all unknown is all costly, all free / all occupied has nothing costly, the sparse grid has all three
    want_b, want_c = _compose(TM._want(g, 0, 0, 0), TM._want(g, 1, 0, 0))
    bits = lambda words: int(sum(bin(int(x)).count("1") for x in words))  # noqa: E731
    assert bits(want_c[2]) == lat.num_nodes and bits(want_c[1]) == 0 and bits(want_c[3]) == 0
    assert bits(want_c[5]) > 10 and bits(want_b[5]) - 5 > 10 and bits(want_c[5]) + bits(want_b[5]) - 5 < lat.num_nodes - 10  # the sparse grid


def test_the_lds_limit_of_two_planes():
    """At the largest grid whose two planes fit LDS (more than a launch may ask for without the attribute) all three modes agree
    with the oracle; one above it mode 1 is refused by the return code before anything is launched, modes 0 and 2 read the grid
    in place."""
    from gennbv_amd import _lib
    lib = _lib.load()
    cap = int(lib.gnbv_flightmap_classify_lds_max_grid())
    assert 1 <= cap < int(lib.gnbv_flightmap_lds_max_grid())  # two planes hold less than one
    lat = TM._lattice()
    rs = np.random.RandomState(3)
    for g in (cap, cap + 1):
        tri = np.full((1, g, g, g), -1, np.int8)
        u = rs.rand(1, g, g, g)
        tri[u < 0.0002], tri[(u >= 0.0002) & (u < 0.0006)] = 1, 0  # very sparse (a ball holds thousands of voxels): all three classes occur
        rng, vox = TM._frames(g)
        rng, vox = rng[:1], vox[:1]
        want_b, want_c = _compose(*[MO.blocked_words(tri, rng, vox, lat.dims, lat.lo, lat.h, RHO, unk, False, False) for unk in (False, True)])
        count = lambda w: sum(bin(int(x)).count("1") for x in w[0])  # noqa: E731
        assert count(want_b) - 5 > 20 and count(want_c) > 20 and count(want_b) - 5 + count(want_c) < lat.num_nodes - 20
        rng_t, vox_t = torch.as_tensor(rng).to(DEV), torch.as_tensor(vox).to(DEV)
        forms = {"i8": torch.as_tensor(tri.reshape(1, -1)).to(DEV), "f32": torch.as_tensor(tri.reshape(1, -1).astype(f32)).to(DEV)}
        for name, t in forms.items():
            for mode in (0, 1, 2):
                err, got_b, got_c = _classify(lat, t, g, rng_t, vox_t, RHO, 0, 0, mode)
                if mode == 1 and g > cap:
                    assert err == INVALID and (got_b == POISON_B).all() and (got_c == POISON_C).all()  # nothing was launched
                else:
                    assert err == 0 and np.array_equal(got_b, want_b) and np.array_equal(got_c, want_c), (g, name, mode)


# ---------------------------------------------------------------------------
# 2. BeliefFlightField(unknown="costly")
# ---------------------------------------------------------------------------
def test_cautious_field_refresh_update_paths_and_counts():
    from gennbv_amd import _lib
    from gennbv_amd.ops.flight_field import BeliefFlightField, field_u32
    g = 12
    tri, rng, vox = TM._case(g)
    lat = TM._lattice()
    body = TM._body(sweep_radius=0.05, ground=True)
    kw = dict(margin=0.02, device=DEV, shortcut=True)
    ff = BeliefFlightField(N_ENVS, lat, body, torch.as_tensor(rng), torch.as_tensor(vox), g, unknown="costly", unknown_penalty_m=0.777, **kw)
    assert ff.belief and ff.penalty_mm == 777 and ff.costly is ff.costly_map and ff.unknown == "costly"
    assert (field_u32(ff.blocked_map) == 0xFFFFFFFF).all() and not ff.costly_map.any()  # nothing is flyable before the first refresh
    want_b, want_c = _compose(*[MO.blocked_words(tri, rng, vox, lat.dims, lat.lo, lat.h, ff.rho, unk, False, True) for unk in (False, True)])
    forms = TM._forms(tri, g)
    for t in forms.values():
        ff.blocked_map.fill_(0)
        ff.costly_map.fill_(-1)
        assert ff.refresh(t) is ff
        assert np.array_equal(field_u32(ff.blocked_map), want_b) and np.array_equal(field_u32(ff.costly_map), want_c)
    assert ff.refreshes == 2
    # update(): the source bit is cleared in `blocked` only; blocked_map and costly_map stay the pure kernel output
    nodes = np.array([0, 100, 157, 314, 31, 32])
    poses = np.zeros((N_ENVS, 6), f32)
    poses[:, :3] = lat.node_positions()[nodes] + 0.3 * lat.h * np.array([1, -1, 1])
    poses[4, 1] = np.nan
    ff.update(torch.as_tensor(poses).to(DEV))
    assert np.array_equal(field_u32(ff.blocked_map), want_b) and np.array_equal(field_u32(ff.costly_map), want_c)
    cleared = want_b.copy()
    for e in (0, 1, 2, 3, 5):
        cleared[e, nodes[e] >> 5] &= ~np.uint32(1 << (nodes[e] & 31))
    assert np.array_equal(field_u32(ff.blocked), cleared) and (cleared != want_b).any()
    blocked = FO.unpack_bits(cleared.view(np.int32), lat.num_nodes)
    costly = FO.unpack_bits(want_c.view(np.int32), lat.num_nodes)
    field = field_u32(ff.field)
    ref = np.stack([WO.dijkstra_w(blocked[e], costly[e], lat.dims, lat.cost, -1 if e == 4 else int(nodes[e]), 777) for e in range(N_ENVS)])
    assert np.array_equal(field, ref)
    plain = np.stack([FO.dijkstra(blocked[e], lat.dims, lat.cost, -1 if e == 4 else int(nodes[e])) for e in range(N_ENVS)])
    assert np.array_equal(field == INF_MM, plain == INF_MM) and (field[2] > plain[2]).any()  # (env 2 is all unknown: every hop pays)
    ff.check()
    # the walk, the counts and the penalised cost
    rs = np.random.RandomState(6)
    seen = 0
    for _ in range(3):
        tnode = rs.randint(0, lat.num_nodes, N_ENVS)
        for e in (1, 2, 5):  # three envs aim at nodes a route reaches (env 2: through unknown space, whichever it is; env 0 has none)
            tnode[e] = rs.choice(np.nonzero((ref[e] != INF_MM) & (ref[e] != 0))[0])
        tpose = np.zeros((N_ENVS, 6), f32)
        tpose[:, :3] = lat.node_positions()[tnode]
        t = torch.as_tensor(tpose).to(DEV)
        got_nodes, got_count = ff.path_nodes(t)
        unknown = ff.costly_count(got_nodes, got_count).cpu().numpy()
        assert unknown.dtype == np.int64
        mm = field_u32(ff.cost_mm(t[:, None]))[:, 0]
        assert np.array_equal(mm, ref[np.arange(N_ENVS), tnode])
        assert np.array_equal(ff.reachable(t[:, None])[:, 0].cpu().numpy(), mm != INF_MM)
        for e in range(N_ENVS):
            want = WO.walk_w(ref[e], costly[e], lat.dims, lat.cost, 777, int(tnode[e]))
            assert got_nodes[e, :int(got_count[e])].tolist() == want and int(got_count[e]) == len(want)
            assert unknown[e] == int(costly[e][want[:-1]].sum()) if want else unknown[e] == 0
            if want:
                geometric = WO.route_cost(want, np.zeros_like(costly[e]), lat.dims, lat.cost, 0)
                assert int(mm[e]) == geometric + 777 * int(unknown[e])
                seen += int(unknown[e] > 0)
    assert seen >= 3
    at = ff.costly_at(torch.tensor([[0, -1, 314]] * N_ENVS, device=DEV)).cpu().numpy()
    assert np.array_equal(at[:, 0], costly[:, 0]) and not at[:, 1].any() and np.array_equal(at[:, 2], costly[:, 314])
    # pairwise_mm stays geometric (the plain kernel over `blocked`), sweep judges with unknown voxels blocking
    strict = BeliefFlightField(N_ENVS, lat, body, torch.as_tensor(rng), torch.as_tensor(vox), g, unknown="blocked", **kw)
    loose = BeliefFlightField(N_ENVS, lat, body, torch.as_tensor(rng), torch.as_tensor(vox), g, unknown="free", **kw)
    strict.refresh(forms["i8"])
    loose.refresh(forms["i8"]).update(torch.as_tensor(poses).to(DEV))
    assert loose.costly_map is None and loose.costly is None and np.array_equal(field_u32(loose.blocked), cleared)
    pts = torch.as_tensor(poses[:, None, :].repeat(3, 1)).to(DEV)
    pts[:, 1, :3] = torch.as_tensor(lat.node_positions()[[8] * N_ENVS].astype(f32)).to(DEV)
    pts[:, 2, :3] = torch.as_tensor(lat.node_positions()[[200] * N_ENVS].astype(f32)).to(DEV)
    assert torch.equal(ff.pairwise_mm(pts), loose.pairwise_mm(pts))
    assert np.array_equal(field_u32(ff.field), ref)  # the private field of pairwise_mm: update() state untouched
    frm = torch.as_tensor(poses).to(DEV).nan_to_num(0.0)
    assert torch.equal(ff.sweep(frm, pts), strict.sweep(frm, pts)) and ff.sweeps == 1
    with pytest.raises(_lib.GennbvHipError):
        loose.costly_at(torch.zeros(N_ENVS, 1, dtype=torch.int64, device=DEV))
    cap = int(_lib.load().gnbv_flightmap_classify_lds_max_grid())
    with pytest.raises(_lib.GennbvHipError):  # map_mode 1 above the two-plane limit
        BeliefFlightField(1, lat, body, torch.as_tensor(rng[:1]), torch.as_tensor(vox[:1]), cap + 1, map_mode=1, device=DEV, unknown="costly",
                          unknown_penalty_m=1.0)


# ---------------------------------------------------------------------------
# 3. the env flies the penalised route, the truth judges it
# ---------------------------------------------------------------------------
ENV_N, ENV_G = TS.ENV_N, TS.ENV_G
PENALTY_M = 5.0


@pytest.mark.parametrize("shortcut", [False, True])
def test_env_flies_the_cautious_route_and_counts_its_unknown_nodes(shortcut):
    from gennbv_amd.ops.flight_field import field_u32
    env, cfg, scene, mesh, lat, body = TS._belief_env("costly", shortcut=shortcut, unknown_penalty_m=PENALTY_M)
    n, fl, m = ENV_N, env.flight, lat.num_nodes
    pen = 5000
    assert fl.penalty_mm == pen and (env.skipped is not None) == shortcut
    rng, vox = scene.range_gt.numpy(), scene.voxel_size.numpy()
    pos32 = lat.node_positions().astype(f32)
    gen = torch.Generator().manual_seed(11)
    obs = env.reset()
    assert fl.refreshes == 1 and fl.launches == 1 and fl.sweeps == 0 and not env.flight_length.any() and int(env.route_overflow) == 0
    assert env.route_unknown.dtype == torch.int64 and not env.route_unknown.any()
    saw = {"routed": 0, "unrouted": 0, "first": 0, "hit": 0, "unknown": 0, "skipped": 0, "legs": 0, "weak": 0}

    def check_map(obs):
        """The pilot's knowledge after a step is the oracle's: both maps, the cleared source bit, the penalised field."""
        tri = TS._tri_of(obs, cfg)
        want_b, want_c = _compose(*[MO.blocked_words(tri, rng, vox, lat.dims, lat.lo, lat.h, fl.rho, unk, False, False) for unk in (False, True)])
        assert np.array_equal(field_u32(fl.blocked_map), want_b) and np.array_equal(field_u32(fl.costly_map), want_c)
        node = lat.nearest_np(env.poses.cpu().numpy())
        cleared = want_b.copy()
        for e in range(n):
            cleared[e, node[e] >> 5] &= ~np.uint32(1 << (node[e] & 31))
        assert np.array_equal(field_u32(fl.blocked), cleared)
        blocked, costly = FO.unpack_bits(cleared.view(np.int32), m), FO.unpack_bits(want_c.view(np.int32), m)
        field = field_u32(fl.field)
        for e in range(n):
            assert np.array_equal(field[e], WO.dijkstra_w(blocked[e], costly[e], lat.dims, lat.cost, int(node[e]), pen)), e
        return tri, costly, field
    tri_prev, costly_prev, field_prev = check_map(obs)
    for step in range(7):
        act = torch.stack([torch.randint(0, int(u) + 1, (n,), generator=gen) for u in cfg.clip_pose_idx_up], -1).to(DEV)
        prev, ep, length_before = env.poses.clone(), env.episode_length_buf.clone() + 1, env.flight_length.clone()
        obs, _, done, _ = env.step(act)
        new = env.poses.clone()
        # --- the host re-enactment: the oracle's walk over the map the pilot had, one MeshScene.sweep per flown leg
        prev_np, new_np, first = prev.cpu().numpy(), new.cpu().numpy(), (ep <= 1).cpu().numpy()
        target = lat.nearest_np(new_np)
        flown, skipped, routed, unknown, metres, legs_flown = [], np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n), 0
        for e in range(n):
            route = WO.walk_w(field_prev[e], costly_prev[e], lat.dims, lat.cost, pen, int(target[e]))[::-1]  # source -> target
            c = len(route)
            pts = np.concatenate([prev_np[e:e + 1, :3], pos32[route].reshape(c, 3), new_np[e:e + 1, :3]]).astype(f32)  # w_0 .. w_{c+1}
            jstar = 1
            if shortcut:  # the farthest waypoint whose straight leg the map -- unknown voxels blocking -- shows in the clear
                code, robust = SO.codes(tri_prev[e:e + 1], rng[e:e + 1], vox[e:e + 1], pts[None, 0], pts[None, 1:], fl.sweep_radius,
                                        True, False, False)
                got = env._map_codes.cpu().numpy()[e, :c + 1]
                assert SO.agrees(got[None], code, robust), (step, e)
                code = np.where(robust[0], code[0], got)  # a non-robust leg takes the kernel's answer
                saw["legs"] += c + 1
                saw["weak"] += int((~robust).sum())
                clear = np.nonzero(code == 0)[0]
                jstar = int(clear.max()) + 1 if clear.size else 1
                skipped[e] = 0 if first[e] else jstar - 1
            flown.append(np.concatenate([pts[:1], pts[jstar:]]))
            routed[e] = jstar <= c and not first[e]
            entered = route[max(jstar, 2) - 1:]  # waypoint j is route[j - 1]; waypoint 1 is the node the drone sat at
            unknown[e] = 0 if first[e] else int(costly_prev[e][entered].sum())
            metres[e] = sum(float(np.linalg.norm((flown[e][i + 1] - flown[e][i]).astype(np.float64))) for i in range(len(flown[e]) - 1))
            legs_flown = max(legs_flown, len(flown[e]) - 1)
        code = TS._judge(mesh, body, ep, prev_np[:, :3], flown)
        assert torch.equal(env.path_code, code), (step, env.path_code.tolist(), code.tolist())
        assert torch.equal(env.collision_buf & 24, code)  # in full: nothing is dropped
        assert torch.equal(env.collision_buf & 7, mesh.collide(new, body))
        assert torch.equal(env.routed.cpu(), torch.as_tensor(routed)), (step, env.routed.tolist(), routed.tolist())
        assert torch.equal(env.route_unknown.cpu(), torch.as_tensor(unknown)), (step, env.route_unknown.tolist(), unknown.tolist())
        if shortcut:
            assert torch.equal(env.skipped.cpu(), torch.as_tensor(skipped)), (step, env.skipped.tolist(), skipped.tolist())
        # metres, not the field's cost: every leg's norm and every addition rounds once in fp32 (2^-24 relative each, a handful per
        # leg), the re-enactment adds in fp64
        want_len = np.where(first, 0.0, length_before.cpu().numpy().astype(np.float64) + metres)
        tol = 4.0 * (legs_flown + 1) * 2.0 ** -24 * np.maximum(want_len, 1.0)
        assert (np.abs(env.flight_length.cpu().numpy() - want_len) <= tol).all(), (step, env.flight_length.tolist(), want_len.tolist())
        first_t = torch.as_tensor(first).to(DEV)
        assert not env.flight_length[first_t].any() and not (code[first_t] != 0).any() and not env.route_unknown[first_t].any()
        assert done[env.collision_buf != 0].all()  # what the truth found ends the episode
        saw["routed"] += int(routed.sum())
        saw["unrouted"] += int((~routed & ~first).sum())
        saw["first"] += int(first.sum())
        saw["hit"] += int((code != 0).sum())
        saw["unknown"] += int(unknown.sum())
        saw["skipped"] += int(skipped.sum())
        tri_prev, costly_prev, field_prev = check_map(obs)
    assert fl.refreshes == 8 and fl.launches == 8 and fl.sweeps == (7 if shortcut else 0) and int(env.route_overflow) == 0
    fl.check()
    assert saw["first"] >= n  # an episode boundary was crossed
    assert saw["routed"] >= 1  # unlike the conservative pilot, the cautious one moves along routes
    assert saw["weak"] <= 0.01 * max(saw["legs"], 1)
    print("cautious env, shortcut", shortcut, saw)


class _NoNewKernel:
    """The library with the new entry points taken away: any launch of them fails the test."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in ("gnbv_flight_classify_tri", "gnbv_flight_field_w", "gnbv_flight_path_w"):
            raise AssertionError(f"{name} was asked for by a field that puts no price on unknown space")
        return getattr(self._lib, name)


@pytest.mark.parametrize("shortcut", [False, True])
def test_a_free_field_launches_nothing_new(shortcut):
    env, cfg, scene, mesh, lat, body = TS._belief_env("free", shortcut=shortcut)
    fl = env.flight
    fl.lib = _NoNewKernel(fl.lib)
    assert fl.costly_map is None and fl.costly is None and fl.penalty_mm == 0
    gen = torch.Generator().manual_seed(11)
    env.reset()
    for _ in range(5):  # across an episode boundary (max_len = 4)
        act = torch.stack([torch.randint(0, int(u) + 1, (ENV_N,), generator=gen) for u in cfg.clip_pose_idx_up], -1).to(DEV)
        env.step(act)
        assert env.route_unknown is None
    fl.path(env.poses)
    assert fl.refreshes == 6 and fl.launches == 6


# ---------------------------------------------------------------------------
# 4. the planner's risk budget
# ---------------------------------------------------------------------------
def test_map_greedy_refuses_what_costs_more_than_the_budget():
    from gennbv_amd.eval.baselines import MapGreedyPolicy
    env, cfg, scene, mesh, lat, body = TS._belief_env("costly", shortcut=False, max_len=30, unknown_penalty_m=PENALTY_M)
    n = ENV_N
    obs = env.reset()
    # a map of the planner's own: free everywhere but an UNKNOWN slab, x voxels 12 .. 14 (1.7 .. 4.2 m), every y, every z: whatever
    # reaches the far side enters unknown nodes, three node layers at least
    tri = torch.full((n, ENV_G, ENV_G, ENV_G), -1, dtype=torch.int8, device=DEV)
    tri[:, 12:15] = 0
    env.flight.refresh(tri.reshape(n, -1)).update(env.poses)
    behind, before = [30, 16, 20, 0, 6, 0], [10, 16, 20, 0, 6, 0]  # (7, 0, 10.1) behind the slab, (-3, 0, 10.1) on the drone's side
    gains = torch.tensor([[300, 0, 0], [100, 0, 0]], dtype=torch.int32, device=DEV)
    real = env.collision_mesh
    env.collision_mesh = TM._NoMesh()
    try:
        picks = {}
        for budget in (None, 12.0):
            pol = MapGreedyPolicy(env, k=2, weights=(1, 0), gain_backend=lambda t, p: gains[None].expand(n, -1, -1), max_cost_m=budget)
            pol.cands = TM._Fixed(cfg, [behind, before])
            picks[budget] = (pol(obs)[0].tolist(), pol._contact.tolist())
        poses = pol.cands.poses(pol.cands.sample(n, DEV))
        cost = env.flight.cost(poses)
        crossed = env.flight.costly_count(*env.flight.path_nodes(poses[:, 0].contiguous()))
    finally:
        env.collision_mesh = real
    assert torch.isfinite(cost).all() and (crossed >= 3).all()
    assert (cost[:, 0] > 7.0 + 3 * PENALTY_M - 1.0).all() and (cost[:, 1] < 4.0).all()  # 7 m and the penalties; 3 m and none
    assert picks[None] == ([behind] * n, [[0, 0]] * n)  # reachable, the larger gain: chosen
    assert picks[12.0] == ([before] * n, [[1, 0]] * n)  # over the budget: refused

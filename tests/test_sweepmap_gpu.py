"""GPU: the swept sphere on the scanned map -- gnbv_sweep_tri (csrc/sweepmap.hip) against the numpy oracle
(tests/sweepmap_oracle.py: robust items bit for bit, the others in every bit but MAP) in both modes, both grid forms, both `from`
forms and every flag combination; its agreement with the node kernel; the LDS limit; BeliefFlightField.sweep and its map
snapshot; the env that flies straight to the farthest waypoint its map shows in the clear, against a host re-enactment; and
MapGreedyPolicy's shortcut."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import PI, TaskConfig
from gennbv_amd.env.flight import FlightLattice
from tests import flightmap_oracle as MO
from tests import sweepmap_cases as SC
from tests import sweepmap_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
INVALID = 1  # hipErrorInvalidValue
GUARD = 32


def _launch(tri_t, g, rng_t, vox_t, frm_t, to_t, radius, flags, mode):
    """gnbv_sweep_tri at the C ABI: tri_t int8 or float32 [N, >= G^3] with any row stride, frm_t [N, >= 3] (one start per env) or
    [N, K, >= 3], to_t [N, K, >= 3] -> (return code, codes uint8 [N,K], the bytes round [N,K] untouched)."""
    from gennbv_amd import _lib
    lib = _lib.load()
    n, k = to_t.shape[0], to_t.shape[1]
    buf = torch.full((n * k + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    i8 = tri_t.dtype == torch.int8
    row = int(tri_t.stride(0)) if n > 1 else g ** 3
    f_env, f_item = (int(frm_t.stride(0)), 0) if frm_t.dim() == 2 else (int(frm_t.stride(0)), int(frm_t.stride(1)))
    err = lib.gnbv_sweep_tri(tri_t.data_ptr() if i8 else None, row if i8 else 0, None if i8 else tri_t.data_ptr(), 0 if i8 else row, g,
                             rng_t.data_ptr(), vox_t.data_ptr(), n, frm_t.data_ptr(), max(f_env, 3), f_item, to_t.data_ptr(), k,
                             int(to_t.stride(1)), float(radius), *[int(f) for f in flags], buf.data_ptr() + GUARD, mode, None)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    guard_ok = bool((out[:GUARD] == 0xA5).all() and (out[-GUARD:] == 0xA5).all())
    return err, out[GUARD:-GUARD].reshape(n, k), guard_ok


def _forms(tri, g):
    """The two grid forms on the device: int8 rows with a padded row stride, fp32 rows inside an observation-shaped buffer."""
    n, g3 = tri.shape[0], g ** 3
    i8 = torch.full((n, g3 + 5), 77, dtype=torch.int8, device=DEV)
    i8[:, :g3] = torch.tensor(tri.reshape(n, g3)).to(DEV)
    obs = torch.full((n, 7 + g3 + 3), 5.0, dtype=torch.float32, device=DEV)  # [state | grid | rgb]: everything round the grid > 0
    obs[:, 7:7 + g3] = torch.tensor(tri.reshape(n, g3).astype(f32)).to(DEV)
    return {"i8": i8[:, :g3], "f32": obs[:, 7:7 + g3]}


def _dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(DEV) for a in arrays]  # (a copy: the shared cases are read-only)


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("g", [12, 8])
@pytest.mark.parametrize("mode", [1, 2])
def test_codes_equal_the_oracle(g, mode):
    tri, rng, vox = SC.case(g)
    frm, to, start = SC.legs(g)
    forms = _forms(tri, g)
    rng_t, vox_t, frm_t, to_t, start_t = _dev(rng, vox, frm, to, start)
    for broadcast, f_t in ((False, frm_t), (True, start_t)):
        for radius in SC.RADII:
            for flags in SC.FLAGS:
                want, robust = SC.want(g, broadcast, radius, flags)
                for name, t in forms.items():
                    err, got, guard_ok = _launch(t, g, rng_t, vox_t, f_t, to_t, radius, flags, mode)
                    assert err == 0 and guard_ok
                    assert SO.agrees(got, want, robust), (broadcast, radius, flags, name, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("g", [12, 8])
def test_mode_0_equals_both_and_unknown_blocks_is_a_superset(g):
    tri, rng, vox = SC.case(g)
    frm, to, _ = SC.legs(g)
    t = _forms(tri, g)["i8"]
    rng_t, vox_t, frm_t, to_t = _dev(rng, vox, frm, to)
    for radius in SC.RADII:
        for flags in ((0, 0, 0), (1, 1, 1)):
            got = [_launch(t, g, rng_t, vox_t, frm_t, to_t, radius, flags, mode) for mode in (0, 1, 2)]
            assert all(err == 0 and ok for err, _, ok in got)
            assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][1], got[2][1])
        for o in (0, 1):
            for gr in (0, 1):
                _, without, _ = _launch(t, g, rng_t, vox_t, frm_t, to_t, radius, (0, o, gr), 0)
                _, with_unknown, _ = _launch(t, g, rng_t, vox_t, frm_t, to_t, radius, (1, o, gr), 0)
                assert (without & ~with_unknown == 0).all() and (with_unknown != without).any()


def test_zero_length_legs_agree_with_the_node_kernel():
    """Zero-length legs at all 315 nodes of the 9 x 7 x 5 lattice with R = rho: bit 0, ORed with the OUTSIDE and GROUND bits, is the
    bit of gnbv_flight_blocked_tri on every robust node."""
    from gennbv_amd import _lib
    lib = _lib.load()
    g, rho = 12, 0.23
    tri, rng, vox = SC.case(g)
    lat = SC.lattice()
    nodes = np.broadcast_to(lat.node_positions().astype(f32)[None], (SC.N_ENVS, 315, 3))
    t = _forms(tri, g)["i8"]
    rng_t, vox_t, nodes_t = _dev(rng, vox, nodes)
    dist = SO.min_dist(tri, rng, vox, nodes, nodes)
    lo, h = (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)
    both = 0
    for flags in ((0, 0, 0), (1, 0, 0), (1, 1, 1), (0, 1, 1)):
        words = torch.zeros(SC.N_ENVS, lat.words, dtype=torch.int32, device=DEV)
        assert lib.gnbv_flight_blocked_tri(t.data_ptr(), int(t.stride(0)), None, 0, g, rng_t.data_ptr(), vox_t.data_ptr(), SC.N_ENVS, 9, 7, 5,
                                           lo, h, rho, *flags, words.data_ptr(), 0, None) == 0
        err, got, guard_ok = _launch(t, g, rng_t, vox_t, nodes_t, nodes_t, rho, flags, 0)
        assert err == 0 and guard_ok
        w = words.cpu().numpy().view(np.uint32)
        node_bit = ((w[:, np.arange(315) >> 5] >> (np.arange(315) & 31).astype(np.uint32)) & 1).astype(bool)
        want, robust = SO.codes_from(dist, g, rng, vox, nodes, nodes, rho, *[bool(f) for f in flags])
        assert SO.agrees(got, want, robust) and robust.mean() >= 0.99
        assert np.array_equal((got != 0)[robust], node_bit[robust]), flags
        both += int(node_bit[robust].any() and not node_bit[robust].all())
    assert both == 4


def test_the_lds_limit_and_the_largest_grid():
    """G = 109 is the largest grid whose bits fit LDS (more than a launch may ask for without the attribute): mode 1 serves it; at 110
    mode 1 is refused by the return code before anything is launched; 128^3 is read in place."""
    from gennbv_amd import _lib
    cap = int(_lib.load().gnbv_sweepmap_lds_max_grid())
    assert cap == 109
    for g, modes in ((cap, (1, 0, 2)), (cap + 1, (1, 0, 2)), (128, (2, 0))):
        tri, rng, vox, frm, to, want, robust = SC.limit_case(g)
        assert robust.all() and 0 < (want == 1).sum() < want.size
        rng_t, vox_t, frm_t, to_t = _dev(rng, vox, frm, to)
        forms = {"i8": torch.tensor(tri.reshape(1, -1)).to(DEV), "f32": torch.tensor(tri.reshape(1, -1).astype(f32)).to(DEV)}
        for name, t in forms.items():
            for mode in modes:
                err, got, guard_ok = _launch(t, g, rng_t, vox_t, frm_t, to_t, SC.LIMIT_RADIUS, (1, 0, 0), mode)
                assert guard_ok
                if mode == 1 and g > cap:
                    assert err == INVALID and (got == 0xA5).all()  # nothing was launched
                else:
                    assert err == 0 and np.array_equal(got, want), (g, name, mode)


# ---------------------------------------------------------------------------
# 2. BeliefFlightField.sweep and the map snapshot
# ---------------------------------------------------------------------------
def _body(**kw):
    from gennbv_amd.env.collision import CollisionBody
    return CollisionBody(sweep=True, **kw)


def test_belief_field_snapshot_and_sweep():
    from gennbv_amd import _lib
    from gennbv_amd.ops.flight_field import BeliefFlightField
    g = 12
    tri, rng, vox = SC.case(g)
    frm, to, start = SC.legs(g)
    lat = SC.lattice()
    body = _body(sweep_radius=0.2, ground=True)
    ff = BeliefFlightField(SC.N_ENVS, lat, body, torch.tensor(rng), torch.tensor(vox), g, unknown="blocked", device=DEV, shortcut=True,
                           shortcut_margin=0.03)
    assert ff.shortcut and ff.sweep_radius == 0.2 + 0.03 and ff.sweeps == 0
    assert ff.map_i8.shape == (SC.N_ENVS, g ** 3) and ff.map_i8.dtype == torch.int8
    frm_t, to_t, start_t = _dev(frm, to, start)
    with pytest.raises(_lib.GennbvHipError):  # no snapshot yet and no tri
        ff.sweep(frm_t, to_t)
    sign = np.sign(tri.reshape(SC.N_ENVS, -1).astype(np.int64))
    want, robust = SO.codes_from(SC.dist(g, False), g, rng, vox, frm, to, ff.sweep_radius, True, False, True)
    want_b, robust_b = SO.codes_from(SC.dist(g, True), g, rng, vox, start, to, ff.sweep_radius, True, False, True)
    for name, t in _forms(tri, g).items():
        ff.refresh(t)
        snap = ff.map_i8.cpu().numpy()
        if name == "i8":
            assert np.array_equal(snap, tri.reshape(SC.N_ENVS, -1))  # int8 rows are copied
        assert np.array_equal(np.sign(snap.astype(np.int64)), sign)
        t.fill_(1 if name == "i8" else 1.0)  # the caller reuses its buffer: the pilot's knowledge does not alias it
        assert np.array_equal(ff.map_i8.cpu().numpy(), snap)
        assert SO.agrees(ff.sweep(frm_t, to_t).cpu().numpy(), want, robust)
        assert SO.agrees(ff.sweep(start_t, to_t).cpu().numpy(), want_b, robust_b)  # one start per env
        out = torch.zeros(SC.N_ENVS, SC.K, dtype=torch.uint8, device=DEV)
        assert ff.sweep(start_t[:, None, :].expand(-1, SC.K, -1), to_t, out=out) is out and SO.agrees(out.cpu().numpy(), want_b, robust_b)
    assert ff.sweeps == 6 and ff.refreshes == 2
    # a tri of the caller's, another radius
    forms = _forms(tri, g)
    thin, thin_robust = SO.codes_from(SC.dist(g, False), g, rng, vox, frm, to, 0.06, True, False, True)
    for t in forms.values():
        assert SO.agrees(ff.sweep(frm_t, to_t, tri=t, radius=0.06).cpu().numpy(), thin, thin_robust)
    with pytest.raises(ValueError):
        ff.sweep(frm_t, to_t, radius=0.0)
    with pytest.raises(_lib.GennbvHipError):
        ff.sweep(frm_t.cpu(), to_t)
    with pytest.raises(_lib.GennbvHipError):
        ff.sweep(frm_t, to_t, tri=forms["i8"].to(torch.int32))
    with pytest.raises(_lib.GennbvHipError):
        ff.sweep(frm_t[:, :5], to_t)
    # without the shortcut: no snapshot, and sweep works on a tri of the caller's only
    plain = BeliefFlightField(SC.N_ENVS, lat, body, torch.tensor(rng), torch.tensor(vox), g, unknown="blocked", device=DEV)
    plain.refresh(forms["i8"])
    assert plain.shortcut is False and plain.map_i8 is None and plain.sweeps == 0
    with pytest.raises(_lib.GennbvHipError):
        plain.sweep(frm_t, to_t)
    assert SO.agrees(plain.sweep(frm_t, to_t, tri=forms["i8"], radius=0.23).cpu().numpy(), want, robust)


# ---------------------------------------------------------------------------
# 3. the env flies straight where its map shows the way in the clear, the truth judges what was flown
# ---------------------------------------------------------------------------
ENV_N, ENV_G = 4, 20


def _env_cfg():
    """The default task's volume on a coarser pose lattice (0.5 m): the stride-2 flight lattice has 17 x 17 x 11 nodes."""
    return TaskConfig(camera_width=80, camera_height=60, grid_size=ENV_G, clip_pose_idx_up=[32, 32, 20, 0, 12, 12],
                      action_unit=[0.5, 0.5, 0.5, 0.0, PI / 12.0, PI / 6.0], init_action=[16, 16, 20, 0, 12, 0])


def _belief_env(unknown, shortcut, max_len=4, seed=2, **kw):
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
    flight = BeliefFlightField(ENV_N, lat, body, scene.range_gt, scene.voxel_size, ENV_G, unknown=unknown, device=DEV, shortcut=shortcut, **kw)
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


def _judge(mesh, body, ep, prev, flown):
    """The truth's code of the flown polylines (a list of [m_e, 3] f32 arrays, one per env): one MeshScene.sweep per leg."""
    n = len(flown)
    code = torch.zeros(n, dtype=torch.uint8, device=DEV)
    for j in range(max(len(p) for p in flown) - 1):
        on = np.array([j < len(p) - 1 for p in flown])
        a = np.stack([p[j] if on[e] else prev[e] for e, p in enumerate(flown)]).astype(f32)
        b = np.stack([p[j + 1] if on[e] else prev[e] for e, p in enumerate(flown)]).astype(f32)
        a_t, b_t, on_t = _dev(a, b, on)
        code |= torch.where(on_t, mesh.sweep(a_t, b_t, body, ep), torch.zeros_like(code))
    return code


def _tri_of(obs, cfg):
    return np.sign(obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim].reshape(ENV_N, ENV_G, ENV_G, ENV_G).cpu().numpy()).astype(np.int8)


@pytest.mark.parametrize("unknown", ["free", "blocked"])
def test_env_flies_straight_to_the_farthest_waypoint_in_the_clear(unknown):
    env, cfg, scene, mesh, lat, body = _belief_env(unknown, shortcut=True)
    n, fl = ENV_N, env.flight
    rng, vox = scene.range_gt.numpy(), scene.voxel_size.numpy()
    gen = torch.Generator().manual_seed(11)
    obs = env.reset()
    assert fl.refreshes == 1 and fl.sweeps == 0 and not env.flight_length.any() and not env.skipped.any() and env.skipped.dtype == torch.int64
    saw = {"legs": 0, "weak": 0, "skipped": 0, "straight": 0, "partial": 0, "routed": 0, "first": 0, "hit": 0}
    for step in range(7):
        act = torch.stack([torch.randint(0, int(u) + 1, (n,), generator=gen) for u in cfg.clip_pose_idx_up], -1).to(DEV)
        probe = _probe(env, lat, body)
        tri_prev = _tri_of(obs, cfg)  # the map the pilot has: what the previous step wrote
        assert np.array_equal(np.sign(fl.map_i8.cpu().numpy().astype(np.int64)).reshape(tri_prev.shape), tri_prev)
        prev, ep, length_before = env.poses.clone(), env.episode_length_buf.clone() + 1, env.flight_length.clone()
        obs, _, done, _ = env.step(act)
        new = env.poses.clone()
        # --- the host re-enactment: FlightField.path, the oracle's map sweep on the previous step's tri, one MeshScene.sweep per flown leg
        way, length = probe.path(new)
        way, length = way.cpu().numpy(), length.cpu().numpy()
        prev_np, new_np, first = prev.cpu().numpy(), new.cpu().numpy(), (ep <= 1).cpu().numpy()
        kernel_codes = env._map_codes.cpu().numpy()
        flown, skipped, routed, metres, legs_flown = [], np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n), 0
        for e in range(n):
            c = max(int(length[e]) - 2, 0)
            pts = np.concatenate([prev_np[e:e + 1, :3], way[e, 1:1 + c], new_np[e:e + 1, :3]]).astype(f32)  # w_0 .. w_{c+1}
            code, robust = SO.codes(tri_prev[e:e + 1], rng[e:e + 1], vox[e:e + 1], pts[None, 0], pts[None, 1:], fl.sweep_radius,
                                    unknown == "blocked", False, False)
            got = kernel_codes[e, :c + 1]
            assert SO.agrees(got[None], code, robust), (step, e)
            code = np.where(robust[0], code[0], got)  # a non-robust leg takes the kernel's answer
            saw["legs"] += c + 1
            saw["weak"] += int((~robust).sum())
            clear = np.nonzero(code == 0)[0]
            jstar = int(clear.max()) + 1 if clear.size else 1
            flown.append(np.concatenate([pts[:1], pts[jstar:]]))
            skipped[e] = 0 if first[e] else jstar - 1
            routed[e] = jstar <= c and not first[e]
            metres[e] = sum(float(np.linalg.norm((flown[e][i + 1] - flown[e][i]).astype(np.float64))) for i in range(len(flown[e]) - 1))
            legs_flown = max(legs_flown, len(flown[e]) - 1)
            if not first[e] and c > 0:
                saw["straight"] += int(jstar == c + 1)
                saw["partial"] += int(1 < jstar <= c)
        code = _judge(mesh, body, ep, prev_np[:, :3], flown)
        assert torch.equal(env.skipped.cpu(), torch.as_tensor(skipped)), (step, env.skipped.tolist(), skipped.tolist())
        assert torch.equal(env.path_code, code), (step, env.path_code.tolist(), code.tolist())
        assert torch.equal(env.collision_buf & 24, code)  # in full: nothing is dropped
        assert torch.equal(env.collision_buf & 7, mesh.collide(new, body))
        assert torch.equal(env.routed.cpu(), torch.as_tensor(routed))
        # every leg's norm and every addition rounds once in fp32 (2^-24 relative each, a handful per leg)
        want_len = np.where(first, 0.0, length_before.cpu().numpy().astype(np.float64) + metres)
        tol = 4.0 * (legs_flown + 1) * 2.0 ** -24 * np.maximum(want_len, 1.0)
        assert (np.abs(env.flight_length.cpu().numpy() - want_len) <= tol).all(), (step, env.flight_length.tolist(), want_len.tolist())
        assert not env.flight_length[torch.as_tensor(first).to(DEV)].any() and not (code[torch.as_tensor(first).to(DEV)] != 0).any()
        assert done[env.collision_buf != 0].all()  # what the truth found ends the episode
        saw["skipped"] += int(skipped.sum())
        saw["routed"] += int(routed.sum())
        saw["first"] += int(first.sum())
        saw["hit"] += int((code != 0).sum())
    assert fl.refreshes == 8 and fl.sweeps == 7 and int(env.route_overflow) == 0  # one map sweep per step, no more
    fl.check()
    assert saw["weak"] <= 0.01 * saw["legs"]
    assert saw["first"] >= n  # an episode boundary was crossed
    if unknown == "free":
        assert saw["skipped"] >= 1 and saw["straight"] >= 1  # the optimistic pilot sees the way through what it has not seen
    print("belief env, shortcut", unknown, saw)


@pytest.mark.parametrize("unknown", ["free", "blocked"])
def test_env_without_the_shortcut_flies_the_route_as_before(unknown):
    """shortcut=False: the route's legs all go to the truth, flight_length adds the field's cost, nothing of the shortcut exists."""
    env, cfg, scene, mesh, lat, body = _belief_env(unknown, shortcut=False)
    n, fl = ENV_N, env.flight
    gen = torch.Generator().manual_seed(11)
    env.reset()
    assert env.skipped is None and fl.map_i8 is None
    for step in range(7):
        act = torch.stack([torch.randint(0, int(u) + 1, (n,), generator=gen) for u in cfg.clip_pose_idx_up], -1).to(DEV)
        probe = _probe(env, lat, body)
        prev, ep, length_before = env.poses.clone(), env.episode_length_buf.clone() + 1, env.flight_length.clone()
        env.step(act)
        new = env.poses.clone()
        way, length = probe.path(new)
        way, length = way.cpu().numpy(), length.cpu().numpy()
        prev_np, new_np = prev.cpu().numpy(), new.cpu().numpy()
        flown = [np.concatenate([prev_np[e:e + 1, :3], way[e, 1:max(int(length[e]) - 1, 1)], new_np[e:e + 1, :3]]).astype(f32) for e in range(n)]
        code = _judge(mesh, body, ep, prev_np[:, :3], flown)
        routed, first = torch.as_tensor(length > 0).to(DEV), ep <= 1
        metres = torch.where(routed, probe.cost(new[:, None])[:, 0], (new[:, :3] - prev[:, :3]).norm(dim=-1))
        assert torch.equal(env.path_code, code) and torch.equal(env.collision_buf & 24, code)
        assert torch.equal(env.flight_length, torch.where(first, torch.zeros_like(metres), length_before + metres))
        assert torch.equal(env.routed, routed & ~first)
    assert env.skipped is None and fl.sweeps == 0 and fl.refreshes == 8  # no map sweep was launched


# ---------------------------------------------------------------------------
# 4. the planner accepts what a clear straight leg reaches
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


def test_map_greedy_accepts_a_clear_straight_leg():
    from gennbv_amd.eval.baselines import MapGreedyPolicy
    env, cfg, scene, mesh, lat, body = _belief_env("free", shortcut=True, max_len=30)
    n, fl = ENV_N, env.flight
    rng, vox = scene.range_gt.numpy(), scene.voxel_size.numpy()
    obs = env.reset()
    # a map of the planner's own: free everywhere but an occupied slab, x voxels 12 .. 14, every y, z voxels 0 .. 9.  `near` lies a
    # metre in front of the slab: its lattice node is blocked under the inflated rho (0.97 m), so no route ends there, but the
    # straight leg from the start (0, 0, 10.1) stays clear of the slab by far more than the body's 0.10 m
    tri = torch.full((n, ENV_G, ENV_G, ENV_G), -1, dtype=torch.int8, device=DEV)
    tri[:, 12:15, :, :10] = 1
    fl.refresh(tri.reshape(n, -1)).update(env.poses)
    inside, near, free_far = [22, 16, 4, 0, 6, 0], [18, 16, 4, 0, 6, 0], [30, 16, 10, 0, 6, 0]  # (3, 0, 2.1), (1, 0, 2.1), (7, 0, 5.1)
    gains = torch.tensor([[300, 0, 0], [200, 0, 0], [100, 0, 0]], dtype=torch.int32, device=DEV)
    backend = lambda t, p: gains[None].expand(n, -1, -1)  # noqa: E731
    real = env.collision_mesh
    env.collision_mesh = _NoMesh()
    try:
        pol = MapGreedyPolicy(env, k=3, weights=(1, 0), gain_backend=backend)
        assert pol.shortcut  # None follows the field
        pol.cands = _Fixed(cfg, [inside, near, free_far])
        before = fl.sweeps
        act = pol(obs)[0]
        assert fl.sweeps == before + 1
        reach = fl.reachable(pol.cands.poses(pol.cands.sample(n, DEV)))
        assert reach.tolist() == [[False, False, True]] * n
        assert act.tolist() == [near] * n and pol._contact.tolist() == [[1, 0, 0]] * n
        off = MapGreedyPolicy(env, k=3, weights=(1, 0), gain_backend=backend, shortcut=False)
        off.cands = pol.cands
        before = fl.sweeps
        assert off(obs)[0].tolist() == [free_far] * n and off._contact.tolist() == [[1, 1, 0]] * n  # the same candidate, refused
        assert fl.sweeps == before  # the launches of today
        # random candidates, the real gain kernel: contact = ~reachable & (the oracle's sweep != 0) on robust candidates
        pol = MapGreedyPolicy(env, k=16, seed=5, shortcut=True)
        tri_np = tri.cpu().numpy()
        accepted_by_leg = 0
        for _ in range(3):
            pol(obs)
            poses = pol.cands.poses(pol.cands.sample(n, DEV))  # (the sampler has moved on: judge the contact of these instead)
            contact = pol.contact(poses).cpu().numpy()
            reach = fl.reachable(poses).cpu().numpy()
            code, robust = SO.codes(tri_np, rng, vox, env.poses.cpu().numpy(), poses.cpu().numpy(), fl.sweep_radius, False, False, False)
            assert robust.mean() >= 0.99
            assert np.array_equal(contact[robust] != 0, (~reach & (code != 0))[robust])
            accepted_by_leg += int((~reach & (contact == 0)).sum())
        assert accepted_by_leg >= 1
    finally:
        env.collision_mesh = real

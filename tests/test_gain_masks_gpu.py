"""GPU: gnbv_view_gain_masks (csrc/viewgain.hip) against the CPU oracle (tests/gain_masks_oracle.py) with == on every word of both
masks, into buffers pre-filled with 0xFF bytes; output selection, chunking and grid forms; the refusals at the raw binding; the
operator's set-cover plan against the numpy greedy on the oracle's masks; and MapCoverPolicy on a real closed-loop env.  The
mechanism is asserted, not planning quality."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import PI, TaskConfig
from tests import cover_greedy_oracle as CO
from tests import gain_masks_oracle as MO
from tests.test_view_gain_gpu import _lattice_poses, _outside_poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = 1  # hipErrorInvalidValue


def _cfg(h, w, g):
    return TaskConfig(camera_width=w, camera_height=h, grid_size=g)


def _kinv(cfg):
    return S.inverse_intrinsics(cfg.camera_height, cfg.camera_width, cfg.horizontal_fov).numpy()


def _op(cfg, scene, n, k, stride, range_m, chunk=0, **kw):
    from gennbv_amd.ops.gain_masks import ViewGainMasks
    op = ViewGainMasks(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, range_m=range_m, device=DEV, with_c2w=True, chunk=chunk, **kw)
    for buf in (op.unknown_bits, op.hit_bits):
        if buf is not None:
            buf.view(torch.uint8).fill_(0xFF)
    op.gain.fill_(-12345)
    return op


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _pad(m, words):
    out = np.zeros(m.shape[:-1] + (words,), np.uint32)
    out[..., :m.shape[-1]] = m
    return out


CASES = [  # g, (h, w), stride, range, n, k, chunk, occupied density (None: all unknown), poses
    (16, (60, 80), 4, 50.0, 37, 3, 2, 0.10, "lattice"),
    (20, (60, 80), 1, 50.0, 1, 5, 2, 0.01, "lattice"),
    (20, (240, 320), 4, 50.0, 1, 7, 3, 0.05, "outside"),
    (33, (60, 80), 4, 2.0, 1, 5, 0, 0.10, "lattice"),  # 33^3 is not a multiple of 32: the last word is partial
    (64, (60, 80), 4, 2.0, 3, 3, 2, 0.05, "lattice"),
    (20, (60, 80), 4, 50.0, 2, 5, 0, None, "lattice"),
    # a lattice of exactly one wave (64 rays), and one of 4 800 rays: no whole number of waves, more than one turn of 1 024 lanes
    (20, (8, 8), 1, 50.0, 1, 5, 2, 0.05, "lattice"),
    (20, (60, 80), 1, 50.0, 1, 5, 2, 0.05, "lattice"),
]


@pytest.mark.parametrize("g,cam,stride,range_m,n,k,chunk,occ,kind", CASES)
def test_masks_equal_the_oracle_on_every_word(g, cam, stride, range_m, n, k, chunk, occ, kind):
    from gennbv_amd import _lib
    from gennbv_amd.ops.view_gain import ViewGain
    cfg = _cfg(cam[0], cam[1], g)
    scene = S.make_scenes(n, g, seed=2)
    tri = MO.random_tri(n, g, occ, seed=g + n)
    poses = (_lattice_poses(cfg, n, k, seed=g) if kind == "lattice" else _outside_poses(n, k)).to(DEV)
    tri_d = tri.to(DEV)
    plain = ViewGain(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, range_m=range_m, device=DEV, chunk=chunk)(tri_d, poses).cpu()
    want = None
    sizes = (MO.min_words(g), int(_lib.load().gnbv_grid_bit_words(g)))
    assert sizes[0] <= sizes[1] and sizes[0] % 4 == 0 and sizes[0] * 32 >= g ** 3 > (sizes[0] - 4) * 32
    for words in sizes:
        op = _op(cfg, scene, n, k, stride, range_m, chunk, words=words)
        gain = op(tri_d, poses).cpu()
        if want is None:  # the camera comes from the kernel (c2w_out), as in the view-gain tests; once per case
            want = MO.masks(tri.numpy(), op.c2w.cpu().numpy(), scene.range_gt.numpy(), scene.voxel_size.numpy(), _kinv(cfg), cam[0], cam[1],
                            stride, range_m, words=sizes[0])
        ub, hb = _u32(op.unknown_bits), _u32(op.hit_bits)
        assert ub.shape == hb.shape == (n, k, words)
        print("words", words, "popcount U", int(CO.popcount(ub).sum()), "H", int(CO.popcount(hb).sum()))
        assert np.array_equal(ub, _pad(want[0], words)), np.argwhere(ub != _pad(want[0], words))[:5].tolist()
        assert np.array_equal(hb, _pad(want[1], words)), np.argwhere(hb != _pad(want[1], words))[:5].tolist()
        assert torch.equal(gain, plain)  # byte-equal to gnbv_view_gain on the same inputs
        assert np.array_equal(CO.popcount(ub), gain[..., 0].numpy()) and np.array_equal(CO.popcount(hb), gain[..., 1].numpy())
    assert CO.popcount(want[0]).sum() > 0 and (occ is None or CO.popcount(want[1]).sum() > 0)


def test_output_selection_chunks_overwrite_and_grid_forms():
    g, n, k = 20, 5, 7
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=4)
    tri = MO.random_tri(n, g, 0.03, seed=1).to(DEV)
    poses = _lattice_poses(cfg, n, k, seed=5).to(DEV)
    other = _lattice_poses(cfg, n, k, seed=6).to(DEV)
    both = _op(cfg, scene, n, k, 4, 50.0, chunk=3)
    gain = both(tri, poses).clone()
    ub, hb = both.unknown_bits.clone(), both.hit_bits.clone()
    assert int(gain[..., 1].sum()) > 0 and not bool((gain == -12345).any())
    # one output only: the same rows
    only_u = _op(cfg, scene, n, k, 4, 50.0, chunk=3, hit=False)
    only_h = _op(cfg, scene, n, k, 4, 50.0, chunk=3, unknown=False)
    assert torch.equal(only_u(tri, poses), gain) and torch.equal(only_u.unknown_bits, ub) and only_u.hit_bits is None
    assert torch.equal(only_h(tri, poses), gain) and torch.equal(only_h.hit_bits, hb) and only_h.unknown_bits is None
    # chunking
    for chunk in (1, k):
        op = _op(cfg, scene, n, k, 4, 50.0, chunk=chunk)
        assert torch.equal(op(tri, poses), gain) and torch.equal(op.unknown_bits, ub) and torch.equal(op.hit_bits, hb)
    # a second call on other poses overwrites every word: equal to a fresh operator's
    both(tri, other)
    fresh = _op(cfg, scene, n, k, 4, 50.0, chunk=3)
    fresh(tri, other)
    assert torch.equal(both.unknown_bits, fresh.unknown_bits) and torch.equal(both.hit_bits, fresh.hit_bits)
    assert not torch.equal(both.unknown_bits, ub)
    # tri as a strided int8 row slice (unaligned row stride) and as the fp32 slice of a flat observation
    big = torch.full((n, g ** 3 + 13), 1, dtype=torch.int8, device=DEV)
    big[:, 5:5 + g ** 3] = tri
    obs = torch.full((n, 7 + g ** 3 + 3), 5.0, dtype=torch.float32, device=DEV)
    obs[:, 7:7 + g ** 3] = tri.float()
    for form in (big[:, 5:5 + g ** 3], obs[:, 7:7 + g ** 3], tri.view(n, g, g, g)):
        op = _op(cfg, scene, n, k, 4, 50.0, chunk=3)
        assert torch.equal(op(form, poses), gain) and torch.equal(op.unknown_bits, ub) and torch.equal(op.hit_bits, hb)


def test_refusals_at_the_raw_binding_and_the_operator():
    from gennbv_amd import _lib
    from gennbv_amd.ops.gain_masks import ViewGainMasks
    g, n, k = 20, 2, 4
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=1)
    op = _op(cfg, scene, n, k, 4, 50.0)
    tri, poses = torch.zeros(n, g ** 3, dtype=torch.int8, device=DEV), torch.zeros(n, k, 6, device=DEV)
    op(tri, poses)
    lib = _lib.load()
    ub, hb, words = op.unknown_bits.data_ptr(), op.hit_bits.data_ptr(), op.words

    def call(words=words, ub=ub, hb=hb, **kw):
        a = _lib.GnbvViewGain()
        C.memmove(C.byref(a), C.byref(op._args), C.sizeof(a))
        for f, v in kw.items():
            setattr(a, f, v)
        return lib.gnbv_view_gain_masks(C.byref(a), words, ub, hb, None)
    assert call() == 0 and call(ub=None) == 0 and call(hb=None) == 0 and call(words=MO.min_words(g)) == 0
    for kw in (dict(stride=0), dict(range=0.0), dict(range=float("inf")), dict(k=0), dict(g=128), dict(g=65), dict(g=1), dict(gain=None)):
        assert call(**kw) == INVALID, kw
    assert call(ub=None, hb=None) == INVALID
    for w in (0, 248, 250, 251, 253):
        assert call(words=w) == INVALID, w
    for bad in (dict(ub=ub + 4), dict(hb=hb + 8), dict(ub=ub + 1, hb=None)):
        assert call(**bad) == INVALID, bad
    assert call(n=65536, k=4096, g=2, tri_row_stride=8, words=8) == INVALID  # n k words = 2^31
    for ablate in (1, 2, 3):
        assert call(ablate=ablate) == INVALID
    torch.cuda.synchronize()
    with pytest.raises(_lib.GennbvHipError, match="slab"):
        ViewGainMasks(n, k, _cfg(60, 80, 65), scene.range_gt, scene.voxel_size, device=DEV)
    with pytest.raises(_lib.GennbvHipError, match="above max_bytes"):
        ViewGainMasks(n, k, cfg, scene.range_gt, scene.voxel_size, device=DEV, max_bytes=2 * n * k * op.words * 4 - 1)
    ViewGainMasks(n, k, cfg, scene.range_gt, scene.voxel_size, device=DEV, max_bytes=2 * n * k * op.words * 4)
    with pytest.raises(_lib.GennbvHipError):
        op.plan(0)
    with pytest.raises(_lib.GennbvHipError):
        op.plan(2, which="both")
    with pytest.raises(_lib.GennbvHipError):
        op.plan(2, contact=torch.zeros(n, k, dtype=torch.uint8))


@functools.lru_cache(maxsize=None)
def _plan_case():
    """5 envs x 7 candidates at 20^3: the operator after one call, and the oracle's masks of the same cameras (computed once)."""
    g, n, k = 20, 5, 7
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=4)
    tri = MO.random_tri(n, g, 0.05, seed=3)
    poses = _lattice_poses(cfg, n, k, seed=8, extremes=False).to(DEV)
    op = _op(cfg, scene, n, k, 4, 50.0)
    gain = op(tri.to(DEV), poses).clone()
    want = MO.masks(tri.numpy(), op.c2w.cpu().numpy(), scene.range_gt.numpy(), scene.voxel_size.numpy(), _kinv(cfg), 60, 80, 4, 50.0,
                    words=op.words)
    gen = torch.Generator().manual_seed(11)
    contact = (torch.rand(n, k, generator=gen) < 0.4).to(torch.uint8)
    contact[0] = 1  # an env whose candidates are all refused: candidate 0
    return op, gain, want, contact


@pytest.mark.parametrize("with_contact", [False, True])
@pytest.mark.parametrize("rounds", [1, 4])
def test_plan_equals_the_exhaustive_greedy_on_the_oracle_masks(rounds, with_contact):
    from gennbv_amd.eval.baselines import choose
    op, gain, want, contact = _plan_case()
    n, k = gain.shape[:2]
    con = contact if with_contact else torch.zeros_like(contact)
    con_d = con.to(DEV) if with_contact else None
    for which, masks, w in (("unknown", want[0], (1, 0)), ("hit", want[1], (0, 1))):
        for lazy in (True, False):
            choice, g, covered = op.plan(rounds, which=which, contact=con_d, lazy=lazy)
            ref = CO.batch_exhaustive(masks, np.zeros((n, op.words), np.uint32), con.numpy(), rounds)
            assert np.array_equal(choice.cpu().numpy(), ref[0]) and np.array_equal(g.cpu().numpy(), ref[1]), (which, lazy)
            assert np.array_equal(_u32(covered), ref[2]) and np.array_equal(op.gains0.cpu().numpy(), ref[3])
            assert op.plan(rounds, which=which, contact=con_d)[0] is choice  # cached per `rounds`
        if rounds == 1:
            assert torch.equal(choice[:, 0].long(), choose(gain, w, con_d))
        else:
            assert any(ref[1][e, t] < ref[3][e, ref[0][e, t]] for e in range(n) for t in range(1, rounds))  # overlap seen


def test_call_and_plan_do_not_synchronise():
    op, gain, _, contact = _plan_case()
    g = 20
    tri = MO.random_tri(5, g, 0.05, seed=3).to(DEV)
    poses = _lattice_poses(_cfg(60, 80, g), 5, 7, seed=8, extremes=False).to(DEV)
    con = contact.to(DEV)
    op.plan(3, which="hit", contact=con)  # (warm-up: the first use allocates the plan's outputs)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = op(tri, poses)
        plan = op.plan(3, which="hit", contact=con)
        plan_u = op.plan(3, which="unknown")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out, gain) and plan[0].shape == (5, 3) and plan_u[0] is plan[0]


# ---------------------------------------------------------------------------
# MapCoverPolicy on a real closed-loop env
# ---------------------------------------------------------------------------
ENV_N, ENV_G, EP_LEN = 8, 20, 20


def _env(seed=2):
    """The construction of tests/test_frontview_gpu.py: the default task's volume on a 0.5 m pose lattice, a swept body, a belief
    flight field with unknown space free, on a lattice of stride 2."""
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.flight import FlightLattice
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.ops.flight_field import BeliefFlightField
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=ENV_G, clip_pose_idx_up=[32, 32, 20, 0, 12, 12],
                     action_unit=[0.5, 0.5, 0.5, 0.0, PI / 12.0, PI / 6.0], init_action=[16, 16, 20, 0, 12, 0])
    scene = S.make_scenes(ENV_N, ENV_G, seed=seed)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = CollisionBody(sweep=True)
    flight = BeliefFlightField(ENV_N, FlightLattice(cfg, stride=2), body, scene.range_gt, scene.voxel_size, ENV_G, unknown="free", device=DEV)
    return ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=EP_LEN, collision=body, flight=flight), cfg


def test_horizon_one_flies_what_map_greedy_flies():
    from gennbv_amd.eval.baselines import MapCoverPolicy, MapGreedyPolicy
    env_a, cfg = _env()
    env_b, _ = _env()
    pa = MapCoverPolicy(env_a, k=8, horizon=1, mask="unknown", seed=7, stride=4)
    pb = MapGreedyPolicy(env_b, k=8, weights=(1, 0), seed=7, stride=4)
    oa, ob = env_a.reset(), env_b.reset()
    for step in range(EP_LEN + 2):  # a whole episode and its restart
        a, b = pa(oa)[0], pb(ob)[0]
        assert torch.equal(a, b), step
        assert torch.equal(pa.last_gain3, pb.last_gain) and bool(pa.adopted.all()) and bool((pa.last_length_mm == -1).all())
        oa, ob = env_a.step(a)[0], env_b.step(b)[0]
        assert torch.equal(oa, ob)


def test_committed_plans_are_flown_in_order_and_replaced_on_reset():
    """horizon = commit = 3: a host mirror of the stored plans, fed only with what the policy exposes at each decision."""
    from gennbv_amd.eval.baselines import MapCoverPolicy
    env, cfg = _env()
    pol = MapCoverPolicy(env, k=8, horizon=3, commit=3, mask="hit", seed=5)
    obs = env.reset()
    plan, views, cursor = [None] * ENV_N, [0] * ENV_N, [0] * ENV_N
    multi = resets_mid_plan = 0
    for step in range(2 * EP_LEN + 5):
        ep_len = env.episode_length_buf.cpu().tolist()
        act = pol(obs)[0]
        adopted, new_plan, new_views = pol.adopted.cpu().tolist(), pol.last_actions.cpu(), pol.last_views.cpu().tolist()
        choice, gain = pol.last_choice.cpu(), pol.last_gain.cpu()
        assert choice.shape == gain.shape == (ENV_N, 3) and pol.last_gain3.shape == (ENV_N, 8, 3)
        for e in range(ENV_N):
            restart = ep_len[e] <= 1
            mid = 0 < cursor[e] < min(3, views[e])
            assert adopted[e] == (restart or cursor[e] >= min(3, views[e])), (step, e)
            if restart and mid:
                resets_mid_plan += 1  # the rest of the old plan is dropped: the action below comes from a plan made after the reset
            if adopted[e]:
                plan[e], views[e], cursor[e] = new_plan[e], new_views[e], 0
                assert 0 <= views[e] <= int((gain[e] > 0).sum())
                multi += views[e] > 1
            assert torch.equal(act[e].cpu(), plan[e][cursor[e]]), (step, e, cursor[e])
            cursor[e] += 1
        assert pol.cursor.cpu().tolist() == cursor and pol.plan_views.cpu().tolist() == views
        obs = env.step(act)[0]
    print("plans with more than one view", multi, "resets in mid-plan", resets_mid_plan)
    assert multi > 0 and resets_mid_plan > 0


def test_routed_plan_length_is_the_sum_of_its_legs():
    from gennbv_amd.eval.baselines import MapCoverPolicy
    env, cfg = _env()
    t_max = 4
    pol = MapCoverPolicy(env, k=8, horizon=t_max, commit=t_max, mask="unknown", route=True, seed=9)
    obs = env.reset()
    routed_views = 0
    for step in range(6):
        start = env.poses[:, :3].clone()
        act = pol(obs)[0]
        views, acts = pol.last_views, pol.last_actions
        pts = torch.cat([start[:, None], S.poses_from_actions(acts, cfg).float()[..., :3]], dim=1).contiguous()
        dist = env.flight.pairwise_mm(pts, (views + 1).to(torch.int32)).long() & 0xFFFFFFFF
        legs = dist[:, torch.arange(t_max), torch.arange(1, t_max + 1)]  # leg i: point i -> point i + 1 of the flown order
        flown = torch.arange(t_max, device=DEV)[None] < views[:, None]
        assert not bool((flown & (legs == 0xFFFFFFFF)).any())
        assert torch.equal(pol.last_length_mm, torch.where(flown, legs, torch.zeros_like(legs)).sum(dim=1)), step
        routed_views += int(views.sum())
        obs = env.step(act)[0]
    assert routed_views > 0

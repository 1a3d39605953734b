"""GPU: gnbv_view_gain_slab_masks (csrc/viewgain.hip, k_vg_prep<true> / k_vg_slab<true>) against the CPU oracle
(tests/gain_masks_oracle.py) with == on every word of both masks, into buffers pre-filled with 0xFF bytes, at grids from 65^3 to
128^3, both row lengths, default and ragged slab heights; against gnbv_view_gain_masks on the grids both answer, at slab heights
that put seams everywhere; env batches over one workspace; output selection, overwrite, grid forms and the call without rays; the
refusals at the raw binding; the factory; the set-cover plans on slab masks; and MapCoverPolicy on a closed-loop env above 64^3.
Every comparison is == on integers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import PI, TaskConfig
from tests import cover_greedy_oracle as CO
from tests import cover_weighted_oracle as CW
from tests import gain_masks_oracle as MO
from tests.test_view_gain_gpu import _lattice_poses, _outside_poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = 1  # hipErrorInvalidValue


def _cfg(h, w, g):
    return TaskConfig(camera_width=w, camera_height=h, grid_size=g)


def _kinv(cfg):
    return S.inverse_intrinsics(cfg.camera_height, cfg.camera_width, cfg.horizontal_fov).numpy()


def _fill(op):
    for buf in (op.unknown_bits, op.hit_bits):
        if buf is not None:
            buf.view(torch.uint8).fill_(0xFF)
    op.gain.fill_(-12345)
    return op


def _op(cfg, scene, n, k, stride, range_m, chunk=0, slab=0, **kw):
    from gennbv_amd.ops.gain_masks import ViewGainMasksSlab
    return _fill(ViewGainMasksSlab(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, range_m=range_m, device=DEV, with_c2w=True,
                                   chunk=chunk, slab=slab, **kw))


def _lds_op(cfg, scene, n, k, stride, range_m, **kw):
    from gennbv_amd.ops.gain_masks import ViewGainMasks
    return _fill(ViewGainMasks(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, range_m=range_m, device=DEV, **kw))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _pad(m, words):
    out = np.zeros(m.shape[:-1] + (words,), np.uint32)
    out[..., :m.shape[-1]] = m
    return out


CASES = [  # g, (h, w), stride, range, n, k, slab heights, occupied density (None: all unknown), poses
    (65, (60, 80), 4, 50.0, 2, 5, (0, 24), 0.05, "lattice"),      # G^2 % 32 = 1: every seam is unaligned
    (72, (60, 80), 4, 50.0, 3, 4, (0, 5), 0.05, "lattice"),       # aligned G^2, ragged slabs
    (100, (60, 80), 4, 50.0, 2, 4, (0, 7), None, "lattice"),      # G^2 % 32 = 16, all unknown
    (127, (60, 80), 4, 50.0, 1, 3, (0, 5), 0.02, "lattice"),      # odd, with a partial last word
    (128, (240, 320), 4, 50.0, 1, 5, (0, 24), 0.01, "lattice"),   # (24 planes exceed the LDS: reduced to 19)
    (128, (60, 80), 4, 50.0, 1, 3, (0, 5), 0.02, "outside"),      # sources outside the grid
    (72, (60, 80), 4, 3000.0, 2, 4, (0, 5), 0.02, "lattice"),     # the 64-bit rays
]


@pytest.mark.parametrize("g,cam,stride,range_m,n,k,slabs,occ,kind", CASES)
def test_masks_equal_the_oracle_on_every_word(g, cam, stride, range_m, n, k, slabs, occ, kind):
    from gennbv_amd import _lib
    from gennbv_amd.ops.view_gain import ViewGainSlab
    cfg = _cfg(cam[0], cam[1], g)
    scene = S.make_scenes(n, g, seed=2)
    tri = MO.random_tri(n, g, occ, seed=g + n)
    poses = (_lattice_poses(cfg, n, k, seed=g) if kind == "lattice" else _outside_poses(n, k)).to(DEV)
    tri_d = tri.to(DEV)
    plain = ViewGainSlab(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, range_m=range_m, device=DEV)(tri_d, poses).cpu()
    want = None
    sizes = (MO.min_words(g), int(_lib.load().gnbv_grid_bit_words(g)))
    assert sizes[0] <= sizes[1] and sizes[0] % 4 == 0 and sizes[0] * 32 >= g ** 3 > (sizes[0] - 4) * 32
    for words in sizes:
        for slab in slabs:
            for chunk in (0, 2):
                op = _op(cfg, scene, n, k, stride, range_m, chunk, slab, words=words)
                gain = op(tri_d, poses).cpu()
                if want is None:  # the camera comes from the kernel (c2w_out), as in the view-gain tests; once per case
                    want = MO.masks(tri.numpy(), op.c2w.cpu().numpy(), scene.range_gt.numpy(), scene.voxel_size.numpy(), _kinv(cfg), cam[0],
                                    cam[1], stride, range_m, words=sizes[0])
                    print("popcount U", int(CO.popcount(want[0]).sum()), "H", int(CO.popcount(want[1]).sum()))
                ub, hb = _u32(op.unknown_bits), _u32(op.hit_bits)
                assert ub.shape == hb.shape == (n, k, words)
                tag = (words, slab, chunk)
                assert np.array_equal(ub, _pad(want[0], words)), (tag, np.argwhere(ub != _pad(want[0], words))[:5].tolist())
                assert np.array_equal(hb, _pad(want[1], words)), (tag, np.argwhere(hb != _pad(want[1], words))[:5].tolist())
                assert torch.equal(gain, plain), tag  # byte-equal to gnbv_view_gain_slab on the same inputs
                assert np.array_equal(CO.popcount(ub), gain[..., 0].numpy()) and np.array_equal(CO.popcount(hb), gain[..., 1].numpy()), tag
    assert CO.popcount(want[0]).sum() > 0 and (occ is None or CO.popcount(want[1]).sum() > 0)


@pytest.mark.parametrize("g,n,k", [(20, 37, 3), (33, 2, 3), (64, 2, 3)])
def test_seams_inside_grids_the_lds_kernel_answers(g, n, k):
    """Slab heights 1, 3, 7, 16 and g against gnbv_view_gain_masks; 37 envs: the 8-env XCD padding and a partial last group."""
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=3)
    tri = MO.random_tri(n, g, 0.03, seed=g).to(DEV)
    poses = _lattice_poses(cfg, n, k, seed=g + 1).to(DEV)
    ref = _lds_op(cfg, scene, n, k, 4, 50.0)
    gain = ref(tri, poses)
    assert int(gain[..., 0].sum()) > 0 and int(gain[..., 1].sum()) > 0
    for slab in (1, 3, 7, 16, g):
        op = _op(cfg, scene, n, k, 4, 50.0, slab=slab)
        assert torch.equal(op(tri, poses), gain), slab
        assert torch.equal(op.unknown_bits, ref.unknown_bits) and torch.equal(op.hit_bits, ref.hit_bits), slab


def test_env_batches_write_the_rows_of_the_global_env():
    """tests/test_view_gain_slab_gpu.py's batch shape: 24 envs x 8 candidates x 76 800 rays run in three batches over one workspace."""
    g, n, k = 20, 24, 8
    cfg = _cfg(240, 320, g)
    scene = S.make_scenes(n, g, seed=5)
    tri = MO.random_tri(n, g, 0.03, seed=9).to(DEV)
    poses = _lattice_poses(cfg, n, k, seed=4).to(DEV)
    ref = _lds_op(cfg, scene, n, k, 1, 50.0)
    gain = ref(tri, poses)
    op = _op(cfg, scene, n, k, 1, 50.0, slab=7)
    assert op.workspace_bytes < n * k * 76800 * 20  # the workspace does not hold all envs: several batches
    assert torch.equal(op(tri, poses), gain)
    assert torch.equal(op.unknown_bits, ref.unknown_bits) and torch.equal(op.hit_bits, ref.hit_bits)
    assert len({bytes(r) for r in _u32(op.unknown_bits)[:, 0]}) == n  # (the envs' rows differ: a batch-local row index would show)


def test_overwrite_output_selection_grid_forms_and_the_call_without_rays():
    g, n, k = 72, 5, 7
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=4)
    tri = MO.random_tri(n, g, 0.03, seed=1).to(DEV)
    poses = _lattice_poses(cfg, n, k, seed=5).to(DEV)
    other = _lattice_poses(cfg, n, k, seed=6).to(DEV)
    both = _op(cfg, scene, n, k, 4, 50.0, chunk=3, slab=5)
    gain = both(tri, poses).clone()
    ub, hb = both.unknown_bits.clone(), both.hit_bits.clone()
    assert int(gain[..., 1].sum()) > 0 and not bool((gain == -12345).any())
    # one output only: the same rows
    only_u = _op(cfg, scene, n, k, 4, 50.0, chunk=3, slab=5, hit=False)
    only_h = _op(cfg, scene, n, k, 4, 50.0, chunk=3, slab=5, unknown=False)
    assert torch.equal(only_u(tri, poses), gain) and torch.equal(only_u.unknown_bits, ub) and only_u.hit_bits is None
    assert torch.equal(only_h(tri, poses), gain) and torch.equal(only_h.hit_bits, hb) and only_h.unknown_bits is None
    # a second call on other poses overwrites every word: equal to a fresh operator's
    both(tri, other)
    fresh = _op(cfg, scene, n, k, 4, 50.0, chunk=3, slab=5)
    fresh(tri, other)
    assert torch.equal(both.unknown_bits, fresh.unknown_bits) and torch.equal(both.hit_bits, fresh.hit_bits)
    assert not torch.equal(both.unknown_bits, ub)
    # tri as a strided int8 row slice (unaligned row stride), as the fp32 slice of a flat observation and as [N,G,G,G]
    big = torch.full((n, g ** 3 + 13), 1, dtype=torch.int8, device=DEV)
    big[:, 5:5 + g ** 3] = tri
    obs = torch.full((n, 7 + g ** 3 + 3), 5.0, dtype=torch.float32, device=DEV)
    obs[:, 7:7 + g ** 3] = tri.float()
    for form in (big[:, 5:5 + g ** 3], obs[:, 7:7 + g ** 3], tri.view(n, g, g, g)):
        op = _op(cfg, scene, n, k, 4, 50.0, chunk=3, slab=5)
        assert torch.equal(op(form, poses), gain) and torch.equal(op.unknown_bits, ub) and torch.equal(op.hit_bits, hb)
    # no ray at all (stride / 2 >= width): every word of every row is still written, and gain is zero
    for kw in (dict(), dict(hit=False), dict(unknown=False)):
        none = _op(cfg, scene, n, k, 700, 50.0, slab=5, **kw)
        assert int(none(tri, poses).abs().sum()) == 0
        for buf in (none.unknown_bits, none.hit_bits):
            assert buf is None or (buf.shape == (n, k, none.words) and int((buf != 0).sum()) == 0)


def test_refusals_at_the_raw_binding_and_accepted_selections():
    from gennbv_amd import _lib
    g, n, k = 72, 2, 4
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=1)
    op = _op(cfg, scene, n, k, 4, 50.0)
    tri, poses = torch.zeros(n, g ** 3, dtype=torch.int8, device=DEV), torch.zeros(n, k, 6, device=DEV)
    op(tri, poses)
    lib = _lib.load()
    ub, hb, words, ws, ws_bytes = op.unknown_bits.data_ptr(), op.hit_bits.data_ptr(), op.words, op.workspace.data_ptr(), op.workspace_bytes

    def call(slab=0, ws=ws, ws_bytes=ws_bytes, words=words, ub=ub, hb=hb, **kw):
        a = _lib.GnbvViewGain()
        C.memmove(C.byref(a), C.byref(op._args), C.sizeof(a))
        for f, v in kw.items():
            setattr(a, f, v)
        return lib.gnbv_view_gain_slab_masks(C.byref(a), slab, ws, ws_bytes, words, ub, hb, None)
    assert words > MO.min_words(g)
    assert call() == 0 and call(ub=None) == 0 and call(hb=None) == 0 and call(words=MO.min_words(g)) == 0 and call(slab=5) == 0
    for kw in (dict(stride=0), dict(range=0.0), dict(range=float("inf")), dict(k=0), dict(g=129), dict(g=1), dict(gain=None), dict(slab=-1),
               dict(ws=None), dict(ws_bytes=ws_bytes - 256), dict(ws=ws + 8)):
        assert call(**kw) == INVALID, kw
    assert call(ub=None, hb=None) == INVALID
    for w in (0, -4, MO.min_words(g) - 4, MO.min_words(g) + 1, MO.min_words(g) + 2):
        assert call(words=w) == INVALID, w
    for bad in (dict(ub=ub + 4), dict(hb=hb + 8), dict(ub=ub + 1, hb=None)):
        assert call(**bad) == INVALID, bad
    assert call(n=65536, k=4096, g=2, tri_row_stride=8, words=8, ws_bytes=1 << 40) == INVALID  # n k words = 2^31
    for ablate in (1, 2, 3):
        assert call(ablate=ablate) == INVALID
    torch.cuda.synchronize()


def test_the_factory_picks_by_grid_size():
    from gennbv_amd.ops.gain_masks import ViewGainMasks, ViewGainMasksSlab, make_view_gain_masks
    for g, cls in ((20, ViewGainMasks), (64, ViewGainMasks), (65, ViewGainMasksSlab), (128, ViewGainMasksSlab)):
        scene = S.make_scenes(1, g, seed=1)
        op = make_view_gain_masks(1, 2, _cfg(60, 80, g), scene.range_gt, scene.voxel_size, device=DEV, slab=3, hit=(g != 128))
        assert type(op) is cls and op.g == g and (cls is ViewGainMasks or op.slab == 3)
        assert (op.hit_bits is None) == (g == 128) and op.unknown_bits.shape == (1, 2, op.words)


@functools.lru_cache(maxsize=None)
def _plan_case():
    """2 envs x 8 candidates at 72^3: the slab operator after one call, and the oracle's masks of the same cameras (computed once)."""
    g, n, k = 72, 2, 8
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=4)
    tri = MO.random_tri(n, g, 0.02, seed=3)
    poses = _lattice_poses(cfg, n, k, seed=8, extremes=False).to(DEV)
    op = _op(cfg, scene, n, k, 4, 50.0, slab=5)
    gain = op(tri.to(DEV), poses).clone()
    want = MO.masks(tri.numpy(), op.c2w.cpu().numpy(), scene.range_gt.numpy(), scene.voxel_size.numpy(), _kinv(cfg), 60, 80, 4, 50.0,
                    words=op.words)
    contact = torch.tensor([[1] * k, [0, 1, 0, 0, 1, 0, 1, 0]], dtype=torch.uint8)  # env 0: all refused -> candidate 0
    return op, gain, want, contact


@pytest.mark.parametrize("with_contact", [False, True])
@pytest.mark.parametrize("rounds", [1, 4])
def test_plans_on_slab_masks_equal_the_numpy_greedy_on_the_oracle_masks(rounds, with_contact):
    op, gain, want, contact = _plan_case()
    n, k = gain.shape[:2]
    assert np.array_equal(_u32(op.unknown_bits), want[0]) and np.array_equal(_u32(op.hit_bits), want[1])
    assert CO.popcount(want[0]).sum() > 0 and CO.popcount(want[1]).sum() > 0
    con = contact if with_contact else torch.zeros_like(contact)
    con_d = con.to(DEV) if with_contact else None
    zero = np.zeros((n, op.words), np.uint32)
    for which, masks in (("unknown", want[0]), ("hit", want[1])):
        choice, g, covered = op.plan(rounds, which=which, contact=con_d)
        ref = CO.batch_exhaustive(masks, zero, con.numpy(), rounds)
        assert np.array_equal(choice.cpu().numpy(), ref[0]) and np.array_equal(g.cpu().numpy(), ref[1]), which
        assert np.array_equal(_u32(covered), ref[2]) and np.array_equal(op.gains0.cpu().numpy(), ref[3])
    for w in ((1, 4), (4, 1)):
        choice, g, covered = op.plan_weighted(rounds, weights=w, contact=con_d)
        ref = CW.batch_exhaustive(list(want), [zero, zero], list(w), con.numpy(), rounds)
        assert np.array_equal(choice.cpu().numpy(), ref[0]) and np.array_equal(g.cpu().numpy(), ref[1]), w
        assert np.array_equal(op.plane_gain.cpu().numpy(), ref[2]) and np.array_equal(op.gains0.cpu().numpy(), ref[4])
        assert all(np.array_equal(_u32(covered[p]), ref[3][p]) for p in range(2))


# ---------------------------------------------------------------------------
# MapCoverPolicy on a real closed-loop env above 64^3 (tests/test_gain_masks_gpu.py's env at 72^3: MapCoverPolicy needs the belief
# flight field that construction adds)
# ---------------------------------------------------------------------------
ENV_N, ENV_G, EP_LEN = 3, 72, 5


def _env(seed=2):
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


@pytest.mark.parametrize("mask,weights", [("unknown", (1, 0)), ("mixed", (1, 4))])
def test_horizon_one_flies_what_map_greedy_flies_above_64(mask, weights):
    from gennbv_amd.eval.baselines import MapCoverPolicy, MapGreedyPolicy
    from gennbv_amd.ops.gain_masks import ViewGainMasksSlab
    from gennbv_amd.ops.view_gain import ViewGainSlab
    env_a, cfg = _env()
    env_b, _ = _env()
    pa = MapCoverPolicy(env_a, k=8, horizon=1, mask=mask, seed=7, stride=4, **(dict(weights=weights) if mask == "mixed" else {}))
    pb = MapGreedyPolicy(env_b, k=8, weights=weights, seed=7, stride=4)
    assert type(pa.gain_backend) is ViewGainMasksSlab and type(pb.gain_backend) is ViewGainSlab
    assert (pa.gain_backend.hit_bits is not None) == (mask == "mixed") and pa.gain_backend.unknown_bits is not None
    oa, ob = env_a.reset(), env_b.reset()
    gained = 0
    for step in range(EP_LEN + 2):  # a whole episode and its restart
        a, b = pa(oa)[0], pb(ob)[0]
        assert torch.equal(a, b), step
        assert torch.equal(pa.last_gain3, pb.last_gain) and bool(pa.adopted.all())
        if mask == "mixed":
            assert torch.equal(pa.last_gain[:, 0], pa.last_plane_gain[:, 0, 0] + 4 * pa.last_plane_gain[:, 0, 1])
        gained += int(pa.last_gain.sum())
        oa, ob = env_a.step(a)[0], env_b.step(b)[0]
        assert torch.equal(oa, ob)
    assert gained > 0

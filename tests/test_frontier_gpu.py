"""GPU: the frontier of the scanned map -- gnbv_frontier_tri (csrc/frontier.hip) against the numpy oracle (tests/frontier_oracle.py)
with == on every u32 of the bits (padding included) and every int32 of the block records, over grid sizes with unaligned rows,
both grid forms, every block size and slab height; the Frontier op on a real closed-loop env; and the greedy planners with
FrontierCandidates.  The mechanism is asserted, not planning quality: nobody has measured whether aimed candidates raise coverage."""
import functools

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import PI, TaskConfig
from tests import frontier_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x5A5A5A5A
BLOCKS = (1, 3, 4, 16)
RANDOM, FREE, UNKNOWN, OCCUPIED, SPARSE, ONE = range(6)


@functools.lru_cache(maxsize=None)
def _case(g):
    """int8 [N,G,G,G].  G < 60, six envs: random thirds of -1 / 0 / 1 with the int8 extremes, all free, all unknown, all occupied,
    sparse (5 % free, 3 % occupied in unknown space), one free voxel in unknown space.  Else two envs: random thirds and sparse."""
    rs = np.random.RandomState(g)
    if g >= 60:
        tri = rs.randint(-1, 2, (2, g, g, g)).astype(np.int8)
        u = rs.rand(g, g, g)
        tri[1] = np.where(u < 0.05, -1, np.where(u < 0.08, 1, 0))
    else:
        tri = rs.randint(-1, 2, (6, g, g, g)).astype(np.int8)
        tri[FREE], tri[UNKNOWN], tri[OCCUPIED] = -1, 0, 1
        u = rs.rand(g, g, g)
        tri[SPARSE] = np.where(u < 0.05, -1, np.where(u < 0.08, 1, 0))
        tri[ONE] = 0
        tri[ONE, g // 2, g - 1, 0] = -1  # on the edge of the faces y = G - 1 and z = 0: four neighbours
    ext = rs.rand(*tri.shape) < 0.3
    tri = np.where(ext & (tri < 0), -128, np.where(ext & (tri > 0), 127, tri)).astype(np.int8)
    assert (tri == -128).any() and (tri == 127).any() and (tri == 0).any()
    tri.setflags(write=False)
    return tri


@functools.lru_cache(maxsize=None)
def _front(g):
    f = FO.frontier_bool(_case(g))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _want(g, block):
    """The oracle's (words, records), computed once per (grid, block) and shared."""
    w, r = FO.pack_words(_front(g)), FO.block_records(_front(g), block)
    w.setflags(write=False)
    r.setflags(write=False)
    return w, r


@functools.lru_cache(maxsize=None)
def _forms(g):
    """The two grid forms on the device, with junk of the FREE class round every row: int8 rows with a padded row stride (-1), fp32
    rows inside an observation-shaped buffer (-5.0) -- a read past a row shows up as a false frontier."""
    tri = _case(g)
    n, g3 = tri.shape[0], g ** 3
    rows = torch.tensor(tri.reshape(n, g3)).to(DEV)  # (a copy: the cached case is read-only)
    i8 = torch.full((n, g3 + 5), -1, dtype=torch.int8, device=DEV)
    i8[:, :g3] = rows
    obs = torch.full((n, 7 + g3 + 3), -5.0, dtype=torch.float32, device=DEV)  # [state | grid | rgb]
    obs[:, 7:7 + g3] = rows.float()
    return {"i8": i8[:, :g3], "f32": obs[:, 7:7 + g3]}


def _launch(tri_t, g, block, slab, with_bits=True):
    """gnbv_frontier_tri at the C ABI into buffers pre-filled with 0x5A5A5A5A -> (return code, words or None, records)."""
    from gennbv_amd import _lib
    lib = _lib.load()
    n = tri_t.shape[0]
    nb = (g + block - 1) // block
    bits = torch.full((n, (g ** 3 + 31) // 32), FILL, dtype=torch.int32, device=DEV) if with_bits else None
    blocks = torch.full((n, nb ** 3, 4), FILL, dtype=torch.int32, device=DEV)
    i8 = tri_t.dtype == torch.int8
    row = int(tri_t.stride(0)) if n > 1 else g ** 3
    err = lib.gnbv_frontier_tri(tri_t.data_ptr() if i8 else None, row if i8 else 0, None if i8 else tri_t.data_ptr(), 0 if i8 else row,
                                g, n, block, None if bits is None else bits.data_ptr(), blocks.data_ptr(), slab, None)
    torch.cuda.synchronize()
    return err, None if bits is None else bits.cpu().numpy().view(np.uint32), blocks.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("g", [8, 12, 20, 37, 67])  # 12: unaligned rows; 37: G^3 odd, a tail word, rows that straddle words; 67: slabs
def test_frontier_equals_the_oracle_on_every_word_and_record(g, block):
    want_bits, want_rec = _want(g, block)
    first = None
    for name, t in _forms(g).items():
        for slab in (0, 1, 3, 7, g, 128):
            err, bits, rec = _launch(t, g, block, slab)
            assert err == 0
            assert np.array_equal(bits, want_bits), (name, slab, np.argwhere(bits != want_bits)[:5].tolist())
            assert np.array_equal(rec, want_rec), (name, slab, np.argwhere(rec != want_rec)[:5].tolist())
            first = rec if first is None else first
            assert np.array_equal(rec, first)  # the same for every slab and form
        err, bits, rec = _launch(t, g, block, 0, with_bits=False)  # bits_out = NULL leaves the records the same
        assert err == 0 and bits is None and np.array_equal(rec, want_rec), name


@pytest.mark.parametrize("g", [8, 12, 20, 37])
def test_the_cases_reach_what_they_are_there_for(g):
    front, (words, _) = _front(g), _want(g, 4)
    count = front.reshape(6, -1).sum(1)
    assert count[RANDOM] > 10 and count[SPARSE] > 10
    assert count[FREE] == 0 and count[UNKNOWN] == 0 and count[OCCUPIED] == 0 and count[ONE] == 4
    assert (words[[FREE, UNKNOWN, OCCUPIED]] == 0).all()
    pad = words.shape[1] * 32 - g ** 3
    if pad:
        assert (words[:, -1] >> np.uint32(32 - pad) == 0).all()  # padding bits clear
    for block in BLOCKS:
        rec = _want(g, block)[1]
        assert np.array_equal(rec[..., 0].sum(1), count)  # the per-env total is the sum of the counts
    # the wrap of a row would be seen: some unknown voxel at z = 0 follows a free voxel in memory without being a frontier voxel
    tri = _case(g)[RANDOM].reshape(-1)
    follows = np.zeros(g ** 3, bool)
    follows[1:] = (tri[:-1] < 0) & (tri[1:] == 0)
    at_z0 = (np.arange(g ** 3) % g) == 0
    assert (follows & at_z0 & ~front[RANDOM].reshape(-1)).any()


def test_the_large_grid_is_cut_into_slabs_and_its_edge_blocks_hold_frontier():
    g = 67
    front = _front(g)
    count = front.reshape(2, -1).sum(1)
    assert (count > 10).all()
    xs = np.nonzero(front)[1]
    assert (xs < 3).any() and (xs >= 64).any() and len(np.unique(xs // 16)) >= 2  # frontier in more than one slab of every height used
    for block in (3, 4, 16):  # 67 = 22 * 3 + 1 = 16 * 4 + 3 = 4 * 16 + 3: the last block of an axis is cut by the grid edge
        nb = (g + block - 1) // block
        rec = _want(g, block)[1].reshape(2, nb, nb, nb, 4)
        assert (rec[:, nb - 1, ..., 0] > 0).any() and (rec[:, :, nb - 1, :, 0] > 0).any() and (rec[..., nb - 1, 0] > 0).any()
        if block > 3:  # the corner block, cut on all three axes to 3^3 voxels (a single voxel where block = 3)
            assert rec[:, nb - 1, nb - 1, nb - 1, 0].sum() > 0


# ---------------------------------------------------------------------------
# 2. the op on a real closed-loop env, and the planners with FrontierCandidates
# ---------------------------------------------------------------------------
ENV_N, ENV_G, BLOCK, K = 4, 20, 4, 8


def _env_cfg():
    """The default task's volume on a coarser pose lattice (0.5 m), as the belief-flight tests have it."""
    return TaskConfig(camera_width=80, camera_height=60, grid_size=ENV_G, clip_pose_idx_up=[32, 32, 20, 0, 12, 12],
                      action_unit=[0.5, 0.5, 0.5, 0.0, PI / 12.0, PI / 6.0], init_action=[16, 16, 20, 0, 12, 0])


def _env(belief=False, max_len=30, seed=2):
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.flight import FlightLattice
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.ops.flight_field import BeliefFlightField
    cfg = _env_cfg()
    scene = S.make_scenes(ENV_N, ENV_G, seed=seed)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    kw = {}
    if belief:
        body = CollisionBody(sweep=True)
        kw = dict(collision=body, flight=BeliefFlightField(ENV_N, FlightLattice(cfg, stride=2), body, scene.range_gt, scene.voxel_size,
                                                           ENV_G, unknown="free", device=DEV))
    return ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=max_len, **kw), cfg, scene


def _tri(obs, cfg):
    return obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]


def _on_lattice(act, cfg):
    low, up = torch.tensor(cfg.clip_pose_idx_low, device=act.device), torch.tensor(cfg.clip_pose_idx_up, device=act.device)
    return act.dtype == torch.int64 and act.shape == (ENV_N, 6) and bool((act >= low).all()) and bool((act <= up).all())


def test_frontier_op_on_a_closed_loop_env_equals_the_oracle():
    from gennbv_amd import _lib
    from gennbv_amd.eval.baselines import RandomLatticePolicy
    from gennbv_amd.ops.frontier import Frontier
    env, cfg, scene = _env()
    pol = RandomLatticePolicy(cfg, ENV_N, seed=3)
    obs = env.reset()
    for _ in range(4):
        obs = env.step(pol(obs)[0])[0]
    tri = _tri(obs, cfg)
    host = tri.reshape(ENV_N, ENV_G, ENV_G, ENV_G).cpu().numpy()
    want_bits, want_rec = FO.frontier(host, BLOCK)
    fr = Frontier(ENV_N, ENV_G, block=BLOCK, device=DEV, keep_bits=True)
    assert fr.nb == 5 and fr.blocks.shape == (ENV_N, 125, 4) and fr.bits.shape == (ENV_N, 250)
    snapshot = torch.sign(tri).to(torch.int8).contiguous()
    for t in (tri, snapshot):  # the fp32 slice of the observation (row stride obs_dim), an int8 snapshot
        fr.blocks.fill_(FILL)
        fr.bits.fill_(FILL)
        assert fr(t) is fr.blocks
        assert np.array_equal(fr.blocks.cpu().numpy(), want_rec) and np.array_equal(fr.bits.cpu().numpy().view(np.uint32), want_bits)
    assert fr.launches == 2
    count = fr.count().cpu().numpy()
    assert (count > 0).all() and np.array_equal(count, want_rec[..., 0].sum(1))
    idx, cnt = fr.top(8)
    want_idx, want_cnt = FO.top_blocks(want_rec, 8)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(cnt.cpu().numpy(), want_cnt) and (want_cnt[:, 0] > 0).all()
    cent = fr.centroids(idx, scene.range_gt, scene.voxel_size)
    assert cent.dtype == torch.float64
    assert np.array_equal(cent.cpu().numpy(), FO.centroids(want_rec, want_idx, scene.range_gt.numpy(), scene.voxel_size.numpy()), equal_nan=True)
    plain = Frontier(ENV_N, ENV_G, block=BLOCK, device=DEV)  # keep_bits=False: no bits, the same records
    assert plain.bits is None and np.array_equal(plain(tri).cpu().numpy(), want_rec)
    for bad in (tri.cpu(), tri.double(), tri[:2], tri[:, :-1], tri[:, ::2]):
        with pytest.raises(_lib.GennbvHipError):
            fr(bad)


def _frontier_source(cfg, scene, seed, **kw):
    from gennbv_amd.eval.baselines import FrontierCandidates
    from gennbv_amd.ops.frontier import Frontier
    fr = Frontier(ENV_N, ENV_G, block=BLOCK, device=DEV)
    return FrontierCandidates(cfg, K, seed, fr, scene.range_gt, scene.voxel_size, **kw), fr


def _check_decisions(pol, env, cfg, src, fr, steps=3):
    """A few closed-loop decisions: the source is shown each step's map, the candidates are aimed, the actions lie on the lattice;
    then observe + sample once more with host synchronisation made an error."""
    from gennbv_amd.eval.baselines import LatticeCandidates
    plain = LatticeCandidates(cfg, K, 5)
    obs = env.reset()
    aimed = 0
    for step in range(steps):
        act = pol(obs)[0]
        assert _on_lattice(act, cfg) and fr.launches == step + 1
        want_rec = FO.frontier(_tri(obs, cfg).reshape(ENV_N, ENV_G, ENV_G, ENV_G).cpu().numpy(), BLOCK)[1]
        assert np.array_equal(src.blocks.cpu().numpy(), want_rec)  # this step's map
        base = plain.sample(ENV_N)
        assert pol.last_gain.shape == (ENV_N, K, 3)
        aimed += int((want_rec[..., 0].sum(1) > 0).sum())
        obs = env.step(act)[0]
    assert aimed >= ENV_N  # (the reset map has free space along the first view's rays: there is a frontier from step 0 on)
    tri = _tri(obs, cfg)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        cand = pol._sample(tri)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    base = plain.sample(ENV_N).to(DEV)
    assert cand.shape == (ENV_N, K, 6) and torch.equal(cand[..., :4], base[..., :4])  # the same base draw, aim alone differs
    low, up = torch.tensor(cfg.clip_pose_idx_low, device=DEV), torch.tensor(cfg.clip_pose_idx_up, device=DEV)
    assert bool((cand >= low).all()) and bool((cand <= up).all())
    # every aimed candidate looks towards its block's centroid: the forward axis has a positive component along c - p
    idx, cnt = fr.top(8)
    cent = fr.centroids(idx, src.range_gt, src.voxel_size)
    live = (cnt > 0).sum(1)
    assert bool((live > 0).all())
    rank = torch.arange(K, device=DEV)[None] % live[:, None]
    c = cent.gather(1, rank[..., None].expand(-1, -1, 3))
    pose = pol.cands.poses(cand).double()
    fwd = torch.stack([torch.cos(pose[..., 4]) * torch.cos(pose[..., 5]), torch.cos(pose[..., 4]) * torch.sin(pose[..., 5]),
                       -torch.sin(pose[..., 4])], -1)
    off = c - pose[..., :3]
    cosine = (fwd * off).sum(-1) / off.norm(dim=-1).clamp(min=1e-12)
    # half a lattice step of error on each angle at most (pi / 24 of pitch, pi / 12 of yaw): the view axis stays within 18 degrees
    assert bool((cosine[off.norm(dim=-1) > 1e-6] > 0.95).all()), cosine


def test_greedy_gain_policy_with_frontier_candidates():
    from gennbv_amd.eval.baselines import FrontierCandidates, GreedyGainPolicy
    env, cfg, scene = _env()
    src, fr = _frontier_source(cfg, scene, seed=5)
    pol = GreedyGainPolicy(env, k=K, candidates=src)
    assert pol.cands is src and isinstance(src, FrontierCandidates)
    _check_decisions(pol, env, cfg, src, fr)
    with pytest.raises(ValueError):
        GreedyGainPolicy(env, k=K + 1, candidates=src)


def test_map_greedy_policy_with_frontier_candidates_keeps_its_contact_rule():
    from gennbv_amd.eval.baselines import MapGreedyPolicy
    env, cfg, scene = _env(belief=True)
    src, fr = _frontier_source(cfg, scene, seed=5, radius_m=1.0)
    pol = MapGreedyPolicy(env, k=K, candidates=src)
    obs = env.reset()
    for step in range(3):
        act = pol(obs)[0]
        assert _on_lattice(act, cfg) and fr.launches == step + 1
        # the contact rule is the map planner's own: never an unreachable choice while a reachable candidate exists
        pose = S.poses_from_actions(act, cfg).float()
        chosen = env.flight.cost(pose[:, None])[:, 0]
        reach = pol._contact == 0
        assert torch.isfinite(chosen[reach.any(1)]).all()
        obs = env.step(act)[0]
    # radius_m: the positions were replaced, inside the clamp
    tri = _tri(obs, cfg)
    cand = pol._sample(tri)
    low, up = torch.tensor(cfg.clip_pose_idx_low, device=DEV), torch.tensor(cfg.clip_pose_idx_up, device=DEV)
    assert bool((cand >= low).all()) and bool((cand <= up).all())
    refused = ~env.flight.reachable(src.poses(cand))
    assert torch.equal(pol.contact(src.poses(cand)) != 0, refused)

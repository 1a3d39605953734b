"""CPU: the numpy oracle of gnbv_frontier_tri (tests/frontier_oracle.py) on hand-made cases, the entry point's argument refusals
(all made before any launch, so they need no GPU), FrontierCandidates on injected block summaries, and the planners' candidate
hook on a stub env."""
import math
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env.config import TaskConfig
from tests import frontier_oracle as FO

INVALID = 1  # hipErrorInvalidValue
G = 4


def _grid(fill=0, free=(), occupied=(), unknown=()):
    tri = np.full((1, G, G, G), fill, np.int8)
    for cells, val in ((free, -1), (occupied, 1), (unknown, 0)):
        for x, y, z in cells:
            tri[0, x, y, z] = val
    return tri


def _cells(front):
    return sorted(tuple(int(v) for v in c[1:]) for c in np.argwhere(front))


# ---------------------------------------------------------------------------
# the oracle on hand cases
# ---------------------------------------------------------------------------
def test_one_free_voxel_in_an_unknown_grid_gives_its_face_neighbours():
    assert _cells(FO.frontier_bool(_grid(free=[(1, 2, 1)]))) == sorted([(0, 2, 1), (2, 2, 1), (1, 1, 1), (1, 3, 1), (1, 2, 0), (1, 2, 2)])
    assert _cells(FO.frontier_bool(_grid(free=[(0, 0, 3)]))) == sorted([(1, 0, 3), (0, 1, 3), (0, 0, 2)])  # a corner: three
    assert _cells(FO.frontier_bool(_grid(free=[(0, 2, 3)]))) == sorted([(1, 2, 3), (0, 1, 3), (0, 3, 3), (0, 2, 2)])  # an edge: four


def test_no_frontier_through_the_wrap_of_a_row():
    # free at z = G - 1 of every row but the last, the rest occupied except unknown voxels at z = 0: in memory each unknown voxel
    # follows a free one, but they are not neighbours
    tri = _grid(fill=1)
    tri[0, :, :, G - 1] = -1
    tri[0, :, :, 0] = 0
    assert not FO.frontier_bool(tri).any()
    tri[0, 2, 1, 1] = -1  # a real neighbour of (2, 1, 0)
    assert _cells(FO.frontier_bool(tri)) == [(2, 1, 0)]
    # the same through the wrap of a plane: y = G - 1 free, y = 0 unknown
    tri = _grid(fill=1)
    tri[0, :, G - 1, :] = -1
    tri[0, :, 0, :] = 0
    assert not FO.frontier_bool(tri).any()


def test_uniform_grids_and_an_occupied_wall_give_none():
    for fill in (-1, 0, 1):
        assert not FO.frontier_bool(_grid(fill=fill)).any()
    tri = _grid(fill=0)
    tri[0, 0] = -1
    tri[0, 1] = 1  # an occupied plane between free and unknown
    assert not FO.frontier_bool(tri).any()
    tri[0, 1, 2, 2] = 0  # a hole in the wall: the hole itself is the frontier
    assert _cells(FO.frontier_bool(tri)) == [(1, 2, 2)]


def test_the_int8_extremes_keep_their_signs():
    tri = _grid(fill=127, free=[(1, 1, 1)], unknown=[(1, 1, 2), (3, 3, 3)])
    tri[tri < 0] = -128
    assert _cells(FO.frontier_bool(tri)) == [(1, 1, 2)]
    assert _cells(FO.frontier_bool(tri.astype(np.float32) * 0.25)) == [(1, 1, 2)]


def test_pack_words_and_block_records():
    f = np.zeros((2, 40), bool)
    f[0, [0, 31, 32]] = True
    w = FO.pack_words(f)
    assert w.dtype == np.uint32 and w.shape == (2, 2)
    assert w[0].tolist() == [0x80000001, 0x00000001] and w[1].tolist() == [0, 0]  # padding bits clear
    front = np.zeros((1, 5, 5, 5), bool)
    for c in ((0, 0, 0), (1, 1, 1), (4, 4, 4), (4, 1, 3), (2, 0, 4)):
        front[(0,) + c] = True
    rec = FO.block_records(front, 2)  # nb = 3: the last block of an axis is cut by the grid edge
    assert rec.dtype == np.int32 and rec.shape == (1, 27, 4)
    assert rec[0, 0].tolist() == [2, 1, 1, 1] and rec[0, 26].tolist() == [1, 4, 4, 4]
    assert rec[0, (2 * 3 + 0) * 3 + 1].tolist() == [1, 4, 1, 3] and rec[0, (1 * 3 + 0) * 3 + 2].tolist() == [1, 2, 0, 4]
    assert rec[0, :, 0].sum() == 5
    one = FO.block_records(front, 16)  # B > G: one block
    assert one.shape == (1, 1, 4) and one[0, 0].tolist() == [5, 11, 6, 12]


# ---------------------------------------------------------------------------
# the C ABI refuses before it launches
# ---------------------------------------------------------------------------
def test_argument_refusals_at_the_c_abi():
    from gennbv_amd import _lib
    lib = _lib.load()
    assert lib.gnbv_abi_version() == 5
    fake = 0x1000  # never dereferenced: every call below is refused before a launch

    def call(i8=fake, i8_stride=8 ** 3, f32_=None, f32_stride=0, g=8, n=2, block=4, bits=fake, blocks=fake, slab=0):
        return lib.gnbv_frontier_tri(i8, i8_stride, f32_, f32_stride, g, n, block, bits, blocks, slab, None)
    for kw in (dict(i8=None), dict(f32_=fake, f32_stride=8 ** 3), dict(blocks=None), dict(n=0), dict(n=-3), dict(g=0),
               dict(g=129, i8_stride=129 ** 3), dict(block=0), dict(block=17), dict(i8_stride=8 ** 3 - 1),
               dict(i8=None, f32_=fake, f32_stride=8 ** 3 - 1), dict(slab=-1)):
        assert call(**kw) == INVALID, kw


def test_the_op_refuses_to_run_off_the_gpu():
    from gennbv_amd import _lib
    from gennbv_amd.ops.frontier import Frontier
    with pytest.raises(_lib.GennbvHipError):
        Frontier(2, 8, device="cpu")
    for kw in (dict(grid_size=0), dict(grid_size=129), dict(block=0), dict(block=17), dict(slab=-1), dict(num_envs=0)):
        with pytest.raises(ValueError):
            Frontier(**{**dict(num_envs=2, grid_size=8, device="cpu"), **kw})


# ---------------------------------------------------------------------------
# top / centroids on the CPU, against the oracle
# ---------------------------------------------------------------------------
def test_top_ties_go_to_the_lowest_block_and_centroids_use_the_voxel_frame():
    from gennbv_amd.ops.frontier import block_centroids, top_blocks
    rec = np.zeros((2, 27, 4), np.int32)
    rec[0, [5, 9, 20], 0] = 7  # three equal counts
    rec[0, 13, 0] = 9
    rec[0, [5, 9, 13, 20], 1:] = [[7, 14, 21], [0, 7, 35], [9, 18, 27], [70, 0, 7]]
    rec[1, 26] = [3, 12, 12, 13]
    idx, cnt = top_blocks(torch.as_tensor(rec), 5)
    assert idx[0].tolist()[:4] == [13, 5, 9, 20] and cnt[0].tolist() == [9, 7, 7, 7, 0]
    assert idx[0, 4].item() == 0  # among the empty ones too: the lowest index
    assert idx[1].tolist() == [26, 0, 1, 2, 3] and cnt[1].tolist() == [3, 0, 0, 0, 0]
    want_idx, want_cnt = FO.top_blocks(rec, 5)
    assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(cnt.numpy(), want_cnt)
    rng = np.array([[7.3, -7.3, 7.3, -7.3, 11.9, 0.1], [3.5, 0.5, 3.5, 0.5, 3.5, 0.5]], np.float32)
    vox = np.array([[0.77, 0.77, 0.6], [1.0, 1.0, 1.0]], np.float32)
    got = block_centroids(torch.as_tensor(rec), idx, torch.as_tensor(rng), torch.as_tensor(vox))
    want = FO.centroids(rec, want_idx, rng, vox)
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want, equal_nan=True)
    assert got[1, 0].tolist() == [4.5, 4.5, 13.0 / 3.0 + 0.5]  # o = 0, v = 1: mean index + one half
    assert torch.isnan(got[1, 1:]).all() and not torch.isnan(got[0, :4]).any()
    with pytest.raises(ValueError):
        top_blocks(torch.as_tensor(rec), 28)


# ---------------------------------------------------------------------------
# FrontierCandidates with injected summaries
# ---------------------------------------------------------------------------
N_ENVS, K, NB, BLOCK = 4, 12, 5, 4  # a 20^3 grid in blocks of 4
RANGE = torch.tensor([[4.75, -4.75, 4.75, -4.75, 4.875, 0.125]] * N_ENVS)  # voxels over [-5, 5]^2 x [0, 5]: binary fractions, an exact frame
VOXEL = torch.tensor([[0.5, 0.5, 0.25]] * N_ENVS)


def _summary():
    """Block records [4, 125, 4]: env 0 has three non-empty blocks (fewer than top), env 1 none, env 2 more than top, env 3 one
    block whose centroid lies exactly below a lattice column."""
    rs = np.random.RandomState(4)
    rec = np.zeros((N_ENVS, NB ** 3, 4), np.int32)

    def put(e, b, count):
        bx, by, bz = b // (NB * NB), (b // NB) % NB, b % NB
        pts = np.stack([rs.randint(BLOCK * c, BLOCK * c + BLOCK, count) for c in (bx, by, bz)], -1)
        rec[e, b] = [count, *pts.sum(0)]
    for b, c in ((7, 30), (93, 12), (41, 21)):
        put(0, b, c)
    for b in rs.choice(NB ** 3, 20, replace=False):
        put(2, int(b), int(rs.randint(1, 50)))
    rec[3, 62] = [2, 2 * 10 - 1, 2 * 10 - 1, 2 * 9]  # mean index 9.5 -> x = y = -5 + 10 * 0.5 = 0.0: the lattice column x = y = 0
    return rec


def _frontier_cands(seed=3, **kw):
    from gennbv_amd.eval.baselines import FrontierCandidates
    cfg = TaskConfig()
    fc = FrontierCandidates(cfg, K, seed, frontier=None, range_gt=RANGE, voxel_size=VOXEL, **kw)
    return cfg, fc


def _angles(cfg, ax):
    return np.arange(cfg.clip_pose_idx_low[ax], cfg.clip_pose_idx_up[ax] + 1) * np.float64(cfg.action_unit[ax]) + np.float64(cfg.clip_pose_low[ax])


def test_frontier_candidates_base_draw_round_robin_and_aim():
    from gennbv_amd.eval.baselines import LatticeCandidates
    cfg, fc = _frontier_cands(top=8)
    plain = LatticeCandidates(cfg, K, 3)
    assert torch.equal(fc.sample(N_ENVS), plain.sample(N_ENVS))  # nothing observed yet: the base draw itself
    rec = _summary()
    fc.set_blocks(torch.as_tensor(rec))
    for _ in range(2):  # the generators stay in step draw after draw
        base, got = plain.sample(N_ENVS), fc.sample(N_ENVS)
        assert got.dtype == torch.int64 and got.shape == (N_ENVS, K, 6)
        assert torch.equal(got[1], base[1])  # an env without frontier gets its base candidates unchanged
        assert torch.equal(got[..., :4], base[..., :4])  # radius_m=None: the two sources differ in aim only
        low, up = torch.tensor(cfg.clip_pose_idx_low), torch.tensor(cfg.clip_pose_idx_up)
        assert (got >= low).all() and (got <= up).all()
        idx, cnt = FO.top_blocks(rec, 8)
        cent = FO.centroids(rec, idx, RANGE.numpy(), VOXEL.numpy())
        yaws, pitches = _angles(cfg, 5), _angles(cfg, 4)
        aimed_off_axis = 0
        for e in (0, 2, 3):
            live = int((cnt[e] > 0).sum())
            assert live == {0: 3, 2: 8, 3: 1}[e]
            for j in range(K):
                c = cent[e, j % live]  # round-robin over the M' non-empty blocks
                p = base[e, j, :3].numpy() * np.array(cfg.action_unit[:3]) + np.array(cfg.clip_pose_low[:3])
                dx, dy = c[0] - p[0], c[1] - p[1]
                want_pitch = math.atan2(p[2] - c[2], math.hypot(dx, dy))
                d_pitch = np.abs(pitches - want_pitch)
                assert d_pitch[int(got[e, j, 4]) - cfg.clip_pose_idx_low[4]] <= d_pitch.min() + 1e-9
                if dx == 0.0 and dy == 0.0:
                    assert got[e, j, 5] == base[e, j, 5]  # straight above or below: the base yaw stays
                    continue
                aimed_off_axis += 1
                d_yaw = np.abs(np.remainder(yaws - math.atan2(dy, dx) + math.pi, 2 * math.pi) - math.pi)
                assert d_yaw[int(got[e, j, 5]) - cfg.clip_pose_idx_low[5]] <= d_yaw.min() + 1e-9
                # and the camera does look that way: the forward axis of camera_to_world has a positive component towards c
                yaw, pitch = yaws[int(got[e, j, 5])], pitches[int(got[e, j, 4])]
                fwd = np.array([math.cos(pitch) * math.cos(yaw), math.cos(pitch) * math.sin(yaw), -math.sin(pitch)])
                assert fwd @ (c - p) > 0.0
        assert aimed_off_axis >= 2 * K
        assert (got[[0, 2, 3], :, 4:] != base[[0, 2, 3], :, 4:]).any()


def test_frontier_candidates_zero_horizontal_offset_keeps_the_base_yaw():
    cfg, fc = _frontier_cands(top=8, radius_m=0.0)  # r = 0: every candidate of env 3 sits on the lattice column of its one centroid
    rec = _summary()
    fc.set_blocks(torch.as_tensor(rec))
    from gennbv_amd.eval.baselines import LatticeCandidates
    base, got = LatticeCandidates(cfg, K, 3).sample(N_ENVS), fc.sample(N_ENVS)
    assert (got[3, :, 0] == 40).all() and (got[3, :, 1] == 40).all()  # x = y = 0.0 m is index 40
    assert torch.equal(got[3, :, 5], base[3, :, 5])
    z = got[3, :, 2].double() * 0.2 + 0.1
    cz = (9.0 + 0.5) * 0.25  # straight down or up, by the sign of the height difference
    above = (z > cz + 1e-9).numpy()
    assert (got[3, :, 4].numpy()[above] == 12).all() and (got[3, :, 4].numpy()[~above] == 0).all()


def test_frontier_candidates_radius_positions():
    from gennbv_amd.eval.baselines import LatticeCandidates
    radius, r = 4.1, 20  # r = floor(4.1 / 0.2) = 20 steps on every axis: far enough for the clamp to bite
    cfg, fc = _frontier_cands(top=4, radius_m=radius)
    rec = _summary()
    fc.set_blocks(torch.as_tensor(rec))
    base, got = LatticeCandidates(cfg, K, 3).sample(N_ENVS), fc.sample(N_ENVS)
    assert torch.equal(got[1], base[1])
    low, up = np.array(cfg.clip_pose_idx_low[:3]), np.array(cfg.clip_pose_idx_up[:3])
    unit, off = np.array(cfg.action_unit[:3]), np.array(cfg.clip_pose_low[:3])
    idx, cnt = FO.top_blocks(rec, 4)
    cent = FO.centroids(rec, idx, RANGE.numpy(), VOXEL.numpy())
    clamped = 0
    for e in (0, 2, 3):
        live = int((cnt[e] > 0).sum())
        assert live == {0: 3, 2: 4, 3: 1}[e]
        for j in range(K):
            c = cent[e, j % live]
            lattice = [np.arange(low[a], up[a] + 1) * unit[a] + off[a] for a in range(3)]
            near = np.array([low[a] + int(np.argmin(np.abs(lattice[a] - c[a]))) for a in range(3)])
            pos = got[e, j, :3].numpy()
            assert (pos >= low).all() and (pos <= up).all() and (np.abs(pos - near) <= r).all()
            moved = near + base[e, j, :3].numpy() % (2 * r + 1) - r
            want = np.clip(moved, low, up)
            assert (pos == want).all()
            clamped += int((moved != want).any())
            assert got[e, j, 3] == base[e, j, 3]
    assert clamped > 0 and (got[[0, 2, 3], :, :3] != base[[0, 2, 3], :, :3]).any()
    # an axis whose unit is 0 keeps r = 0 and index 0
    flat = TaskConfig(clip_pose_idx_up=[80, 80, 0, 0, 12, 12], action_unit=[0.2, 0.2, 0.0, 0.0, math.pi / 12.0, math.pi / 6.0])
    from gennbv_amd.eval.baselines import FrontierCandidates
    fc = FrontierCandidates(flat, K, 3, None, RANGE, VOXEL, top=4, radius_m=radius)
    fc.set_blocks(torch.as_tensor(rec))
    assert (fc.sample(N_ENVS)[..., 2] == 0).all()
    for bad in (dict(top=0), dict(radius_m=-0.1), dict(radius_m=math.nan)):
        with pytest.raises(ValueError):
            FrontierCandidates(cfg, K, 3, None, RANGE, VOXEL, **bad)


# ---------------------------------------------------------------------------
# the planners' hook
# ---------------------------------------------------------------------------
class _Source:
    """A candidate source that records what it is shown."""

    def __init__(self, cfg, k, with_observe=True):
        from gennbv_amd.eval.baselines import LatticeCandidates
        self.k, self.base, self.seen = k, LatticeCandidates(cfg, k, 0), []
        if with_observe:
            self.observe = self.seen.append

    def sample(self, num_envs, device="cpu"):
        self.seen.append("sample")
        return self.base.sample(num_envs, device)

    def poses(self, actions):
        return self.base.poses(actions)


def test_the_planners_take_a_candidate_source():
    from gennbv_amd.eval.baselines import GreedyGainPolicy, LatticeCandidates, MapGreedyPolicy
    cfg, n, k = TaskConfig(), 3, 5
    env = types.SimpleNamespace(cfg=cfg, num_envs=n, collision=None, device="cpu", flight=None)
    shown = []

    def gain(tri, poses):
        shown.append(tri)
        return torch.arange(n * k * 3, dtype=torch.int32).reshape(n, k, 3)
    obs = torch.zeros(n, cfg.state_dim + cfg.grid_dim + 8)
    tri = obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]
    # None: LatticeCandidates, as ever
    pol = GreedyGainPolicy(env, k=k, seed=9, gain_backend=gain)
    assert type(pol.cands) is LatticeCandidates and pol.cands.k == k
    want = LatticeCandidates(cfg, k, 9).sample(n)
    assert torch.equal(pol(obs)[0], want[:, k - 1])  # the gain rises with the candidate index
    # a source with observe: shown the step's tri slice once per decision, before sample
    src = _Source(cfg, k)
    pol = GreedyGainPolicy(env, k=k, gain_backend=gain, candidates=src)
    assert pol.cands is src
    for step in range(2):
        act = pol(obs)[0]
        assert act.shape == (n, 6)
    assert len(src.seen) == 4 and src.seen[1] == "sample" and src.seen[3] == "sample"
    for t in (src.seen[0], src.seen[2]):
        assert t.data_ptr() == tri.data_ptr() and t.shape == tri.shape and t.stride() == tri.stride()
    assert shown[-1].data_ptr() == tri.data_ptr()  # the gain sees the same slice
    # a source without observe is only sampled
    src = _Source(cfg, k, with_observe=False)
    GreedyGainPolicy(env, k=k, gain_backend=gain, candidates=src)(obs)
    assert src.seen == ["sample"]
    # a wrong k
    with pytest.raises(ValueError):
        GreedyGainPolicy(env, k=k + 1, gain_backend=gain, candidates=src)
    # the map planner: the same hook, its own contact rule
    flight = types.SimpleNamespace(num_envs=n, belief=True, shortcut=False, reachable=lambda poses: torch.ones(n, k, dtype=torch.bool))
    menv = types.SimpleNamespace(cfg=cfg, num_envs=n, collision=None, device="cpu", flight=flight)
    assert type(MapGreedyPolicy(menv, k=k, gain_backend=gain).cands) is LatticeCandidates
    src = _Source(cfg, k)
    pol = MapGreedyPolicy(menv, k=k, gain_backend=gain, candidates=src)
    assert pol.cands is src and MapGreedyPolicy.contact is not GreedyGainPolicy.contact
    act = pol(obs)[0]
    assert len(src.seen) == 2 and src.seen[0].data_ptr() == tri.data_ptr() and src.seen[1] == "sample"
    assert torch.equal(act, LatticeCandidates(cfg, k, 0).sample(n)[:, k - 1]) and pol._contact.tolist() == [[0] * k] * n
    with pytest.raises(ValueError):
        MapGreedyPolicy(menv, k=k + 2, gain_backend=gain, candidates=src)

"""CPU: the frontier viewpoints without a GPU -- the oracle (tests/frontview_oracle.py) on hand-made cases, what the random cases of
the GPU test reach (checked with the oracle alone, so that the GPU test cannot pass trivially), the argument refusals of
gnbv_frontier_viewpoints at the C ABI with a pointer that is never dereferenced, the torch glue of ops/frontier_view.py, and the
selection of FrontierViewPolicy with the kernel replaced by an injected backend."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from gennbv_amd import _lib
from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import PI, TaskConfig
from gennbv_amd.env.flight import FlightLattice
from gennbv_amd.ops.frontier import block_centroids, top_blocks
from gennbv_amd.ops.frontier_view import FrontierViewpoints, aim_indices, block_target_voxels, node_actions
from tests import frontview_cases as FC
from tests import frontview_oracle as VO

INF = 0xFFFFFFFF
INVALID = 1  # hipErrorInvalidValue


# ---------------------------------------------------------------------------
# 1. the oracle on hand-made cases: an 8^3 grid of unit voxels centred on the integers (voxel i spans [i - 0.5, i + 0.5]), eight
#    nodes along x at (i, 3, 3) -- node i stands in voxel (i, 3, 3) -- and the target voxel (6, 3, 3)
# ---------------------------------------------------------------------------
G = 8
RANGE = np.array([7.0, 0.0, 7.0, 0.0, 7.0, 0.0], np.float32)
VOX = np.ones(3, np.float32)
DIMS, LO, H = (8, 1, 1), np.array([0.0, 3.0, 3.0]), np.array([1.0, 0.0, 0.0])
TARGET = np.array([[6, 3, 3]])


def _row(tri, field=None, targets=TARGET, r_min=0.0, r_max=100.0, max_unknown=0):
    field = np.arange(8, dtype=np.uint32) * 10 + 100 if field is None else np.asarray(field, np.uint32)
    node, cost, count, tied, _ = VO.viewpoints_env(tri, RANGE, VOX, DIMS, LO, H, field, targets, r_min, r_max, max_unknown)
    return node.tolist(), cost.tolist(), count.tolist(), tied.tolist()


def _free():
    return np.full((G, G, G), -1, np.int8)


def test_oracle_a_wall_between_node_and_target_hides_it_and_a_wall_behind_does_not():
    tri = _free()
    tri[4, 3, 3] = 1
    # nodes 0 .. 3 look through the wall, node 4 stands in it (w_0 is its own voxel); 5, 6 (L = 0) and 7 see the target
    assert _row(tri) == ([5], [150], [[3, 3]], [False])
    tri = _free()
    tri[7, 3, 3] = 1  # behind the target for the nodes 0 .. 6; node 7 stands in it
    assert _row(tri) == ([0], [100], [[7, 7]], [False])


def test_oracle_max_unknown_counts_the_unknown_voxels_on_the_line():
    tri = _free()
    tri[5, 3, 3] = 0
    assert _row(tri, max_unknown=0) == ([6], [160], [[2, 2]], [False])  # 6 (L = 0) and 7 alone
    assert _row(tri, max_unknown=1) == ([0], [100], [[8, 8]], [False])


def test_oracle_a_source_inside_the_target_voxel_sees_it_whatever_its_class():
    tri = np.full((G, G, G), 1, np.int8)  # all occupied: every other node stands in an occupied voxel
    assert _row(tri) == ([6], [160], [[1, 1]], [False])


def test_oracle_a_target_outside_the_grid_is_no_target():
    for t in ([-1, 3, 3], [6, 8, 3], [6, 3, 1000]):
        assert _row(_free(), targets=np.array([t])) == ([-1], [INF], [[0, 0]], [False])


def test_oracle_ties_go_to_the_lowest_node_and_a_node_without_a_route_is_counted_only():
    field = [INF, 500, 700, 500, 900, 500, 900, INF]
    # node 0 would be first by id but has no route: skipped, counted in count[0] only; 1, 3 and 5 tie at 500: the lowest id wins
    assert _row(_free(), field=field) == ([1], [500], [[8, 6]], [True])
    assert _row(_free(), field=[INF] * 8) == ([-1], [INF], [[8, 0]], [False])


def test_oracle_r_min_excludes_the_nearest_node_and_r_max_the_far_ones():
    field = [900, 900, 900, 900, 900, 500, 100, 300]
    assert _row(_free(), field=field) == ([6], [100], [[8, 8]], [False])
    assert _row(_free(), field=field, r_min=0.5) == ([7], [300], [[7, 7]], [False])   # node 6 is at distance 0
    assert _row(_free(), field=field, r_min=1.0, r_max=1.0) == ([7], [300], [[2, 2]], [False])  # both bounds are closed
    assert _row(_free(), field=field, r_min=1.5, r_max=2.5) == ([4], [900], [[1, 1]], [False])


def test_oracle_the_line_is_bresenhams_from_the_source():
    """A diagonal: the line from node 0's voxel (0, 3, 3) to (6, 5, 3) passes (3, 4, 3) -- and not (3, 5, 3) or (3, 3, 3); the line
    back from (6, 5, 3) is another one (Bresenham is not symmetric), and the oracle walks from the node."""
    from oracle import oracle as O
    target = np.array([[6, 5, 3]], np.int32)

    def line(src, dst):
        traj, lens = O.bresenham3d(np.array(src, np.int32), np.array([dst], np.int32), G)
        return [tuple(int(v) for v in p) for p in traj[0, :lens[0]]]
    lines = [line((i, 3, 3), (6, 5, 3)) for i in range(8)]
    assert (3, 4, 3) in lines[0] and (3, 5, 3) not in lines[0] and (3, 3, 3) not in lines[0] and lines[0][-1] == (6, 5, 3)
    assert any(set(line((6, 5, 3), (i, 3, 3))) != set(lines[i]) for i in range(8))
    for wall in ((3, 4, 3), (4, 4, 3), (5, 5, 3)):
        tri = _free()
        tri[wall] = 1
        seen = [i for i in range(8) if wall not in lines[i][:-1]]
        assert 0 < len(seen) < 8
        node, cost, count, _ = _row(tri, targets=target)
        assert node == [seen[0]] and cost == [100 + 10 * seen[0]] and count == [[len(seen), len(seen)]]


# ---------------------------------------------------------------------------
# 2. what the random cases of tests/test_frontview_gpu.py reach, per grid size
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("g", FC.GRIDS)
def test_the_random_cases_reach_what_they_are_there_for(g):
    ws = [FC.want(g, ci) for ci in range(len(FC.CONFIGS))]
    node = np.concatenate([w["node"].ravel() for w in ws])
    in_range = np.concatenate([w["in_range"].ravel() for w in ws])
    tied = np.concatenate([w["tied"].ravel() for w in ws])
    count = np.concatenate([w["count"].reshape(-1, 2) for w in ws])
    assert (node >= 0).mean() >= 0.25                 # at least a quarter of the (env, target) pairs have a node
    assert ((node < 0) & (in_range > 0)).any()        # none although nodes are in range
    assert tied.any()                                 # a winner decided by the tie rule
    assert (count[:, 0] > count[:, 1]).any()          # nodes that see the target but have no route
    assert ((in_range > 0) & (count[:, 0] == 0)).any() and (in_range > count[:, 0]).any()  # lines of sight are lost
    for ci, w in enumerate(ws):
        c = FC.case(g, ci)
        m = int(np.prod(c["dims"]))
        small = c["r_max"] < 2.0
        # a small r_max keeps most of the lattice out of range of every target; a large one holds all of it but what r_min excludes
        assert (w["in_range"].max() < m // 2) if small else (w["in_range"].max() > m - 8)
    # the lattices stick out of the grid on every side
    tri, range_gt, voxel_size = FC.grid_case(g)
    for name in ("box", "flat"):
        dims, lo, h = FC.lattice(name)
        hi = lo + h * (np.array(dims) - 1)
        o = range_gt[:, 1::2].astype(np.float64) - 0.5 * voxel_size
        axes = [0, 1, 2] if name == "box" else [0, 1]
        assert (lo[axes] < o[:, axes]).all() and (hi[axes] > o[:, axes] + g * voxel_size[:, axes].astype(np.float64)).all()


def test_the_large_grid_is_above_the_lds_limit():
    lib = _lib.load()
    limit = int(lib.gnbv_frontview_lds_max_grid())
    assert limit == 86 and limit < FC.GRIDS[-1] <= 128 and all(g <= limit for g in FC.GRIDS[:-1])


# ---------------------------------------------------------------------------
# 3. the argument refusals at the C ABI: every pointer is this never-dereferenced address
# ---------------------------------------------------------------------------
FAKE = 0x1000


def _args(**kw):
    a = _lib.GnbvFrontView(n=2, t=3, g=20, tri_i8=FAKE, tri_i8_row_stride=8000, tri_f32=None, tri_f32_row_stride=0, range_gt=FAKE,
                           voxel_size=FAKE, nx=7, ny=6, nz=1, lo=(C.c_double * 3)(-1.0, -1.0, 0.5), h=(C.c_double * 3)(0.4, 0.4, 0.0),
                           field=FAKE, targets=FAKE, r_min=0.5, r_max=2.0, max_unknown=0, node_out=FAKE, cost_out=FAKE, count_out=FAKE,
                           chunk=0, mode=0)
    for k, v in kw.items():
        setattr(a, k, (C.c_double * 3)(*v) if k in ("lo", "h") else v)
    return a


REFUSED = {
    "both grid forms": dict(tri_f32=FAKE, tri_f32_row_stride=8000),
    "neither grid form": dict(tri_i8=None),
    "NULL range_gt": dict(range_gt=None),
    "NULL voxel_size": dict(voxel_size=None),
    "NULL field": dict(field=None),
    "NULL targets": dict(targets=None),
    "NULL node_out": dict(node_out=None),
    "NULL cost_out": dict(cost_out=None),
    "NULL count_out": dict(count_out=None),
    "n < 1": dict(n=0),
    "t < 1": dict(t=0),
    "N T > 2^31 - 1": dict(n=1 << 16, t=1 << 15),
    "G < 1": dict(g=0),
    "G > 128": dict(g=129, tri_i8_row_stride=129 ** 3),
    "row stride below G^3": dict(tri_i8_row_stride=7999),
    "f32 row stride below G^3": dict(tri_i8=None, tri_f32=FAKE, tri_f32_row_stride=7999),
    "lattice axis < 1": dict(ny=0),
    "lattice axis > 1024": dict(nx=1025),
    "lo not finite": dict(lo=(-1.0, math.inf, 0.5)),
    "h not finite": dict(h=(0.4, math.nan, 0.0)),
    "h <= 0 on an axis with more than one node": dict(h=(0.4, 0.0, 0.0)),
    "r_min not finite": dict(r_min=math.nan),
    "r_max not finite": dict(r_max=math.inf),
    "r_min < 0": dict(r_min=-0.1),
    "r_max <= 0": dict(r_min=0.0, r_max=0.0),
    "r_min > r_max": dict(r_min=2.5),
    "max_unknown < 0": dict(max_unknown=-1),
    "chunk < 0": dict(chunk=-1),
    "mode < 0": dict(mode=-1),
    "mode > 2": dict(mode=3),
    "mode 1 above its limit": dict(g=87, tri_i8_row_stride=87 ** 3, mode=1),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_bad_arguments_are_refused_before_any_launch(what):
    lib = _lib.load()
    assert lib.gnbv_frontier_viewpoints(C.byref(_args(**REFUSED[what])), None) == INVALID, what


def test_a_null_struct_is_refused_and_the_op_is_gpu_only():
    lib = _lib.load()
    assert lib.gnbv_frontier_viewpoints(None, None) == INVALID
    lat = FlightLattice(TaskConfig(), stride=2)
    with pytest.raises(_lib.GennbvHipError):
        FrontierViewpoints(2, 20, lat, torch.zeros(2, 6), torch.ones(2, 3), 4, 0.5, 2.0, device="cpu")
    for bad in (dict(targets=0), dict(r_min_m=3.0), dict(r_max_m=0.0), dict(max_unknown=-1), dict(mode=3)):
        kw = dict(targets=4, r_min_m=0.5, r_max_m=2.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            FrontierViewpoints(2, 20, lat, torch.zeros(2, 6), torch.ones(2, 3), **kw)


# ---------------------------------------------------------------------------
# 4. the torch glue
# ---------------------------------------------------------------------------
def test_block_target_voxels_is_the_floor_of_the_mean_and_minus_one_where_empty():
    blocks = torch.tensor([[[3, 10, 11, 2], [0, 0, 0, 0], [1, 7, 0, 19]],
                           [[0, 0, 0, 0], [4, 3, 4, 5], [2, 39, 1, 0]]], dtype=torch.int32)
    index = torch.tensor([[2, 0, 1], [1, 1, 0]])
    got = block_target_voxels(blocks, index)
    assert got.dtype == torch.int32 and got.shape == (2, 3, 3)
    assert got.tolist() == [[[7, 0, 19], [3, 3, 0], [-1, -1, -1]], [[0, 1, 1], [0, 1, 1], [-1, -1, -1]]]


@pytest.mark.parametrize("unit_x", [0.5, -0.5])
def test_node_actions_are_the_lattice_poses_of_the_nodes(unit_x):
    cfg = TaskConfig(grid_size=20, clip_pose_idx_up=[32, 30, 20, 0, 12, 12], clip_pose_idx_low=[2, 0, 4, 0, 0, 0],
                     action_unit=[unit_x, 0.5, 0.25, 0.0, PI / 12.0, PI / 6.0])
    lat = FlightLattice(cfg, stride=2)
    node = torch.arange(lat.num_nodes).reshape(2, -1)
    act = node_actions(lat, cfg, node)
    assert act.dtype == torch.int64 and act.shape == (2, lat.num_nodes // 2, 3)
    low, up = torch.tensor(cfg.clip_pose_idx_low[:3]), torch.tensor(cfg.clip_pose_idx_up[:3])
    assert bool((act >= low).all()) and bool((act <= up).all())
    full = torch.cat([act, torch.zeros_like(act)], -1)
    pose = S.poses_from_actions(full.double(), cfg)[..., :3]
    want = torch.as_tensor(lat.node_positions()).reshape(2, -1, 3)
    assert torch.allclose(pose.double(), want, rtol=0, atol=1e-6)  # (poses_from_actions rounds the unit to fp32)
    # a negative id is read as node 0
    assert torch.equal(node_actions(lat, cfg, torch.tensor([[-1, -7]])), act[:1, :1].expand(1, 2, 3))


def test_aim_indices_look_at_the_point():
    cfg = TaskConfig()
    unit, low = torch.tensor(cfg.action_unit).double(), torch.tensor(cfg.clip_pose_low).double()
    ang = {ax: torch.arange(cfg.clip_pose_idx_low[ax], cfg.clip_pose_idx_up[ax] + 1).double() * unit[ax] + low[ax] for ax in (4, 5)}
    p = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [1.0, 1.0, 5.0], [1.0, 1.0, 5.0]]).double()
    c = torch.tensor([[3.0, 0.0, 2.0], [0.0, -3.0, 2.0], [1.0, 1.0, 0.0], [-2.0, 1.0, 5.0]]).double()
    base = torch.tensor([9, 9, 9, 9])
    pitch, yaw = aim_indices(p, c, ang[4], ang[5], 0, 0, base)
    # level pitch is index 6 (-pi / 2 + 6 pi / 12 = 0); straight down is pitch +pi / 2, index 12, and keeps the base yaw
    assert pitch.tolist() == [6, 6, 12, 6]
    assert yaw.tolist() == [0, 9, 9, 6]  # 0, 3 pi / 2, (kept), pi


# ---------------------------------------------------------------------------
# 5. FrontierViewPolicy's selection with injected backends
# ---------------------------------------------------------------------------
PN, PG, PB = 3, 8, 4  # envs, grid, block: 2^3 = 8 blocks


class _Fallback:
    def __init__(self, act):
        self.act, self.calls = act, 0

    def __call__(self, obs, deterministic=True):
        self.calls += 1
        return self.act, None, None


class _Views:
    """The injected backend: fixed outputs, and the arguments of every call."""

    def __init__(self, node, cost):
        self.node = torch.tensor(node, dtype=torch.int32)
        self.cost = torch.tensor(np.asarray(cost, np.int64).astype(np.uint32).view(np.int32))
        self.calls = []

    def __call__(self, tri, field, vox):
        self.calls.append((field, vox.clone()))
        return self.node, self.cost, torch.zeros(PN, self.node.shape[1], 2, dtype=torch.int32)


def _policy_env():
    cfg = TaskConfig(grid_size=PG)
    lat = FlightLattice(cfg, stride=2)
    range_gt = torch.tensor([[2.0, -2.0, 2.0, -2.0, 4.0, 0.0]] * PN)
    voxel_size = torch.full((PN, 3), 0.5)
    flight = types.SimpleNamespace(belief=True, lattice=lat, range_gt=range_gt, voxel_size=voxel_size, field=torch.zeros(PN, lat.num_nodes, dtype=torch.int32))
    env = types.SimpleNamespace(cfg=cfg, num_envs=PN, device="cpu", flight=flight, episode_length_buf=torch.ones(PN, dtype=torch.int64))
    return env, cfg, lat


def _blocks(counts):
    """Records [PN, 8, 4] with the given counts; block b's frontier voxels all sit at voxel (b, 1, 2) + its block's corner."""
    b = torch.zeros(PN, 8, 4, dtype=torch.int32)
    for e, row in enumerate(counts):
        for k, c in enumerate(row):
            corner = torch.tensor([(k >> 2) * PB, ((k >> 1) & 1) * PB, (k & 1) * PB])
            b[e, k] = torch.cat([torch.tensor([c]), c * (corner + torch.tensor([k % PB, 1, 2]))])
    return b


def _make(counts, node, cost, **kw):
    from gennbv_amd.eval.baselines import FrontierViewPolicy
    env, cfg, lat = _policy_env()
    fb = _Fallback(torch.tensor([[1, 2, 3, 0, 4, 5]] * PN))
    views = _Views(node, cost)
    state = {"blocks": _blocks(counts)}
    pol = FrontierViewPolicy(env, fb, top=3, block=PB, r_min_m=0.5, r_max_m=4.0, frontier=lambda tri: state["blocks"], view_backend=views, **kw)
    obs = torch.zeros(PN, cfg.obs_dim if hasattr(cfg, "obs_dim") else cfg.state_dim + cfg.grid_dim)
    return pol, env, cfg, lat, fb, views, state, obs


COUNTS = [[0, 5, 0, 5, 2, 0, 0, 0],   # ranks: block 1 (5), block 3 (5), block 4 (2)
          [0, 0, 0, 0, 0, 0, 0, 0],   # no frontier
          [9, 0, 0, 0, 0, 0, 1, 0]]   # ranks: block 0 (9), block 6 (1), then an empty rank


def test_policy_needs_a_belief_field():
    from gennbv_amd.eval.baselines import FrontierViewPolicy
    env, _, _ = _policy_env()
    env.flight.belief = False
    with pytest.raises(_lib.GennbvHipError):
        FrontierViewPolicy(env, None, r_min_m=0.5, r_max_m=4.0)
    env.flight = None
    with pytest.raises(_lib.GennbvHipError):
        FrontierViewPolicy(env, None, r_min_m=0.5, r_max_m=4.0)


def test_policy_takes_the_nearest_frontier_at_value_zero_and_weighs_counts_otherwise():
    node = [[100, 200, 300], [7, 7, 7], [400, -1, 500]]
    cost = [[3000, 3000, 1000], [10, 10, 10], [6000, INF, 20]]
    pol, env, cfg, lat, fb, views, state, obs = _make(COUNTS, node, cost)
    assert pol.max_unknown == PB and pol.tried_count.shape == (PN, 8) and bool((pol.tried_count == -1).all())
    act = pol(obs)[0]
    field, vox = views.calls[0]
    assert field is env.flight
    # the targets are the centroid voxels of the ranked blocks, -1 where the rank is empty
    idx, cnt = top_blocks(state["blocks"], 3)
    assert idx[0].tolist() == [1, 3, 4] and idx[2].tolist()[:2] == [0, 6]
    want_vox = block_target_voxels(state["blocks"], idx)
    assert torch.equal(vox, want_vox) and vox[1].tolist() == [[-1] * 3] * 3 and vox[2, 2].tolist() == [-1] * 3
    # env 0: the cheapest node (rank 2, 1000 mm); env 1: no frontier, whatever the backend says; env 2: rank 2 holds no block, so
    # its node does not count, rank 1 has no node: rank 0
    assert pol.fell_back.tolist() == [False, True, False]
    assert pol.last_node.tolist() == [300, -1, 400] and pol.last_cost_mm.tolist() == [1000, INF, 6000] and pol.last_count.tolist() == [2, 0, 9]
    assert torch.equal(act[1], fb.act[1]) and fb.calls == 1
    assert torch.equal(act[[0, 2], :3], node_actions(lat, cfg, torch.tensor([300, 400])))
    assert act[:, 3].tolist() == [0, 0, 0]
    # pitch and yaw look at the block's fp64 centroid from the node
    blk = torch.tensor([[4], [0], [0]])
    cent = block_centroids(state["blocks"], blk, env.flight.range_gt, env.flight.voxel_size)[:, 0]
    pose = S.poses_from_actions(act.double(), cfg)
    fwd = torch.stack([torch.cos(pose[:, 4]) * torch.cos(pose[:, 5]), torch.cos(pose[:, 4]) * torch.sin(pose[:, 5]), -torch.sin(pose[:, 4])], -1)
    off = cent - pose[:, :3]
    cosine = (fwd * off).sum(-1) / off.norm(dim=-1)
    assert bool((cosine[[0, 2]] > 0.95).all())
    low, up = torch.tensor(cfg.clip_pose_idx_low), torch.tensor(cfg.clip_pose_idx_up)
    assert act.dtype == torch.int64 and bool((act >= low).all()) and bool((act <= up).all())
    # with a value per frontier voxel: env 0 scores 5 * 1000 - 3000 = 2000 (rank 0), 2000 (rank 1), 2 * 1000 - 1000 = 1000: a tie,
    # the lowest rank wins; env 2: 9 * 1000 - 6000 = 3000
    pol2 = _make(COUNTS, node, cost, voxel_value_mm=1000)[0]
    pol2(obs)
    assert pol2.last_node.tolist() == [100, -1, 400] and pol2.last_count.tolist() == [5, 0, 9]


def test_policy_does_not_return_to_a_block_it_has_tried_until_its_count_changes_or_the_episode_restarts():
    node = [[100, 200, 300], [7, 7, 7], [400, -1, 500]]
    cost = [[1000, 2000, 3000], [10, 10, 10], [6000, INF, 20]]
    pol, env, cfg, lat, fb, views, state, obs = _make(COUNTS, node, cost)
    pol(obs)
    assert pol.last_node.tolist() == [100, -1, 400]
    tried = pol.tried_count.clone()
    assert tried[0].tolist() == [-1, 5, -1, -1, -1, -1, -1, -1] and tried[1].tolist() == [-1] * 8 and tried[2, 0].item() == 9
    # the same map again: block 1 of env 0 and block 0 of env 2 are no longer eligible; the ranks move up
    pol(obs)
    idx = views.calls[1][1]
    assert torch.equal(idx[0], block_target_voxels(state["blocks"], torch.tensor([[3, 4, 0]] * PN))[0])
    assert idx[0, 2].tolist() == [-1] * 3
    assert pol.last_count.tolist() == [5, 0, 1] and pol.last_node.tolist() == [100, -1, 400]  # (the backend's rank 0 again)
    assert pol.tried_count[0].tolist() == [-1, 5, -1, 5, -1, -1, -1, -1] and pol.tried_count[2].tolist() == [9, -1, -1, -1, -1, -1, 1, -1]
    # env 2 has tried everything: it falls back; env 0 goes on to its last block
    pol(obs)
    assert pol.fell_back.tolist() == [False, True, True] and pol.last_count.tolist() == [2, 0, 0]
    pol(obs)
    assert pol.fell_back.tolist() == [True, True, True]
    # block 1 of env 0 changes its count: eligible again
    counts = [row[:] for row in COUNTS]
    counts[0][1] = 4
    state["blocks"] = _blocks(counts)
    pol(obs)
    assert pol.fell_back.tolist() == [False, True, True] and pol.last_count.tolist() == [4, 0, 0] and pol.tried_count[0, 1].item() == 4
    # a new episode of env 2 forgets what it tried; env 0 keeps its memory
    env.episode_length_buf[2] = 0
    pol(obs)
    assert pol.fell_back.tolist() == [True, True, False] and pol.last_count.tolist() == [0, 0, 9]
    assert pol.tried_count[2].tolist() == [9, -1, -1, -1, -1, -1, -1, -1] and pol.tried_count[0].tolist() == [-1, 4, -1, 5, 2, -1, -1, -1]


def test_policy_falls_back_where_no_target_has_a_node():
    node = [[-1, -1, -1]] * PN
    cost = [[INF] * 3] * PN
    pol, env, cfg, lat, fb, views, state, obs = _make(COUNTS, node, cost)
    act = pol(obs)[0]
    assert pol.fell_back.tolist() == [True] * PN and torch.equal(act, fb.act)
    assert bool((pol.tried_count == -1).all())  # nothing was targeted
    assert pol.policy is pol and torch.equal(pol.predict(obs)[0], fb.act)

"""CPU: the flight lattice (env/flight.py), the Dijkstra oracle of the flight field (tests/flight_oracle.py) against scipy, and
the parts of the feature that need no GPU."""
import math

import numpy as np
import pytest
import torch

from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.flight import INF_MM, FlightLattice, edge_costs, pack_bits
from tests import flight_oracle as FO


def _cfg(up=(8, 6, 4), unit=(0.2, 0.3, 0.25), low=(-1.0, 2.0, 0.1)):
    return TaskConfig(clip_pose_low=list(low) + [0.0, 0.0, 0.0], clip_pose_idx_up=list(up) + [0, 12, 12],
                      action_unit=list(unit) + [0.0, 0.1, 0.1])


def test_default_lattices():
    cfg = TaskConfig()
    two, five = FlightLattice(cfg), FlightLattice(cfg, stride=5)
    assert two.stride == 2 and two.dims == (41, 41, 26) and two.num_nodes == 41 * 41 * 26 and two.words == (two.num_nodes + 31) // 32
    assert five.dims == (17, 17, 11)
    assert np.allclose(two.h, [0.4, 0.4, 0.4]) and np.allclose(two.lo, [-8.0, -8.0, 0.1])
    pos = five.node_positions()
    assert pos.shape == (five.num_nodes, 3)
    # id order: x fastest, then y, then z
    assert np.allclose(pos[1], [-7.0, -8.0, 0.1]) and np.allclose(pos[17], [-8.0, -7.0, 0.1]) and np.allclose(pos[17 * 17], [-8.0, -8.0, 1.1])
    assert np.allclose(pos[-1], [8.0, 8.0, 10.1])
    # every lattice pose is within |h| / 2 of its nearest node
    rs = np.random.RandomState(0)
    a = np.stack([rs.randint(0, u + 1, 500) for u in cfg.clip_pose_idx_up[:3]], -1)
    p = a * np.array(cfg.action_unit[:3]) + np.array(cfg.clip_pose_low[:3])
    for lat in (two, five):
        d = np.linalg.norm(p - lat.node_positions()[lat.nearest_np(p)], axis=1)
        assert d.max() <= 0.5 * lat.h_norm + 1e-12


def test_stride_must_divide_every_position_axis():
    cfg = TaskConfig()  # 80, 80, 50 steps
    for s in (1, 2, 5, 10):
        FlightLattice(cfg, stride=s)
    for s in (3, 4, 8, 20, 0, -1):  # 4 and 8 divide 80 but not 50
        with pytest.raises(ValueError):
            FlightLattice(cfg, stride=s)
    with pytest.raises(ValueError):
        FlightLattice(_cfg(up=(8, 6, 5)), stride=2)
    flat = FlightLattice(_cfg(up=(8, 6, 4), unit=(0.2, 0.3, 0.0)), stride=2)  # an axis that does not move has one node
    assert flat.dims == (5, 4, 1) and flat.h[2] == 0.0


def test_cost_table_for_unequal_spacing():
    lat = FlightLattice(_cfg(), stride=2)
    h = np.array([0.4, 0.6, 0.5])
    assert np.allclose(lat.h, h)
    want = [0, 400, 600, round(1000 * math.hypot(0.4, 0.6)), 500, round(1000 * math.hypot(0.4, 0.5)), round(1000 * math.hypot(0.6, 0.5)),
            round(1000 * math.sqrt(0.16 + 0.36 + 0.25))]
    assert lat.cost.dtype == np.uint32 and lat.cost.tolist() == want
    assert edge_costs([1.0, 1.0, 1.0]).tolist() == [0, 1000, 1000, 1414, 1000, 1414, 1414, 1732]
    assert FO.cost_index(-1, 0, 1) == 5 and FO.cost_index(0, 1, 0) == 2


def test_nearest_node_rule_ties_clamping_and_nan():
    lat = FlightLattice(_cfg(up=(8, 6, 4), unit=(0.25, 0.5, 0.125), low=(0.0, 0.0, 0.0)), stride=2)  # h = 0.5, 1, 0.25: exact in binary
    assert lat.dims == (5, 4, 3)
    nx, ny, nz = lat.dims

    def nid(i, j, k):
        return (k * ny + j) * nx + i
    p = np.array([
        [0.0, 0.0, 0.0],      # a node
        [0.25, 0.5, 0.125],   # ties on every axis go up: floor(x + 0.5)
        [0.2499, 0.4999, 0.1249],
        [-3.0, -0.6, -1e9],   # clamped below
        [99.0, 3.5, 0.51],    # clamped above
        [1.0, 2.0, 0.25],
        [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf],
    ])
    want = [nid(0, 0, 0), nid(1, 1, 1), nid(0, 0, 0), nid(0, 0, 0), nid(4, 3, 2), nid(2, 2, 1), -1, -1, -1]
    assert lat.nearest_np(p).tolist() == want
    assert lat.nearest_np(p.astype(np.float32)[:, None, :]).shape == (9, 1)
    # the torch twin gives the same nodes' positions, NaN where there is none
    pos = lat.nearest_positions(torch.as_tensor(p)).numpy()
    ok = np.array(want) >= 0
    assert np.array_equal(pos[ok], lat.node_positions()[np.array(want)[ok]]) and np.isnan(pos[~ok]).all()


def test_pack_bits_sets_the_padding():
    rs = np.random.RandomState(1)
    b = rs.rand(3, 315) < 0.3
    w = pack_bits(torch.as_tensor(b))
    assert w.dtype == torch.int32 and w.shape == (3, 10)
    assert np.array_equal(FO.unpack_bits(w.numpy(), 315), b)
    tail = w.numpy().view(np.uint32)[:, -1] >> np.uint32(315 - 9 * 32)
    assert (tail == (1 << (320 - 315)) - 1).all()


@pytest.mark.parametrize("dims,frac,seed", [((9, 7, 5), 0.3, 0), ((6, 1, 11), 0.2, 1), ((4, 5, 1), 0.4, 2), ((7, 7, 7), 0.0, 3),
                                            ((5, 6, 4), 0.6, 4)])
def test_heapq_oracle_equals_scipy_on_random_masks(dims, frac, seed):
    rs = np.random.RandomState(seed)
    m = dims[0] * dims[1] * dims[2]
    cost = edge_costs(rs.uniform(0.1, 0.7, 3))
    for trial in range(3):
        blocked = rs.rand(m) < frac
        src = int(rs.randint(m))
        if trial == 0:
            blocked[src] = False
        got, want = FO.dijkstra(blocked, dims, cost, src), FO.scipy_field(blocked, dims, cost, src)
        assert got.dtype == np.uint32 and np.array_equal(got, want)
        assert (got[blocked] == INF_MM).all() and (blocked[src] or got[src] == 0)
        for target in rs.randint(0, m, 4):
            path = FO.walk(got, dims, cost, int(target))
            assert (path == []) == (got[target] == INF_MM)
            if path:
                assert path[0] == target and path[-1] == src and not blocked[path].any()
    assert (FO.dijkstra(np.zeros(m, bool), dims, cost, -1) == INF_MM).all()


def test_serpentine_route_visits_every_open_column():
    dims = (17, 17, 3)
    cost = edge_costs([0.4, 0.4, 0.4])
    blocked = FO.serpentine(dims)
    field = FO.dijkstra(blocked, dims, cost, 0)
    last = 16  # (16, 0, 0)
    path = FO.walk(field, dims, cost, last)
    # 8 walls with gaps at alternating ends: y runs its 16 steps 8 times, and no hop is shorter than 400 mm
    assert len(path) >= 8 * 16 + 1 and field[last] >= 8 * 16 * 400


def test_choose_is_unchanged():
    from gennbv_amd.eval.baselines import choose
    gain = torch.tensor([[[5, 0, 0], [1, 2, 0], [5, 0, 0], [0, 0, 9]],
                         [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]], dtype=torch.int32)
    assert choose(gain, (1, 4)).tolist() == [1, 0]  # 5, 9, 5, 0: the largest; ties to the lowest index
    assert choose(gain, (1, 0)).tolist() == [0, 0]
    contact = torch.tensor([[0, 8, 0, 0], [1, 16, 0, 2]], dtype=torch.uint8)
    assert choose(gain, (1, 4), contact).tolist() == [0, 2]
    assert choose(gain, (1, 4), torch.ones(2, 4, dtype=torch.uint8)).tolist() == [0, 0]  # all refused: the lowest index


def test_flight_ops_refuse_the_cpu():
    from gennbv_amd import _lib
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.ops.flight_field import FlightField
    mesh = MeshScene.from_boxes(S.make_scenes(2, 20, seed=1), device="cpu")
    lat = FlightLattice(TaskConfig(), stride=5)
    with pytest.raises(_lib.GennbvHipError):
        mesh.flight_blocked(lat, CollisionBody(sweep=True))
    with pytest.raises(_lib.GennbvHipError):
        FlightField(mesh, lat, CollisionBody(sweep=True))

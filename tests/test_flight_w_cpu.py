"""CPU: the oracle of the penalised flight field (tests/flight_w_oracle.py) against scipy, every refusal the new entry points make
before a launch (gnbv_flight_field_w, gnbv_flight_path_w, gnbv_flight_classify_tri: they need no GPU), and the argument errors
of BeliefFlightField(unknown="costly") and MapGreedyPolicy(max_cost_m=...)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.flight import INF_MM, FlightLattice, edge_costs
from tests import flight_oracle as FO
from tests import flight_w_oracle as WO

INVALID = 1  # hipErrorInvalidValue
DIMS = (9, 7, 5)
M = 315


def _lattice():
    cfg = TaskConfig(clip_pose_low=[-1.0, 2.0, 0.1, 0.0, 0.0, 0.0], clip_pose_idx_up=[8, 6, 4, 0, 12, 12],
                     action_unit=[0.2, 0.3, 0.25, 0.0, 0.1, 0.1])
    lat = FlightLattice(cfg, stride=1)
    assert lat.dims == DIMS
    return lat


def largest_penalty(m, cost):
    """The largest penalty_mm the bound M * (max cost + penalty) < 0xFFFFFFFE admits."""
    return (INF_MM - 2) // m - int(max(cost))


@pytest.mark.parametrize("penalty", [0, 1, 777, None])
def test_heapq_oracle_equals_scipy_and_the_walk_adds_up(penalty):
    rs = np.random.RandomState(3)
    cost = edge_costs([0.2, 0.3, 0.25])
    if penalty is None:
        penalty = largest_penalty(M, cost)
        assert M * (int(cost.max()) + penalty) < INF_MM - 1 <= M * (int(cost.max()) + penalty + 1)
    for trial in range(3):
        blocked, costly = rs.rand(M) < 0.3, rs.rand(M) < 0.4
        src = int(rs.randint(M))
        if trial < 2:
            blocked[src] = False
        costly[src] = trial == 0  # a costly source pays nothing
        got = WO.dijkstra_w(blocked, costly, DIMS, cost, src, penalty)
        assert got.dtype == np.uint32 and np.array_equal(got, WO.scipy_field_w(blocked, costly, DIMS, cost, src, penalty))
        plain = FO.dijkstra(blocked, DIMS, cost, src)
        assert np.array_equal(got == INF_MM, plain == INF_MM)  # the price moves no node in or out of reach
        assert (got >= plain).all() and (penalty != 0 or np.array_equal(got, plain))
        assert np.array_equal(WO.dijkstra_w(blocked, np.zeros(M, bool), DIMS, cost, src, penalty), plain)
        for target in rs.randint(0, M, 6):
            path = WO.walk_w(got, costly, DIMS, cost, penalty, int(target))
            assert (path == []) == (got[target] == INF_MM)
            if path:
                assert path[0] == target and path[-1] == src and not blocked[path].any() and len(set(path)) == len(path)
                assert WO.route_cost(path, costly, DIMS, cost, penalty) == int(got[target])
    assert (WO.dijkstra_w(np.zeros(M, bool), np.ones(M, bool), DIMS, cost, -1, penalty) == INF_MM).all()


def test_a_costly_corridor_beside_a_free_detour():
    """One z layer, 5 x 3 nodes, unit spacing; row y = 0 is the corridor (x = 1 .. 3 costly), row y = 1 is blocked at x = 1 .. 3,
    row y = 2 is free.  From (0, 0) to (4, 0): through the corridor 4 straight hops and 3 penalties, 4000 + 3 p; round over row 2
    (0,0) -> (0,1) -> (1,2) -> (2,2) -> (3,2) -> (4,1) -> (4,0) = 1000 + 1414 + 1000 + 1000 + 1414 + 1000 = 6828, and every route
    crosses x = 1 .. 3 in row 0 or in row 2.  4000 + 3 p < 6828 up to p = 942 (6826); at p = 943 (6829) the route goes round."""
    dims, cost = (5, 3, 1), edge_costs([1.0, 1.0, 1.0])
    blocked, costly = np.zeros(15, bool), np.zeros(15, bool)
    blocked[[6, 7, 8]] = True
    costly[[1, 2, 3]] = True
    for p, want in ((0, 4000), (942, 6826), (943, 6828), (5000, 6828)):
        field = WO.dijkstra_w(blocked, costly, dims, cost, 0, p)
        assert int(field[4]) == want, (p, int(field[4]))
        path = WO.walk_w(field, costly, dims, cost, p, 4)
        assert (2 in path) == (p <= 942) and WO.route_cost(path, costly, dims, cost, p) == want


# ---------------------------------------------------------------------------
# the C ABI refuses before it launches
# ---------------------------------------------------------------------------
def test_field_w_and_path_w_refusals_at_the_c_abi():
    from gennbv_amd import _lib
    lib = _lib.load()
    assert lib.gnbv_abi_version() == 5
    lat = _lattice()
    cost, lo, h = (C.c_uint32 * 8)(*lat.cost.tolist()), (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)
    zero_cost = (C.c_uint32 * 8)(0, 0, 200, 300, 250, 300, 300, 400)
    bad_h, nan_lo = (C.c_double * 3)(0.2, 0.0, 0.25), (C.c_double * 3)(0.0, math.nan, 0.0)
    fake = 0x1000  # never dereferenced: every call below is refused before a launch
    pmax = largest_penalty(M, lat.cost)
    cmax = int(lat.cost.max())
    assert M * (cmax + pmax) <= INF_MM - 2 < M * (cmax + pmax + 1)

    def field(b=fake, k=fake, pen=5, n=2, nx=9, ny=7, nz=5, c=cost, ps=fake, stride=6, lo_=lo, h_=h, f=fake, s=fake, mode=0):
        return lib.gnbv_flight_field_w(b, k, pen, n, nx, ny, nz, c, ps, stride, lo_, h_, f, s, mode, None)

    def path(f=fake, k=fake, pen=5, n=2, nx=9, ny=7, nz=5, c=cost, lo_=lo, h_=h, t=fake, stride=6, nodes=fake, max_len=4, ln=fake):
        return lib.gnbv_flight_path_w(f, k, pen, n, nx, ny, nz, c, lo_, h_, t, stride, nodes, max_len, ln, None)
    for kw in (dict(b=None), dict(k=None), dict(ps=None), dict(f=None), dict(s=None), dict(c=None), dict(lo_=None), dict(h_=None), dict(n=0),
               dict(nx=0), dict(nz=1025), dict(stride=2), dict(mode=-1), dict(mode=3), dict(c=zero_cost), dict(h_=bad_h), dict(lo_=nan_lo),
               dict(pen=pmax + 1), dict(pen=0xFFFFFFFF),  # the bound, at its edge: pmax itself is accepted (the GPU tests launch it)
               dict(nx=37, ny=37, nz=30, mode=1)):  # 41070 nodes: above gnbv_flight_lds_max_nodes()
        assert field(**kw) == INVALID, kw
    assert 37 * 37 * 30 > int(lib.gnbv_flight_lds_max_nodes())
    for kw in (dict(f=None), dict(k=None), dict(t=None), dict(nodes=None), dict(ln=None), dict(n=0), dict(max_len=0), dict(stride=2),
               dict(c=None), dict(c=zero_cost), dict(h_=bad_h), dict(ny=0), dict(pen=pmax + 1)):
        assert path(**kw) == INVALID, kw
    # one node, no edge: the bound is the penalty's alone, in 64 bits
    one = dict(nx=1, ny=1, nz=1)
    for pen in (0xFFFFFFFE, 0xFFFFFFFF):
        assert field(pen=pen, **one) == INVALID and path(pen=pen, **one) == INVALID
    # two nodes on x: only cost[1] is used
    two = (C.c_uint32 * 8)(0, 1000, 0, 0, 0, 0, 0, 0)
    assert field(nx=2, ny=1, nz=1, c=two, pen=(INF_MM - 1) // 2 - 1000) == INVALID  # 2 * 2147483647 = 0xFFFFFFFE exactly
    huge = (C.c_uint32 * 8)(*([2 ** 31] * 8))
    assert field(c=huge, pen=0) == INVALID  # 315 * 2^31 does not fit 32 bits: the product is taken in 64


def test_classify_refusals_at_the_c_abi():
    from gennbv_amd import _lib
    lib = _lib.load()
    cap = int(lib.gnbv_flightmap_classify_lds_max_grid())
    plane = lambda g: 4 * ((2 * ((g ** 3 + 63) // 64) + 31) // 32 * 32)  # noqa: E731  map_bits.h: whole ballots, whole groups of 32 words
    assert 2 * plane(cap) <= 160 * 1024 < 2 * plane(cap + 1) and cap < int(lib.gnbv_flightmap_lds_max_grid())
    lo, h = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(0.5, 0.5, 0.5)
    fake = 0x1000

    def call(i8=fake, i8_stride=8 ** 3, f32_=None, f32_stride=0, g=8, rng=fake, vox=fake, n=2, nx=9, ny=7, nz=5, lo_=lo, h_=h, rho=0.4,
             out=fake, costly=fake, mode=0):
        return lib.gnbv_flight_classify_tri(i8, i8_stride, f32_, f32_stride, g, rng, vox, n, nx, ny, nz, lo_, h_, rho, 0, 0, out, costly, mode,
                                            None)
    nan_lo, bad_h = (C.c_double * 3)(0.0, math.nan, 0.0), (C.c_double * 3)(0.5, 0.0, 0.5)
    for kw in (dict(g=0), dict(g=129, i8_stride=129 ** 3), dict(rho=0.0), dict(rho=-1.0), dict(rho=math.inf), dict(rho=math.nan),
               dict(nx=0), dict(ny=1025), dict(nz=-1), dict(rng=None), dict(vox=None), dict(out=None), dict(costly=None), dict(lo_=None),
               dict(h_=None), dict(i8=None), dict(f32_=fake, f32_stride=8 ** 3), dict(mode=-1), dict(mode=3), dict(n=0),
               dict(i8_stride=8 ** 3 - 1), dict(i8=None, f32_=fake, f32_stride=8 ** 3 - 1), dict(lo_=nan_lo), dict(h_=bad_h),
               dict(g=cap + 1, i8_stride=(cap + 1) ** 3, mode=1)):
        assert call(**kw) == INVALID, kw


# ---------------------------------------------------------------------------
# the operator and the planner
# ---------------------------------------------------------------------------
def test_the_cautious_field_and_planner_refuse_bad_arguments():
    from gennbv_amd import _lib
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.eval.baselines import MapGreedyPolicy
    from gennbv_amd.ops.flight_field import BeliefFlightField
    lat = FlightLattice(TaskConfig(), stride=5)
    rng, vox = torch.tensor([[8.0, -8.0, 8.0, -8.0, 12.0, 0.0]] * 2), torch.full((2, 3), 0.8)
    body = CollisionBody(sweep=True)
    too_much = (largest_penalty(lat.num_nodes, lat.cost) + 1) / 1000.0
    for kw in (dict(unknown="costly"), dict(unknown="costly", unknown_penalty_m=0.0), dict(unknown="costly", unknown_penalty_m=-1.0),
               dict(unknown="costly", unknown_penalty_m=math.nan), dict(unknown="costly", unknown_penalty_m=math.inf),
               dict(unknown="costly", unknown_penalty_m=too_much), dict(unknown="costly", unknown_penalty_m=1e-4),  # rounds to 0 mm
               dict(unknown="free", unknown_penalty_m=1.0), dict(unknown="blocked", unknown_penalty_m=1.0), dict(unknown="dear")):
        with pytest.raises(ValueError):
            BeliefFlightField(2, lat, body, rng, vox, 20, device="cpu", **kw)
    with pytest.raises(_lib.GennbvHipError):  # well-formed, but there is no CPU fallback
        BeliefFlightField(2, lat, body, rng, vox, 20, device="cpu", unknown="costly", unknown_penalty_m=5.0)
    with pytest.raises(_lib.GennbvHipError):
        BeliefFlightField(2, lat, body, rng, vox, 20, device="cpu", unknown="costly", unknown_penalty_m=too_much - 1e-3)
    env = types.SimpleNamespace(cfg=TaskConfig(), num_envs=2, flight=types.SimpleNamespace(num_envs=2, belief=True), collision=None, device="cpu")
    for bad in (0.0, -2.0, math.nan):
        with pytest.raises(ValueError):
            MapGreedyPolicy(env, k=4, gain_backend=lambda tri, poses: None, max_cost_m=bad)
    assert MapGreedyPolicy(env, k=4, gain_backend=lambda tri, poses: None).max_cost_m is None
    assert MapGreedyPolicy(env, k=4, gain_backend=lambda tri, poses: None, max_cost_m=12.5).max_cost_m == 12.5

"""GPU: unknown space at a price in the flight field -- gnbv_flight_field_w / gnbv_flight_path_w (csrc/flight.hip) at the C ABI
against the Dijkstra oracle with node-entry penalties (tests/flight_w_oracle.py) on every u32, in every mode."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.flight import INF_MM, FlightLattice, pack_bits
from tests import flight_oracle as FO
from tests import flight_w_oracle as WO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
INVALID = 1  # hipErrorInvalidValue
N_ENVS = 6
POISON = 0x5A5A5A5A


def _lattice(dims, unit=(0.2, 0.3, 0.25)):
    cfg = TaskConfig(clip_pose_low=[-1.0, 2.0, 0.1, 0.0, 0.0, 0.0], clip_pose_idx_up=[d - 1 for d in dims] + [0, 12, 12],
                     action_unit=list(unit) + [0.0, 0.1, 0.1])
    lat = FlightLattice(cfg, stride=1)
    assert lat.dims == tuple(dims)
    return lat


def _poses(lat, nodes):
    """fp32 poses [N, 6] a little off the given nodes (so the nearest-node rule has work to do)."""
    p = np.zeros((len(nodes), 6), f32)
    p[:, :3] = lat.node_positions()[nodes] + 0.3 * lat.h * np.array([1, -1, 1])
    return p


def largest_penalty(lat):
    """The largest penalty_mm the bound M * (max cost + penalty) < 0xFFFFFFFE admits."""
    return (INF_MM - 2) // lat.num_nodes - int(lat.cost.max())


def _at_the_edge(lat, penalty):
    """The penalty sits exactly at the edge of the entry point's bound."""
    top = int(lat.cost.max())
    return lat.num_nodes * (top + penalty) < INF_MM - 1 <= lat.num_nodes * (top + penalty + 1)


@functools.lru_cache(maxsize=None)
def _case():
    """9 x 7 x 5 (M = 315: a tail word), six envs, 30 % blocked each: 40 % costly, all costly, none costly, a costly source, a
    blocked source, a NaN pose."""
    lat = _lattice((9, 7, 5))
    m, rs = lat.num_nodes, np.random.RandomState(7)
    blocked = rs.rand(N_ENVS, m) < 0.3
    costly = rs.rand(N_ENVS, m) < 0.4
    costly[1], costly[2] = True, False
    src = np.array([17, 200, 314, 150, 100, 42])
    blocked[np.arange(N_ENVS), src] = False
    costly[[0, 5], src[[0, 5]]] = False
    costly[3, src[3]] = True
    blocked[4, src[4]] = True
    poses = _poses(lat, src)
    poses[5, 1] = np.nan
    assert (blocked & costly).any()  # costly bits on blocked nodes: ignored
    for a in (blocked, costly, src, poses):
        a.setflags(write=False)
    return lat, blocked, costly, src, poses


@functools.lru_cache(maxsize=None)
def _want(penalty):
    """The oracle's table, computed once per penalty and shared by every test."""
    lat, blocked, costly, src, _ = _case()
    w = np.stack([WO.dijkstra_w(blocked[e], costly[e], lat.dims, lat.cost, -1 if e == 5 else int(src[e]), penalty) for e in range(N_ENVS)])
    w.setflags(write=False)
    return w


def _bits(mask, lat):
    """bool [N, M] -> int32 [N, words] on the device, padding bits SET (in `costly` they must not be read)."""
    return pack_bits(torch.tensor(np.asarray(mask)).to(DEV), lat.words)


def _ptrs(lat):
    return (C.c_uint32 * 8)(*lat.cost.tolist()), (C.c_double * 3)(*lat.lo), (C.c_double * 3)(*lat.h)


def _field_w(lat, blocked_t, costly_t, penalty, poses_t, mode, plain=False):
    """gnbv_flight_field_w (plain: gnbv_flight_field) at the C ABI -> (return code, field u32 [N, M], status [N])."""
    from gennbv_amd import _lib
    lib = _lib.load()
    n = blocked_t.shape[0]
    nx, ny, nz = lat.dims
    cost, lo, h = _ptrs(lat)
    field = torch.full((n, lat.num_nodes), POISON, dtype=torch.int32, device=DEV)
    status = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    tail = (n, nx, ny, nz, cost, poses_t.data_ptr(), int(poses_t.stride(0)), lo, h, field.data_ptr(), status.data_ptr(), mode, None)
    if plain:
        err = lib.gnbv_flight_field(blocked_t.data_ptr(), *tail)
    else:
        err = lib.gnbv_flight_field_w(blocked_t.data_ptr(), costly_t.data_ptr(), int(penalty), *tail)
    torch.cuda.synchronize()
    return err, field.cpu().numpy().view(np.uint32), status.cpu().numpy()


def _path_w(lat, field_u32, costly_t, penalty, targets_t, max_len):
    from gennbv_amd import _lib
    lib = _lib.load()
    n = field_u32.shape[0]
    nx, ny, nz = lat.dims
    cost, lo, h = _ptrs(lat)
    field = torch.tensor(field_u32.view(np.int32)).to(DEV)
    nodes = torch.full((n, max_len), -9, dtype=torch.int32, device=DEV)
    count = torch.full((n,), -9, dtype=torch.int32, device=DEV)
    err = lib.gnbv_flight_path_w(field.data_ptr(), costly_t.data_ptr(), int(penalty), n, nx, ny, nz, cost, lo, h, targets_t.data_ptr(),
                                 int(targets_t.stride(0)), nodes.data_ptr(), max_len, count.data_ptr(), None)
    torch.cuda.synchronize()
    return err, nodes.cpu().numpy(), count.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. the field
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 0])
def test_field_w_equals_the_oracle_on_every_u32(mode):
    lat, blocked, costly, src, poses = _case()
    b, k, p = _bits(blocked, lat), _bits(costly, lat), torch.tensor(poses).to(DEV)
    pmax = largest_penalty(lat)
    for penalty in (0, 1, 777, pmax):
        want = _want(penalty)
        err, got, status = _field_w(lat, b, k, penalty, p, mode)
        assert err == 0 and not status.any()
        assert np.array_equal(got, want), (penalty, np.argwhere(got != want)[:5].tolist())
    # the cases reach what they are there for
    w0, w1, wmax = _want(0), _want(777), _want(pmax)
    assert (w1[4] == INF_MM).all() and (w1[5] == INF_MM).all()  # a blocked source, no source
    for e in range(4):
        reached = (w1[e] != INF_MM) & ~blocked[e]
        assert reached.sum() > 100 and w1[e, src[e]] == 0 and (w1[e][blocked[e]] == INF_MM).all()
    assert np.array_equal(w1[2], w0[2]) and (w1[0] > w0[0]).any()  # none costly: the plain field; costly: dearer
    near = [nb for nb, _ in FO.neighbours(int(src[1]), lat.dims) if not blocked[1, nb]]
    assert near and all(w1[1, nb] == w0[1, nb] + 777 for nb in near)  # all costly: one hop is one penalty
    assert (wmax[1][(wmax[1] != INF_MM) & (wmax[1] != 0)] > pmax).all() and _at_the_edge(lat, pmax)  # the largest penalty: nothing wraps
    # a strided pose tensor
    wide = torch.zeros(N_ENVS, 11, device=DEV)
    wide[:, :6] = p
    err, got, _ = _field_w(lat, b, k, 777, wide[:, :6], mode)
    assert err == 0 and np.array_equal(got, w1)


@pytest.mark.parametrize("mode", [1, 2, 0])
def test_no_price_is_the_plain_field_byte_for_byte(mode):
    lat, blocked, costly, src, poses = _case()
    b, k, p = _bits(blocked, lat), _bits(costly, lat), torch.tensor(poses).to(DEV)
    err, plain, plain_status = _field_w(lat, b, None, 0, p, mode, plain=True)
    assert err == 0
    err, free_of_charge, status = _field_w(lat, b, k, 0, p, mode)
    assert err == 0 and free_of_charge.tobytes() == plain.tobytes() and status.tobytes() == plain_status.tobytes()
    none = torch.zeros_like(k)
    err, nothing_costly, status = _field_w(lat, b, none, 777, p, mode)
    assert err == 0 and nothing_costly.tobytes() == plain.tobytes() and status.tobytes() == plain_status.tobytes()
    assert np.array_equal(plain, _want(0))


@pytest.mark.parametrize("mode", [1, 2])
def test_the_route_leaves_the_costly_corridor_at_the_penalty_worked_out_by_hand(mode):
    """tests/test_flight_w_cpu.py has the arithmetic: 5 x 3 x 1, unit spacing, row 0 a costly corridor (x = 1 .. 3), row 1 blocked
    there, row 2 free.  Through: 4000 + 3 p.  Round: 6828.  p = 942 goes through (6826), p = 943 goes round."""
    lat = _lattice((5, 3, 1), unit=(1.0, 1.0, 1.0))
    assert lat.cost.tolist()[:4] == [0, 1000, 1000, 1414]
    blocked, costly = np.zeros((1, 15), bool), np.zeros((1, 15), bool)
    blocked[0, [6, 7, 8]] = True
    costly[0, [1, 2, 3]] = True
    b, k = _bits(blocked, lat), _bits(costly, lat)
    pose, target = torch.as_tensor(_poses(lat, [0])).to(DEV), torch.as_tensor(_poses(lat, [4])).to(DEV)
    for penalty, want, through in ((0, 4000, True), (942, 6826, True), (943, 6828, False), (5000, 6828, False)):
        err, field, _ = _field_w(lat, b, k, penalty, pose, mode)
        assert err == 0 and int(field[0, 4]) == want, (penalty, int(field[0, 4]))
        assert np.array_equal(field[0], WO.dijkstra_w(blocked[0], costly[0], lat.dims, lat.cost, 0, penalty))
        err, nodes, count = _path_w(lat, field, k, penalty, target, 16)
        path = nodes[0, :count[0]].tolist()
        assert err == 0 and path == ([4, 3, 2, 1, 0] if through else [4, 9, 13, 12, 11, 5, 0])


def test_above_the_lds_threshold_the_table_lives_in_global_memory():
    from gennbv_amd import _lib
    cap = int(_lib.load().gnbv_flight_lds_max_nodes())
    nx = ny = 36
    nz = cap // (nx * ny) + 1
    lat = _lattice((nx, ny, nz), unit=(0.2, 0.2, 0.2))
    m = lat.num_nodes
    assert cap < m <= cap + nx * ny
    rs = np.random.RandomState(9)
    blocked, costly = rs.rand(1, m) < 0.3, rs.rand(1, m) < 0.4
    src = int(np.nonzero(~blocked[0])[0][m // 3])
    want = WO.dijkstra_w(blocked[0], costly[0], lat.dims, lat.cost, src, 777)
    assert (want != INF_MM).sum() > m // 2
    b, k, p = _bits(blocked, lat), _bits(costly, lat), torch.as_tensor(_poses(lat, [src])).to(DEV)
    for mode in (2, 0):
        err, got, status = _field_w(lat, b, k, 777, p, mode)
        assert err == 0 and not status.any() and np.array_equal(got[0], want), mode
    err, got, status = _field_w(lat, b, k, 777, p, 1)
    assert err == INVALID and (got == POISON).all() and (status == -7).all()  # refused before anything was launched


# ---------------------------------------------------------------------------
# 2. the walk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("penalty", [777, 0, None])
def test_walk_w_equals_the_oracles_walk(penalty):
    lat, blocked, costly, src, poses = _case()
    penalty = largest_penalty(lat) if penalty is None else penalty
    field = _want(penalty)
    k = _bits(costly, lat)
    rs = np.random.RandomState(4)
    walked = longest = 0
    for trial in range(4):
        tnode = rs.randint(0, lat.num_nodes, N_ENVS)
        if trial == 0:
            tnode = src.copy()  # target and source share a node: one node
        if trial >= 2:  # nodes a route reaches (trial 1: whatever comes, blocked and cut-off nodes included)
            for e in range(4):
                tnode[e] = rs.choice(np.nonzero(field[e] != INF_MM)[0])
        t = _poses(lat, tnode)
        if trial == 1:
            t[2, 0] = np.nan  # no node
        err, nodes, count = _path_w(lat, field, k, penalty, torch.as_tensor(t).to(DEV), 64)
        assert err == 0
        for e in range(N_ENVS):
            want = WO.walk_w(field[e], costly[e], lat.dims, lat.cost, penalty, -1 if (trial == 1 and e == 2) else int(tnode[e]))
            got = nodes[e, :max(count[e], 0)].tolist()
            assert count[e] == len(want) and got == want, (trial, e, got, want)
            if want:
                assert want[0] == tnode[e] and want[-1] == src[e] and not blocked[e][want].any()
                # consecutive nodes are 26-adjacent (route_cost looks every hop up among the neighbours), and the edge costs plus
                # the penalties of the nodes entered add up to the field at the target
                assert WO.route_cost(want, costly[e], lat.dims, lat.cost, penalty) == int(field[e, tnode[e]])
                walked += 1
                longest = max(longest, len(want))
            if trial == 0 and e < 4:
                assert want == [int(src[e])]
    assert walked >= 12 and longest >= 4
    # a short buffer: -needed, the first max_len nodes written
    tnode = np.array([int(np.argmax(np.where(field[e] == INF_MM, 0, field[e]))) for e in range(N_ENVS)])  # the dearest node of each env
    t = torch.as_tensor(_poses(lat, tnode)).to(DEV)
    _, full, need = _path_w(lat, field, k, penalty, t, 64)
    assert need[:4].min() >= 3 and (need[4:] == 0).all()
    err, short, count = _path_w(lat, field, k, penalty, t, 2)
    assert err == 0 and (count[:4] == -need[:4]).all() and (count[4:] == 0).all()
    assert np.array_equal(short[:4], full[:4, :2])

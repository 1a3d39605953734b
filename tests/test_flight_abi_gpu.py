"""GPU: the six entry points of csrc/flight.hip at the C ABI in every launch regime -- gnbv_flight_field / _w with one, two, 33, 40
and 41 nodes per lane, the table in LDS and in global memory, a second chunk of one node, axes of one node, lines that need every
sweep the cap allows, sums at the edge of 32 bits and both orders of raising the LDS limit; gnbv_flight_query past one block, at
three row strides, outside the lattice, on non-finite coordinates and exactly half-way between nodes; gnbv_flight_path / _w past
one block with buffers of exactly the longest route, one short of it and one node.  Outputs are poisoned first, every word is
compared and the guard words after every output must still hold the poison; every comparison with the heapq oracles
(tests/flight_oracle.py, tests/flight_w_oracle.py) is exact.  tests/flight_abi_util.py has the cases;
tests/test_flight_abi_regimes_cpu.py shows, without a GPU, that each reaches the regime its id names and would catch the slips it
is there for."""
import functools
import shutil

import numpy as np
import pytest

from tests import flight_abi_util as U
from tests import flight_oracle as FO

pytestmark = pytest.mark.gpu
INF = U.INF


@functools.lru_cache(maxsize=4)
def _field_inputs(cid):
    """A field case on the device: blocked and costly words (padding bits set), poses."""
    s = U.field_case(cid)
    return U.to_dev(U.pack_words(s.blocked)), U.to_dev(U.pack_words(s.costly)), U.to_dev(s.poses)


def _run_field(cid, weighted, mode, lib=None):
    s = U.field_case(cid)
    b, k, p = _field_inputs(cid)
    if weighted:
        return U.call_field(s.lat, b, p, mode, costly_t=k, penalty=s.penalty, lib=lib)
    return U.call_field(s.plain_lat, b, p, mode, lib=lib)


def _untouched(field, status):
    return bool((field == U.POISON).all() and (status == U.STATUS_POISON).all())


# ---------------------------------------------------------------------------
# 1. the field
# ---------------------------------------------------------------------------
def test_capacity_first_then_a_small_lattice_in_a_fresh_image_of_the_library(tmp_path):
    """launch_field raises the kernel's dynamic-LDS limit once per instantiation, the first time a launch asks for more than
    64 KiB.  Elsewhere a small lattice always comes first; here, in a second image of the library whose counters are untouched,
    the first launch of each LDS instantiation is the one at capacity, and a small one follows."""
    from gennbv_amd import _lib
    copy = tmp_path / "libgennbv_hip_fresh.so"
    shutil.copyfile(_lib.LIB_PATH, copy)
    fresh = _lib._open(str(copy))
    assert fresh is not _lib.load() and int(fresh.gnbv_flight_lds_max_nodes()) == U.lds_max_nodes()
    big = "pl40-capacity-36x36x31"
    assert U.field_regime(U.FIELD_CASES[big]["dims"], 1).needs_attribute and not U.field_regime(U.SMALL_DIMS, 1).needs_attribute
    s = U.small_sets()
    b, k, p = U.to_dev(U.pack_words(s.blocked)), U.to_dev(U.pack_words(s.costly)), U.to_dev(s.poses)
    for weighted in (False, True):
        err, got, status, guard_ok = _run_field(big, weighted, 1, lib=fresh)
        assert err == 0 and guard_ok and not status.any(), weighted
        assert np.array_equal(got, U.field_want(big, weighted)), weighted
        err, got, status, guard_ok = U.call_field(s.lat, b, p, 1, costly_t=k if weighted else None, penalty=U.PENALTY, lib=fresh)
        assert err == 0 and guard_ok and not status.any(), weighted
        assert np.array_equal(got, U.small_want(U.PENALTY if weighted else None)), weighted


@pytest.mark.parametrize("cid", list(U.FIELD_CASES))
def test_field_equals_the_oracle_in_every_regime(cid):
    s = U.field_case(cid)
    dims = s.lat.dims
    assert int(U.load_lib().gnbv_flight_lds_max_nodes()) == U.lds_max_nodes()
    modes = U.accepted_modes(dims)
    for weighted in (False, True):
        want = U.field_want(cid, weighted)
        for mode in modes:
            assert U.field_regime(dims, mode).lds == (mode == 1 or (mode == 0 and 1 in modes))
            err, got, status, guard_ok = _run_field(cid, weighted, mode)
            what = (weighted, mode)
            assert err == 0 and guard_ok, what
            print("field", cid, what, "status", status.tolist(), "differ", int((got != want).sum()))
            assert not status.any(), what  # (the lines: the table settles on the very sweep the cap still admits)
            assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())
        if 1 not in modes:  # refused before anything is launched
            err, got, status, guard_ok = _run_field(cid, weighted, 1)
            assert err == U.INVALID and guard_ok and _untouched(got, status), weighted
    if cid.startswith("bound"):  # one more millimetre on the penalty, or on the plain call's largest cost, and the host says no
        b, k, p = _field_inputs(cid)
        err, got, status, guard_ok = U.call_field(s.lat, b, p, 0, costly_t=k, penalty=s.penalty + 1)
        assert err == U.INVALID and guard_ok and _untouched(got, status)
        dearer = U.lattice(dims, cost=[int(c) + (int(c) == int(s.plain_lat.cost.max())) for c in s.plain_lat.cost])
        err, got, status, guard_ok = U.call_field(dearer, b, p, 0)
        assert err == U.INVALID and guard_ok and _untouched(got, status)


def test_a_source_pose_half_way_between_nodes_starts_at_the_higher_node():
    lat, t, want = U.tie_targets()
    m = lat.num_nodes
    blocked = np.zeros((len(t), m), bool)
    poses = np.zeros((len(t), 6), np.float32)
    poses[:, :3] = t
    err, got, status, guard_ok = U.call_field(lat, U.to_dev(U.pack_words(blocked)), U.to_dev(poses), 0)
    assert err == 0 and guard_ok and not status.any()
    assert np.array_equal(np.argmin(got, 1), want) and (got[np.arange(len(t)), want] == 0).all()
    for e in (0, len(t) - 1):
        assert np.array_equal(got[e], FO.dijkstra(blocked[e], lat.dims, lat.cost, int(want[e])))


# ---------------------------------------------------------------------------
# 2. the query
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_fields(n, penalty):
    """The kernel's own fields of n envs cycling through the seven small sets (checked against the oracle), on the device."""
    s = U.small_sets()
    sets = U.cycle(n)
    b, p = U.to_dev(U.pack_words(s.blocked[sets])), U.to_dev(s.poses[sets])
    k = None if penalty is None else U.to_dev(U.pack_words(s.costly[sets]))
    err, got, status, guard_ok = U.call_field(s.lat, b, p, 0, costly_t=k, penalty=penalty or 0)
    assert err == 0 and guard_ok and not status.any()
    assert np.array_equal(got, U.small_want(penalty)[sets])
    return U.to_dev(got), k


def _rows(targets, stride):
    """f32 [T, 3] -> a device buffer of T rows of `stride` floats; what lies between the rows' coordinates is NaN."""
    wide = np.full((len(targets), stride), np.nan, np.float32)
    wide[:, :3] = targets
    return U.to_dev(wide)


@pytest.mark.parametrize("n,k", U.QUERY_SHAPES)
def test_query_equals_the_table_lookup_in_every_launch_shape(n, k):
    lat = U.small_sets().lat
    field_t, _ = _small_fields(n, None)
    t, _ = U.query_targets(n, k)
    want = U.query_want(U.small_want(None)[U.cycle(n)], lat, t, k)
    for stride in U.QUERY_STRIDES:
        err, got, guard_ok = U.call_query(lat, field_t, _rows(t, stride), n, k, stride)
        assert err == 0 and guard_ok, stride
        assert np.array_equal(got, want), (stride, np.argwhere(got != want)[:5].tolist())


def test_query_half_way_between_two_nodes_reads_the_higher_one():
    lat, t, want = U.tie_targets()
    table = np.arange(lat.num_nodes, dtype=np.uint32)[None]  # any table in the field's layout: the node read is the value read
    err, got, guard_ok = U.call_query(lat, U.to_dev(table), _rows(t, 3), 1, len(t), 3)
    assert err == 0 and guard_ok and np.array_equal(got, want.astype(np.uint32)), (got.tolist(), want.tolist())


def test_query_on_an_axis_of_one_node_ignores_that_coordinate():
    lat = U.lattice((1, 33, 31))
    m, n, k = lat.num_nodes, 2, 40
    table = np.arange(n * m, dtype=np.uint32).reshape(n, m)
    rs = np.random.RandomState(3)
    span = lat.h * (np.array(lat.dims) - 1)
    t = (lat.lo + span * rs.uniform(-0.1, 1.1, (n * k, 3))).astype(np.float32)
    t[0::4, 0], t[1::4, 0], t[2::4, 0] = 1e6, -1e6, 3.0e38  # finite, however far: node 0 of that axis
    t[3, 0], t[7, 0], t[11, 0] = np.nan, np.inf, -np.inf     # non-finite: no node
    want = U.query_want(table, lat, t, k)
    assert (want[[3, 7, 11]] == INF).all() and (want != INF).sum() == n * k - 3 and len(set(want.tolist())) > n * k // 2
    err, got, guard_ok = U.call_query(lat, U.to_dev(table), _rows(t, 6), n, k, 6)
    assert err == 0 and guard_ok and np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


# ---------------------------------------------------------------------------
# 3. the walk
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("penalty", U.PATH_PENALTIES)
@pytest.mark.parametrize("n", U.PATH_NS)
def test_walks_equal_the_oracles_and_never_leave_their_row(n, penalty):
    lat = U.small_sets().lat
    c = U.path_case(n, penalty)
    field_t, costly_t = _small_fields(n, penalty)
    targets_t = U.to_dev(c.targets)
    assert U.path_blocks(n) == {64: 1, 65: 2, 130: 3}[n]
    for max_len in (c.longest, c.longest - 1, 1):
        want_nodes, want_count = U.path_rows(c, max_len)
        err, nodes, count, guard_ok = U.call_path(lat, field_t, targets_t, max_len, costly_t=costly_t, penalty=penalty or 0)
        assert err == 0 and guard_ok, max_len
        assert np.array_equal(count, want_count), (max_len, np.argwhere(count != want_count)[:5].tolist())
        # the first min(len, max_len) nodes of a routed row; the poison everywhere else, rows of unroutable envs included
        assert np.array_equal(nodes, want_nodes), (max_len, np.argwhere(nodes != want_nodes)[:5].tolist())

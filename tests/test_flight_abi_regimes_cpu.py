"""CPU: every case of tests/test_flight_abi_gpu.py reaches the regime of csrc/flight.hip its id names, and a kernel that is subtly
wrong in the ways these cases exist for would not pass them.  The launch shape is restated in tests/flight_abi_util.py and
evaluated from the numbers alone; the rest comes from the heapq oracles.  No GPU is involved, so a case that has gone vacuous shows
up wherever the suite runs.  These are conditions, not measurements."""
import numpy as np
import pytest

from tests import flight_abi_util as U
from tests import flight_oracle as FO
from tests import flight_w_oracle as WO

INF = U.INF
WEIGHTED_BIG = ("pl33-lds-36x36x26", "pl40-capacity-36x36x31")  # bits 32 .. 39 of `mine` carry the price


# ---------------------------------------------------------------------------
# 1. every case id reaches its regime; the table reaches every regime
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(U.FIELD_CASES))
def test_field_case_reaches_its_regime(cid):
    print("field", cid, U.check_field_case(cid))


def test_the_field_cases_cover_every_regime_once_at_least():
    old = U.field_regime(U.SMALL_DIMS, 1)  # what the kernel-level tests run: one node per lane, one bit of `mine`
    assert old.per_lane == 1 and old.mine_bits == 1 and not old.needs_attribute and old.tail_word and old.unit_axes == ()
    assert U.field_regime((17, 17, 11), 1).per_lane == 4  # the closed-loop env test
    info = {cid: U.check_field_case(cid) for cid in U.FIELD_CASES}
    per_lane = {i["per_lane"] for i in info.values()}
    assert {1, 2, 33, 40} <= per_lane and max(per_lane) == 41  # 41: only ever in global memory
    assert any(i["last_chunk_nodes"] == 1 for i in info.values()) and any(i["last_chunk_nodes"] == U.K_FIELD_LANES for i in info.values())
    axes = {i["unit_axes"] for i in info.values()}
    assert {(0,), (1,), (2,), (1, 2), ()} <= axes
    assert any(i["tail_word"] for i in info.values()) and any(not i["tail_word"] for i in info.values())
    assert any(i["modes"] == (2, 0) for i in info.values()) and any(i["modes"] == (1, 2, 0) for i in info.values())
    assert any(i["lds_bytes"] > U.K_LDS_DEFAULT for i in info.values()) and any(16 < i["lds_bytes"] <= U.K_LDS_DEFAULT for i in info.values())
    assert sum(cid.startswith("bound") for cid in info) == 2 and sum(cid.startswith("line") for cid in info) == 3


def test_thresholds_and_worked_examples():
    assert U.lds_max_nodes() == 40956 and U._bound_sum(64) == 67108863 and 64 * 67108863 == 0xFFFFFFC0
    assert U.field_regime((36, 36, 31), 0).lds and not U.field_regime((36, 36, 32), 0).lds and U.field_regime((36, 36, 32), 1).refused
    assert U.field_regime((36, 36, 31), 1).lds_bytes == 16 + 4 * 40176 <= U.K_LDS_BYTES
    assert [U.field_regime((n, 1, 1), 2).per_lane for n in (1, 1024)] == [1, 1] and U.field_regime((41, 25, 1), 2).per_lane == 2
    assert not U.field_regime((1023, 16, 1), 1).needs_attribute and U.field_regime((1024, 16, 1), 1).needs_attribute  # 64 KiB with the header
    assert [U.path_blocks(n) for n in (7,) + U.PATH_NS] == [1, 1, 2, 3]
    assert [n * k for n, k in U.QUERY_SHAPES] == [1, 256, 257, 513]
    assert [U.query_blocks(n, k) for n, k in ((7, 9),) + U.QUERY_SHAPES] == [1, 1, 1, 2, 3]
    # the last block of each launch has lanes past the end: the guards `e >= n` and `item >= n * k` run
    assert 65 % U.K_WAVE == 1 and 130 % U.K_WAVE == 2 and 257 % U.K_QUERY_LANES == 1 and 513 % U.K_QUERY_LANES == 1


# ---------------------------------------------------------------------------
# 2. the oracle-side conditions of the field cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(U.FIELD_CASES))
def test_field_case_is_reached_priced_and_tells_the_mutants_apart(cid):
    s = U.field_case(cid)
    m = s.lat.num_nodes
    plain, priced = U.field_want(cid, False), U.field_want(cid, True)
    seen = set()
    for e in range(s.n):
        assert not s.blocked[e, s.src[e]] and plain[e, s.src[e]] == 0 == priced[e, s.src[e]]
        reached = priced[e] != INF
        assert np.array_equal(reached, plain[e] != INF) and reached.sum() > m // 2, (e, int(reached.sum()), m)
        assert (priced[e][reached] < U.K_FREE - 1).all()
        if cid in WEIGHTED_BIG:
            high = int((reached & s.costly[e])[32 * U.K_FIELD_LANES:].sum())
            print("costly reached nodes >= 32768", cid, e, high)
            assert high >= 100
        for name, field in U.mutant_fields(cid, e).items():
            differ = int((field != priced[e]).sum())
            print("mutant", cid, e, name, differ)
            assert differ > 0, (e, name)
            seen.add(name)
    want = {"penalty-on-the-node-left"} | ({"chunk-mix-up"} if m > U.K_FIELD_LANES else set()) | ({"32-bit-mine"} if cid in WEIGHTED_BIG else set())
    assert want <= seen
    if not cid.startswith("bound"):
        assert (priced >= plain).all() and (priced[plain != INF] > plain[plain != INF]).any()  # the price is paid somewhere


def test_the_mutants_are_what_they_say():
    s = U.field_case("pl40-capacity-36x36x31")
    c = s.costly[0]
    m = c.shape[0]
    lost = U.clear_high_bits(c)
    assert np.array_equal(lost[:32768], c[:32768]) and not lost[32768:].any() and c[32768:].sum() > 1000
    sw = U.swap_chunks(c)
    assert sw[5] == c[39 * 1024 + 5] and sw[39 * 1024 + 5] == c[5] and sw[3 * 1024 + 77] == c[36 * 1024 + 77]
    assert not sw[1000] and 39 * 1024 + 1000 >= m  # the node it would be taken from does not exist
    assert np.array_equal(U.swap_chunks(s.costly[0][:1024]), s.costly[0][:1024])  # one chunk: nothing to mix up
    # the leaving mutant on three nodes in a row, by hand: 0 -> 1 -> 2, node 1 costly
    kw = dict(dims=(3, 1, 1), cost=[0, 10, 0, 0, 0, 0, 0, 0], src=0, penalty=5)
    none, mid = np.zeros(3, bool), np.array([False, True, False])
    assert WO.dijkstra_w(none, mid, **kw).tolist() == [0, 15, 25] and U.dijkstra_leaving(none, mid, **kw).tolist() == [0, 10, 25]
    # with no price it is the oracle
    small = U.small_sets()
    assert np.array_equal(U.dijkstra_leaving(small.blocked[1], small.costly[1], small.lat.dims, small.lat.cost, 200, 0), U.small_want(0)[1])


# ---------------------------------------------------------------------------
# 3. the sweep cap is tight on a line
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["line-2-cap", "line-64-cap", "bound-line-64"])
def test_a_line_in_one_wave_needs_exactly_m_sweeps(cid):
    """m - 1 sweeps that each reach one more node, and the sweep that finds nothing to do: the loop's `sweep < m` admits exactly
    that many, so status 0 and an exact field are due; a cap one lower would leave with `more` set and report 1."""
    s = U.field_case(cid)
    m = s.lat.num_nodes
    for weighted in (False, True):
        lat = s.lat if weighted else s.plain_lat
        want = U.field_want(cid, weighted)
        for e in range(s.n):
            sweeps, table = U.line_sweeps(m, int(s.src[e]), int(lat.cost[1]), s.costly[e] if weighted else np.zeros(m, bool), s.penalty)
            assert sweeps == m and np.array_equal(table, want[e]), (weighted, e, sweeps)
            assert int(want[e].max()) == int(want[e][m - 1 - s.src[e]]) and (want[e] != INF).all()  # the other end is the farthest


def test_the_line_of_1024_stays_far_below_the_cap():
    s = U.field_case("line-1024-mid")
    want = U.field_want("line-1024-mid", True)
    hops = np.abs(np.arange(1024) - int(s.src[0]))
    assert (want != INF).all() and hops.max() + 1 <= 1024 // 2 + 1  # Jacobi at the worst: 513 sweeps
    assert np.array_equal(U.field_want("line-1024-mid", False)[0], (hops * int(s.plain_lat.cost[1])).astype(np.uint32))


# ---------------------------------------------------------------------------
# 4. sums at the overflow bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["bound-line-64", "bound-4x4x4"])
def test_bound_cases_sit_at_the_edge_of_32_bits(cid):
    s = U.field_case(cid)
    for weighted in (False, True):
        lat, pen = (s.lat, s.penalty) if weighted else (s.plain_lat, 0)
        assert U.cost_sum_at_the_bound(lat, pen)
        want = U.field_want(cid, weighted)  # (dijkstra_w asserts that every route stays below 0xFFFFFFFE)
        top = max(U.largest_candidate(lat, want[e], s.blocked[e], pen) for e in range(s.n))
        print("largest candidate", cid, weighted, hex(top))
        assert top < U.K_FREE
        if "line" in cid:  # the farthest node's own value added to one more hop: 64 hops' worth, 62 below kFree
            assert top == 64 * U._bound_sum(64) == U.K_FREE - 62 and int(want.max()) == 63 * U._bound_sum(64) > 2 ** 31
    if "4x4x4" in cid:
        used = {ci for _, ci in FO.neighbours(21, s.lat.dims)}
        assert used == set(range(1, 8)) and len(set(s.lat.cost[1:].tolist())) == 7  # every cost index occurs, each with its own value


# ---------------------------------------------------------------------------
# 5. query and path cases
# ---------------------------------------------------------------------------
def test_small_sets_keep_the_character_of_the_older_case():
    s = U.small_sets()
    for penalty in U.PATH_PENALTIES:
        w = U.small_want(penalty)
        assert (w[4] == INF).all() and (w[5] == INF).all() and (w[6] == INF).all()
        assert all(((w[e] != INF) & ~s.blocked[e]).sum() > 30 for e in range(4))
        assert not s.blocked[U.SEALED_SET, U.SEALED_NODE] and w[U.SEALED_SET, U.SEALED_NODE] == INF
    assert np.array_equal(U.small_want(0), U.small_want(None)) and (U.small_want(777) > U.small_want(None)).any()
    assert (U.cycle(130)[1:] != U.cycle(130)[:-1]).all() and set(U.cycle(64).tolist()) == set(range(U.D))


@pytest.mark.parametrize("n,k", U.QUERY_SHAPES)
def test_query_targets_hold_every_kind_the_shape_has_room_for(n, k):
    t, kind = U.query_targets(n, k)
    lat = U.lattice(U.SMALL_DIMS)
    node = U.nearest(lat, t)
    assert t.dtype == np.float32 and t.shape == (n * k, 3)
    assert ((node < 0) == ~np.isfinite(t).all(1)).all()
    if n * k >= 32:
        idx = U.node_index(lat)
        top = np.array(lat.dims) - 1
        for side in range(6):  # outside on every side: clamped to that face
            rows = np.nonzero(kind == side)[0]
            a = side // 2
            assert len(rows) and (idx[node[rows], a] == (0 if side % 2 == 0 else top[a])).all()
        for a in range(3):
            col = t[(kind >= 6) & (kind < 15), a]
            assert np.isnan(col).any() and np.isposinf(col).any() and np.isneginf(col).any()
        assert (node >= 0).sum() > n * k // 2
        field = U.small_want(None)[U.cycle(n)]
        want = U.query_want(field, lat, t, k)
        assert (want == INF).any() and (want != INF).any() and (want[node < 0] == INF).all()
    else:
        assert kind[0] == 0 and node[0] >= 0  # the one item: outside, clamped


def test_half_way_targets_go_to_the_higher_node_as_nearest_np_says():
    from gennbv_amd.env.flight import FlightLattice
    lat, t, want = U.tie_targets()
    assert len(t) == sum(d - 1 for d in U.SMALL_DIMS) + 1
    assert np.array_equal(U.nearest(lat, t), want)
    assert np.array_equal(FlightLattice.nearest_np(lat, t), want)  # (the method reads dims, lo and h alone)
    x = (t.astype(np.float64) - lat.lo) / lat.h + 0.5
    assert ((x == np.floor(x)).sum(1) >= 1).all() and (x[-1] == 1.0).all()  # exactly on the rounding edge, in fp64
    # the restated rule is the package's on ordinary targets too, non-finite ones and an axis of one node included
    q, _ = U.query_targets(3, 171)
    small = U.lattice(U.SMALL_DIMS)
    assert np.array_equal(U.nearest(small, q), FlightLattice.nearest_np(small, q))
    flat = U.lattice((1, 33, 31))
    far = q.copy()
    far[:, 0] = 1e6
    assert np.array_equal(U.nearest(flat, far), FlightLattice.nearest_np(flat, far)) and (U.nearest(flat, far)[np.isfinite(far).all(1)] >= 0).all()


@pytest.mark.parametrize("penalty", U.PATH_PENALTIES)
@pytest.mark.parametrize("n", U.PATH_NS)
def test_path_cases_have_routes_of_several_lengths_and_rows_that_stay_untouched(n, penalty):
    c = U.path_case(n, penalty)
    s = U.small_sets()
    lens = np.array([len(w) for w in c.walks])
    assert c.longest >= 6 and (lens == c.longest).any() and ((lens > 1) & (lens < c.longest)).any() and (lens == 0).sum() >= n // 2
    assert {"farthest", "blocked", "cut-off", "nan"} == set(c.kinds)
    assert all((lens[e] > 0) == (c.kinds[e] == "farthest" and c.sets[e] < 4) for e in range(n))
    # past the first block there are routed envs (n = 65: the one env there, its row followed by the guard alone) and unrouted ones
    if n > U.K_WAVE:
        assert (lens[U.K_WAVE:] > 0).any() and (n == U.K_WAVE + 1 or (lens[U.K_WAVE:] == 0).any())
    # a routed row has an unroutable row after it: what spills out of it lands on the poison, not on a neighbour's own stores
    routed = np.nonzero(lens > 0)[0]
    assert all(e + 1 >= n or lens[e + 1] == 0 for e in routed)
    for max_len, some_negative in ((c.longest, False), (c.longest - 1, True), (1, True)):
        nodes, count = U.path_rows(c, max_len)
        assert ((count < 0).any() == some_negative) and (count[lens == 0] == 0).all()
        if max_len == c.longest - 1:
            assert np.array_equal(count < 0, lens == c.longest)
        assert (nodes[lens == 0].view(np.uint32) == U.POISON).all()
    for e in routed[:8]:
        w, d = c.walks[e], c.sets[e]
        assert w[0] == c.tnode[e] and w[-1] == s.src[d] and not s.blocked[d][w].any()
        if penalty is not None:
            assert WO.route_cost(w, s.costly[d], s.lat.dims, s.lat.cost, penalty) == int(U.small_want(penalty)[d, c.tnode[e]])

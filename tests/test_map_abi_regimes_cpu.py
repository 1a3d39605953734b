"""CPU: every case of tests/test_map_abi_gpu.py reaches the regime of csrc/flightmap.hip, csrc/sweepmap.hip or csrc/frontview.hip
its id names.  The host launch shapes and the LDS pack of csrc/map_bits.h are restated in tests/map_abi_util.py and evaluated from
(n, M or K or T, mode, G, chunk) and the numpy oracles' results; no GPU is involved, so a case that has gone vacuous shows up
wherever the suite runs."""
import numpy as np
import pytest

from tests import map_abi_util as U
from tests import sweepmap_oracle as SO


# ---------------------------------------------------------------------------
# 1. every case id reaches its regime
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(U.NODE_CASES))
def test_node_case_reaches_its_regime(cid):
    print("node", cid, U.check_node_case(cid))


@pytest.mark.parametrize("cid", sorted(U.SWEEP_CASES))
def test_sweep_case_reaches_its_regime(cid):
    print("sweep", cid, U.check_sweep_case(cid))


@pytest.mark.parametrize("cid", sorted(U.VIEW_CASES))
def test_viewpoint_case_reaches_its_regime(cid):
    print("viewpoints", cid, U.check_view_case(cid))


def test_the_case_tables_cover_every_regime_once_at_least():
    """What the kernel-level tests of the node kernels run (n = 6, M = 315) against what the tables add."""
    old = U.node_shape(6, 315, 1, 12)
    assert old.chunks == 1 and old.turns == 1 and not old.cap_binds and old.dead_groups == 0
    old = U.sweep_shape(6, 40, 1, 12)
    assert old.chunk_items == U.K_WAVES and old.turns == 1 and old.last_items == U.K_WAVES and not old.cap_binds
    assert U.view_shape(5, 9, 1, 33, 0, 210).turns == 1
    shapes = [U.node_shape(c["n"], int(np.prod(c["dims"])), c["mode"], g) for c in U.NODE_CASES.values() for g in c["gs"]]
    assert any(s.chunks > 1 for s in shapes) and any(s.turns > 1 for s in shapes) and any(s.cap_binds for s in shapes)
    assert any(s.dead_groups for s in shapes) and any(s.words % 2 for s in shapes) and any(s.cap == 1 for s in shapes if s.lds)
    assert {s.shift for s in shapes if s.lds} == {5, 6, 7, 8}
    assert {U.map_swizzle_shift(c["g"]) for c in U.VIEW_CASES.values() if any(mode == 1 for mode, _ in c["runs"])} == {5, 6, 7, 8}
    assert {U.map_swizzle_shift(g) for c in U.SWEEP_CASES.values() for g in c["gs"] if 1 in c["modes"]} == {5, 6, 7, 8}
    assert sum(g ** 3 % 64 != 0 for g in U.SWIZZLE_GS) >= 2 and 64 in U.SWIZZLE_GS and {1, 2} <= set(U.SWIZZLE_GS)
    assert any(40 <= g <= 55 for g in U.SWIZZLE_GS) and any(79 <= g <= 86 for g in U.SWIZZLE_GS)
    assert 13 ** 3 % 64 != 0  # the pack's last ballot is partial: its clamp decides bits


# ---------------------------------------------------------------------------
# 2. the thresholds themselves
# ---------------------------------------------------------------------------
def test_shift_boundaries_lds_limits_and_cap_values():
    assert [U.map_swizzle_shift(g) for g in (1, 39, 40, 55, 56, 78, 79, 109)] == [5, 5, 6, 6, 7, 7, 8, 8]
    assert U.map_swizzle_shift(110) in (8, 9) and U.map_swizzle_shift(64) == 7
    assert U.map_lds_max_grid() == 109 and U.map_planes_max_grid() == 86 and U.view_lds_max_grid() == 86
    assert U.map_lds_bytes(109) <= U.K_LDS_BYTES < U.map_lds_bytes(110)
    assert 2 * U.map_lds_bytes(86) + U.K_VIEW_SCRATCH <= U.K_LDS_BYTES < 2 * U.map_lds_bytes(87)
    assert U.map_lds_bytes(1) == 128 and U.map_lds_bytes(64) == 32768 and U.map_lds_bytes(12) == 256  # 54 words in two groups of 32
    assert [U.chunk_cap(n) for n in (1, 6, 170, 171, 256, 511, 512, 513, 4096)] == [512, 86, 4, 3, 2, 2, 1, 1, 1]
    # where mode 0 turns from LDS to the grid in place, per entry point (the viewpoint kernel's mode 0 is always in place)
    assert U.node_shape(1, 315, 0, 109).lds and not U.node_shape(1, 315, 0, 110).lds
    assert U.node_shape(1, 315, 0, 86, planes=2).lds and not U.node_shape(1, 315, 0, 87, planes=2).lds
    assert U.sweep_shape(1, 8, 0, 109).lds and not U.sweep_shape(1, 8, 0, 110).lds
    assert not U.view_shape(1, 8, 0, 20).lds and U.view_shape(1, 8, 1, 86).lds
    for refused in (lambda: U.node_shape(1, 315, 1, 110), lambda: U.node_shape(1, 315, 1, 87, planes=2), lambda: U.sweep_shape(1, 8, 1, 110),
                    lambda: U.view_shape(1, 8, 1, 87)):
        with pytest.raises(AssertionError):
            refused()
    # worked examples, by hand from the host code
    s = U.node_shape(6, 567, 2, 12)
    assert (s.groups, s.chunks, s.chunk_waves, s.words) == (9, 2, 5, 18) and (s.chunks * s.chunk_waves - 1) * 64 == 576
    s = U.node_shape(171, 2431, 1, 12)
    assert (s.groups, s.uncapped, s.cap, s.chunks, s.chunk_waves, s.turns) == (38, 5, 3, 3, 13, 2)
    s = U.node_shape(512, 567, 1, 12)
    assert (s.chunks, s.chunk_waves, s.turns) == (1, 9, 2)
    s = U.sweep_shape(171, 40, 1, 12)
    assert (s.cap, s.chunk_items, s.chunks, s.turns) == (3, 14, 3, 2)
    s = U.sweep_shape(512, 19, 1, 12)
    assert (s.chunks, s.chunk_items, s.turns) == (1, 19, 3)
    s = U.sweep_shape(6, 41, 2, 12)  # seven items per workgroup, not eight: the last chunk has six, and two waves leave
    assert (s.chunks, s.chunk_items, s.last_items) == (6, 7, 6)
    s = U.view_shape(171, 20, 1, 12)
    assert (s.chunk_items, s.chunks, s.last_items) == (7, 3, 6)
    # the default lattice of TaskConfig
    s = U.node_shape(50, 81 * 81 * 51, 1, 64)
    assert s.cap_binds and s.chunks == 11 and s.turns > 1 and s.shift == 7


# ---------------------------------------------------------------------------
# 3. the swizzle is a bijection inside the LDS it is given
# ---------------------------------------------------------------------------
def test_swizzle_is_a_bijection_of_the_plane_and_every_voxel_word_lands_inside():
    for g in range(1, U.map_lds_max_grid() + 1):
        shift, total = U.map_swizzle_shift(g), U.map_lds_bytes(g) // 4
        assert total % 32 == 0 and U.grid_words(g) <= total and 4 * total * (2 if g <= U.map_planes_max_grid() else 1) <= U.K_LDS_BYTES
        w = np.arange(total)
        image = U.map_swizzle(w, shift)
        assert np.array_equal(np.sort(image), w), g                 # one-to-one on [0, W): also on each of two planes of W words
        assert np.array_equal(image >> 5, w >> 5), g                # inside each aligned group of 32 words
        assert int(image[:U.grid_words(g)].max()) < total, g        # every word that holds a voxel lands inside
        assert ((g ** 3 - 1) >> 5) < U.grid_words(g)                # the readers' last word is one the pack writes
    for g in range(1, U.view_lds_max_grid() + 1):
        assert U.K_VIEW_SCRATCH + 8 * (U.map_lds_bytes(g) // 4) <= U.K_LDS_BYTES and U.K_VIEW_SCRATCH % 128 == 0


def test_a_pack_shift_off_by_one_misplaces_words_at_every_grid_of_the_tables():
    """Were map_pack_bits to swizzle with shift - 1 while the readers keep shift, words of every grid size of the LDS cases but
    the two that fit one group of 16 words would sit where no reader looks."""
    grids = sorted({g for c in U.NODE_CASES.values() if c["mode"] == 1 for g in c["gs"]} | {g for c in U.SWEEP_CASES.values() if 1 in c["modes"]
                                                                                           for g in c["gs"]})
    for g in grids:
        shift = U.map_swizzle_shift(g)
        wrong = U.misplaced_words(g, shift - 1, shift)
        assert bool(wrong) == (U.grid_words(g) > 16), g
        assert not U.misplaced_words(g, shift, shift)
    assert U.misplaced_words(12, 4, 5)  # ... which the G = 12 cases of the older tests see as well


# ---------------------------------------------------------------------------
# 4. the store loop writes every word once; without its chunk term the later chunks' words keep the poison
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(c for c in U.NODE_CASES if "swizzle" not in c))
def test_store_loop_writes_every_word_once(cid):
    from tests import flightmap_oracle as MO
    c = U.NODE_CASES[cid]
    m = int(np.prod(c["dims"]))
    shape = U.node_shape(c["n"], m, c["mode"], c["gs"][0])
    want = U.node_want(c["gs"][0], c["dims"], c["sets"], (0, 0, 0))[U.SPARSE]
    got, writes = U.store_words(shape, U.bits_of(want, m), 0x5A5A5A5A)
    assert (writes == 1).all() and np.array_equal(got, want)
    assert np.array_equal(want, MO.pack_words(U.bits_of(want, m)[None])[0])
    broken, _ = U.store_words(shape, U.bits_of(want, m), 0x5A5A5A5A, drop_chunk_term=True)
    assert (shape.chunks > 1) == bool((broken == 0x5A5A5A5A).any())
    if shape.chunks > 1:
        assert not np.array_equal(broken, want)


# ---------------------------------------------------------------------------
# 5. the oracle-side conditions
# ---------------------------------------------------------------------------
def _shares(g, dims, sets):
    """Per set: the share of nodes blocked with unknown_blocks 0, and the shares (blocked, costly, clear) of the classify kernel."""
    m = int(np.prod(dims))
    blocked, costly = U.classify_want(g, dims, sets, 0, 0)
    b, c = U.bits_of(blocked, m).mean(1), U.bits_of(costly, m).mean(1)
    return b, c, 1.0 - b - c


@pytest.mark.parametrize("g", U.SWIZZLE_GS + (12, 13))
def test_every_answer_of_the_node_kernels_occurs(g):
    dims = (9, 9, 7)
    sets = U.SWIZZLE_SETS if g in U.SWIZZLE_GS else U.ALL_SETS
    b, c, clear = _shares(g, dims, sets)
    print("node shares", g, np.round(b, 3).tolist(), np.round(c, 3).tolist())
    assert ((b >= 0.1) & (b <= 0.9)).any()  # both answers in at least 10 % of the nodes of one env
    if g == 1:  # one voxel has one class: the three classes occur, each in an env of its own or beside one other
        assert (b >= 0.05).any() and (c >= 0.05).any() and (clear >= 0.05).any()
    else:
        assert ((b >= 0.05) & (c >= 0.05) & (clear >= 0.05)).any()
    m = int(np.prod(dims))
    with_unknown = U.bits_of(U.node_want(g, dims, sets, (1, 0, 0)), m).mean(1)
    assert ((with_unknown >= 0.1) & (with_unknown <= 0.9)).any()


def test_the_distinct_sets_keep_the_character_of_the_older_cases():
    tri, rng, vox = U.map_sets(12)
    assert (tri[U.FREE] < 0).all() and (tri[U.UNKNOWN] == 0).all() and (tri[U.OCCUPIED] > 0).all()
    assert (tri == -128).any() and (tri == 127).any()
    assert (np.ptp(vox, axis=1) > 0).all() and (vox[U.SMALL] < 0.3 * vox[U.RANDOM]).all()  # anisotropic; far smaller than the lattice
    for n in (171, 512):
        a = U.assign(n)
        assert set(a.tolist()) == set(range(U.D)) and (a[1:] != a[:-1]).all() and np.array_equal(a, U.assign(n))
    frm, to, start = U.leg_pool(12)
    for k in (5, 8, 19, 24, 40, 41, 57):
        rows = U.pick(k)
        assert len(rows) == k and len(set(rows.tolist())) == k
        kinds = set((rows % 40).tolist())
        assert any(16 <= x < 22 for x in kinds) and any(22 <= x < 28 for x in kinds) and any(31 <= x < 37 for x in kinds)
    assert np.isnan(to[:, U.pick(41)]).any() and frm.shape[-1] > 3 and to.shape[-1] > 3 and start.shape[-1] > 3


@pytest.mark.parametrize("cid", sorted(U.SWEEP_CASES))
def test_sweep_cases_are_robust_and_mixed(cid):
    """At most 1 % of the items of every (from-form, radius, flags) of a case may stand within the oracle's band; both answers of
    the MAP bit occur."""
    c = U.SWEEP_CASES[cid]
    hits = []
    for g in c["gs"]:
        for broadcast in (False, True):
            for radius in c["radii"]:
                for flags in c["flags"]:
                    code, robust = U.sweep_want(g, c["k"], c["sets"], broadcast, radius, flags)
                    assert code.shape == (len(c["sets"]), c["k"])
                    assert (~robust).mean() <= 0.01, (cid, g, broadcast, radius, flags, float((~robust).mean()))
                    hits.append(float(((code & SO.MAP) != 0).mean()))
                    if flags[1]:
                        assert ((code & SO.OUTSIDE) != 0).any()
    print("sweep MAP shares", cid, np.round(hits, 3).tolist())
    assert 0.0 < min(hits) and max(hits) < 1.0
    assert any(0.1 <= h <= 0.9 for h in hits)


def test_viewpoint_winners_sit_where_the_cases_need_them():
    """Derived from the oracle's winners on the 1287-node lattice, whose window is the whole lattice (slot == node id): a winner in
    wave 7 that is tied in cost with the same lane's later turn, and a winner in a lane's third turn."""
    s, w = U.view_case_data("t20-three-turns")
    windows = U.view_windows("t20-three-turns")
    dims, m = s["dims"], int(np.prod(s["dims"]))
    assert m == 1287 and U.view_shape(6, 20, 1, U.VIEW_G, 0, m).turns == 3
    assert len(np.unique(s["field"])) == 4  # three costs and "no route"
    seen = {"wave7": 0, "tied_later_turn": 0, "third_turn": 0, "waves": set(), "turns": set()}
    for (d, j), win in windows.items():
        node = int(w["node"][d, j])
        if node < 0:
            continue
        at = U.slot_of(node, win, dims)
        assert at.slot == node
        seen["waves"].add(at.wave)
        seen["turns"].add(at.turn)
        seen["third_turn"] += at.turn == 2
        if d == U.V_FREE:
            # nothing hides anything in the all-free grid: every node sees the target, so the routed ones are known from the field
            assert int(w["count"][d, j, 0]) == m == int(w["in_range"][d, j])
            later = node + U.K_LANES  # the same lane, one turn on
            assert at.wave == U.K_WAVES - 1 and at.turn == 0 and s["field"][d, later] == s["field"][d, node] == w["cost"][d, j]
            seen["wave7"] += 1
            seen["tied_later_turn"] += bool(w["tied"][d, j])
    print("viewpoint winners", seen)
    assert seen["wave7"] >= 1 and seen["tied_later_turn"] == seen["wave7"] and seen["third_turn"] >= 1
    assert {0, U.K_WAVES - 1} <= seen["waves"] and {0, 2} <= seen["turns"]
    # the first target alone (the T = 1 case) already has both
    first = [U.slot_of(int(w["node"][d, 0]), windows[(d, 0)], dims) for d in (U.V_FREE, U.V_OPEN)]
    assert first[0].wave == U.K_WAVES - 1 and first[1].turn == 2
    # every wave counts: the nodes that see a target are spread over all eight waves' slots
    assert int(w["count"][U.V_OPEN, :, 0].max()) > U.K_LANES and int(w["count"][U.V_UNKNOWN, :, 0].max()) > 0
    # the special targets are no targets; the all-occupied grid hides almost everything
    g = U.VIEW_G
    outside = ~((s["targets"] >= 0) & (s["targets"] < g)).all(-1)
    assert outside.any() and (w["node"][outside] == -1).all() and not w["count"][outside].any()


@pytest.mark.parametrize("cid", sorted(c for c in U.VIEW_CASES if "swizzle" in c))
def test_viewpoint_swizzle_cases_are_mixed(cid):
    c = U.VIEW_CASES[cid]
    s, w = U.view_case_data(cid)
    sets = list(c["sets"])
    see, in_range = w["count"][sets, :, 0], w["in_range"][sets]
    print("viewpoint swizzle", cid, see.tolist(), in_range.tolist())
    assert ((see > 0) & (see < in_range)).sum() >= 3  # some nodes see the target and some are hidden: the planes decide
    assert (w["node"][sets] >= 0).any() and w["tied"][sets].any()

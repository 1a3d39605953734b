"""CPU: the numpy / Python reference of gnbv_tour_route (tests/tour_oracle.py) has the properties the rule promises -- never
longer than nearest neighbour, never shorter than the optimum, the tie rules, the cap, the tail, the status bits; the new entry
point is declared, exported and bound and refuses bad arguments before any launch; euclid_mm equals its oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import tour_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = TO.INF


def _lattice_points(rng, p, side=6, step=100):
    """Integer points on a coarse lattice: many equal distances, so the tie rules have work to do."""
    return rng.integers(0, side, (p, 3)) * step


def _dist(pts):
    pts = np.asarray(pts, np.float64)
    return np.rint(np.linalg.norm(pts[:, None] - pts[None], axis=-1)).astype(np.uint32)


def test_route_is_no_longer_than_nearest_neighbour_and_no_shorter_than_the_optimum():
    rng = np.random.default_rng(0)
    improved = 0
    for trial in range(60):
        p = int(rng.integers(2, 9)) if trial < 40 else int(rng.integers(9, 40))
        D = _dist(_lattice_points(rng, p))
        order, routed, length, status, moves = TO.route(D)
        assert routed == p and status == 0 and sorted(order.tolist()) == list(range(p)) and order[0] == 0
        assert length == TO.path_length(D, order.tolist())
        nn = TO.nearest_neighbour_length(D)
        assert length <= nn
        improved += int(length < nn)
        assert (moves > 0) == (length < nn)
        if p <= 8:
            assert length >= TO.brute_force(D)
    assert improved >= 10


def test_nearest_neighbour_ties_go_to_the_lowest_index():
    # points 1, 2, 3 all 5 away from the start; from 1 the points 2 and 3 are both 7 away: 0, 1, 2, 3
    D = np.array([[0, 5, 5, 5], [5, 0, 7, 7], [5, 7, 0, 7], [5, 7, 7, 0]], np.uint32)
    order, routed, length, status, moves = TO.route(D, max_moves=0)
    assert order.tolist() == [0, 1, 2, 3] and routed == 4 and length == 19 and status == 0
    # an all-equal matrix: the identity, and no move (no delta is below 0)
    E = np.full((6, 6), 9, np.uint32)
    np.fill_diagonal(E, 0)
    order, routed, length, status, moves = TO.route(E)
    assert order.tolist() == list(range(6)) and length == 45 and moves == 0 and status == 0


def _sym(p, fill, entries):
    D = np.full((p, p), fill, np.uint32)
    np.fill_diagonal(D, 0)
    for (a, b), v in entries.items():
        D[a, b] = D[b, a] = v
    return D


def _deltas(D, t):
    """The 2-opt deltas of one round, restated: {(i, j): delta}."""
    out = {}
    for i in range(1, len(t)):
        for j in range(i + 1, len(t)):
            d = int(D[t[i - 1], t[j]]) - int(D[t[i - 1], t[i]])
            if j + 1 < len(t):
                d += int(D[t[i], t[j + 1]]) - int(D[t[j], t[j + 1]])
            out[(i, j)] = d
    return out


def test_two_opt_ties_go_to_the_lowest_i_then_the_lowest_j():
    ident = [0, 1, 2, 3, 4]
    # nearest neighbour gives 0 1 2 3 4; the moves (1, 2) and (1, 3) both have delta -14, every other move is worse: lowest j
    A = _sym(5, 50, {(0, 1): 10, (1, 2): 10, (2, 3): 30, (3, 4): 30, (0, 2): 12, (0, 3): 12, (1, 3): 14, (1, 4): 14, (2, 4): 30})
    assert TO.route(A, max_moves=0)[0].tolist() == ident
    dl = _deltas(A, ident)
    assert sorted(k for k, v in dl.items() if v == min(dl.values())) == [(1, 2), (1, 3)] and dl[(1, 2)] == -14
    assert TO.route(A, max_moves=1)[0].tolist() == [0, 2, 1, 3, 4]
    # (1, 3) and (2, 3) both have delta -26, every other move is worse: lowest i
    B = _sym(5, 50, {(0, 1): 10, (1, 2): 10, (2, 3): 30, (3, 4): 60, (0, 2): 20, (0, 3): 12, (1, 3): 14, (1, 4): 32, (2, 4): 30})
    assert TO.route(B, max_moves=0)[0].tolist() == ident
    dl = _deltas(B, ident)
    assert sorted(k for k, v in dl.items() if v == min(dl.values())) == [(1, 3), (2, 3)] and dl[(1, 3)] == -26
    assert TO.route(B, max_moves=1)[0].tolist() == [0, 3, 2, 1, 4]
    # the cap of one move was met with a further improving move in sight, or not: bit 2 says which
    for D in (A, B):
        free = TO.route(D)
        assert free[3] == 0 and (TO.route(D, max_moves=1)[3] == TO.CAPPED) == (free[4] > 1)


def test_max_moves_zero_is_nearest_neighbour_with_the_cap_bit_exactly_when_a_move_exists():
    rng = np.random.default_rng(1)
    with_move = without = 0
    for trial in range(80):
        p = int(rng.integers(2, 14))
        D = _dist(_lattice_points(rng, p))
        free = TO.route(D)
        capped = TO.route(D, max_moves=0)
        assert capped[4] == 0 and capped[0][0] == 0
        # nearest neighbour, restated: always the nearest unvisited point, ties to the lowest index
        t, left = [0], list(range(1, p))
        while left:
            j = min(left, key=lambda j: (int(D[t[-1], j]), j))
            t.append(j)
            left.remove(j)
        assert capped[0].tolist() == t
        assert (capped[3] == TO.CAPPED) == (free[4] > 0) and capped[3] in (0, TO.CAPPED)
        with_move += int(free[4] > 0)
        without += int(free[4] == 0)
        if free[4] > 1:  # a cap in the middle stops there, bit set
            mid = TO.route(D, max_moves=free[4] - 1)
            assert mid[3] == TO.CAPPED and mid[4] == free[4] - 1 and mid[2] > free[2]
        assert TO.route(D, max_moves=free[4])[3] == 0  # exactly enough moves: no bit
    assert with_move >= 10 and without >= 10


def test_unreachable_points_and_count_go_to_the_tail_in_ascending_order():
    rng = np.random.default_rng(2)
    D = _dist(_lattice_points(rng, 9, side=20))
    for j in (2, 5):  # no route from the start; the rest of their rows and columns is finite (never read: not in the route set)
        D[0, j] = D[j, 0] = INF
    order, routed, length, status, _ = TO.route(D, count=8)
    assert routed == 6 and status == 0
    assert sorted(order[:6].tolist()) == [0, 1, 3, 4, 6, 7] and order[6:].tolist() == [2, 5, 8]
    assert length == TO.path_length(D, order[:6].tolist())
    order, routed, length, status, _ = TO.route(D, count=1)
    assert order.tolist() == list(range(9)) and routed == 1 and length == 0 and status == 0
    # entries at or above count are never read
    D2 = D.copy()
    D2[8, :] = D2[:, 8] = 1
    assert TO.route(D2, count=8)[0].tolist() == TO.route(D, count=8)[0].tolist()


def test_status_bits_one_and_four():
    rng = np.random.default_rng(3)
    D = _dist(_lattice_points(rng, 7, side=20))
    assert TO.route(D)[3] == 0
    M = D.copy()
    M[2, 4] = M[4, 2] = INF  # both reachable from the start, no route between them
    order, routed, length, status, _ = TO.route(M)
    assert routed == 7 and status & TO.MISSING_LEG and not status & TO.BAD_COUNT
    assert length == TO.path_length(M, order.tolist())  # the entry is used as the plain number, wherever it lands
    for bad in (0, 8, -1):
        order, routed, length, status, _ = TO.route(D, count=bad)
        assert order.tolist() == list(range(7)) and (routed, length, status) == (1, 0, TO.BAD_COUNT)
    # a missing leg outside the route set sets nothing
    M = D.copy()
    M[0, 3] = M[3, 0] = M[3, 5] = M[5, 3] = INF
    assert TO.route(M)[3] == 0


def test_header_declares_and_library_exports_the_entry_point():
    from gennbv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gennbv_hip.h")).read()
    assert re.search(r"\bint\s+gnbv_tour_route\s*\(\s*const\s+GnbvTourRoute\s*\*", hdr)
    assert _lib.SIGNATURES["gnbv_tour_route"] == (C.c_int, [C.c_void_p] * 2)
    lib = _lib.load()
    assert lib.gnbv_tour_route is not None
    assert lib.gnbv_abi_version() == 5
    body = re.search(r"typedef struct GnbvTourRoute \{(.*?)\} GnbvTourRoute;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [re.split(r"[\s\*]+", n)[-1] for n in names]
    assert names == [f[0] for f in _lib.GnbvTourRoute._fields_]
    from gennbv_amd.csrc import build
    assert "tour.hip" in build.SOURCES


def test_invalid_arguments_are_refused_before_any_launch():
    """Argument checks come first, so the refusals can be seen without a GPU (the pointers are never dereferenced)."""
    from gennbv_amd import _lib
    lib = _lib.load()

    def args(**kw):
        a = _lib.GnbvTourRoute()
        a.n, a.p, a.max_moves = 2, 5, 25
        a.dist_mm, a.count, a.order, a.routed, a.length_mm, a.status = 4096, 4096, 4096, 4096, 4096, 4096
        for f, v in kw.items():
            setattr(a, f, v)
        return a
    assert lib.gnbv_tour_route(None, None) == 1  # hipErrorInvalidValue
    for kw in (dict(n=0), dict(n=65536), dict(p=0), dict(p=129), dict(max_moves=-1), dict(dist_mm=None), dict(order=None),
               dict(routed=None), dict(length_mm=None), dict(status=None)):
        assert lib.gnbv_tour_route(C.byref(args(**kw)), None) == 1, kw


def test_route_tour_refuses_what_it_cannot_run():
    from gennbv_amd import _lib
    from gennbv_amd.ops.tour import euclid_mm, route_tour
    with pytest.raises(_lib.GennbvHipError):
        route_tour(torch.zeros(2, 4, 4, dtype=torch.int32))  # a CPU tensor: no CPU fallback
    with pytest.raises(_lib.GennbvHipError):
        euclid_mm(torch.zeros(2, 4, 2))


def test_euclid_mm_equals_the_oracle():
    from gennbv_amd.ops.flight_field import field_u32
    from gennbv_amd.ops.tour import euclid_mm
    rng = np.random.default_rng(4)
    pts = (rng.uniform(-8, 8, (3, 7, 6))).astype(np.float32)
    pts[1, 2, 1] = np.nan
    pts[2, 3] = pts[2, 4]  # two points in one place: 0
    count = np.array([7, 5, 1], np.int32)
    for c in (None, count):
        want = TO.euclid(pts, c)
        got = field_u32(euclid_mm(torch.as_tensor(pts), None if c is None else torch.as_tensor(c)))
        assert got.dtype == np.uint32 and np.array_equal(got, want)
    want = TO.euclid(pts, None)
    assert (want[1, 2] == INF).all() and (want[1, :, 2] == INF).all() and want[2, 3, 4] == 0
    assert np.array_equal(want, want.transpose(0, 2, 1)) and (np.diagonal(want[0]) == 0).all()
    assert (TO.euclid(pts, count)[1, 5:] == INF).all() and (TO.euclid(pts, count)[1, :, 5:] == INF).all()
    far = np.zeros((1, 2, 3))
    far[0, 1, 0] = 5.0e6  # 5e9 mm does not fit
    assert field_u32(euclid_mm(torch.as_tensor(far)))[0, 0, 1] == INF and TO.euclid(far)[0, 0, 1] == INF

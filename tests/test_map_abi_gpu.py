"""GPU: the four belief-map entry points at the C ABI past one workgroup's one turn and at every swizzle shift --
gnbv_flight_blocked_tri, gnbv_flight_classify_tri (csrc/flightmap.hip), gnbv_sweep_tri (csrc/sweepmap.hip) and
gnbv_frontier_viewpoints (csrc/frontview.hip) against their unchanged numpy oracles: lattices of several chunks with every tail
residue, batches at which the chunk cap of the LDS modes binds (n = 171) or leaves one workgroup per env (n = 512), a viewpoint
window of three turns whose winner is placed in wave 7 and in a third turn, and one grid size per swizzle shift.  Outputs are
poisoned first and every element is compared, padding and guards included; every comparison is exact (the sweep by
sweepmap_oracle.agrees).  tests/map_abi_util.py has the cases; tests/test_map_abi_regimes_cpu.py shows, without a GPU, that each
reaches the regime its id names."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import map_abi_util as U
from tests import sweepmap_oracle as SO
from tests import test_flight_cautious_gpu as TC
from tests import test_flightmap_gpu as TM
from tests import test_sweepmap_gpu as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x5A5A5A5A
INVALID = 1  # hipErrorInvalidValue

NODE_PARAMS = [(cid, g) for cid in sorted(U.NODE_CASES) for g in U.NODE_CASES[cid]["gs"]]
SWEEP_PARAMS = [(cid, g) for cid in sorted(U.SWEEP_CASES) for g in U.SWEEP_CASES[cid]["gs"]]


def _lib():
    from gennbv_amd import _lib
    return _lib.load()


def _limits_match():
    """The restated LDS limits are the library's."""
    lib = _lib()
    return (U.map_lds_max_grid() == int(lib.gnbv_flightmap_lds_max_grid()) == int(lib.gnbv_sweepmap_lds_max_grid())
            and U.map_planes_max_grid() == int(lib.gnbv_flightmap_classify_lds_max_grid())
            and U.view_lds_max_grid() == int(lib.gnbv_frontview_lds_max_grid()))


@functools.lru_cache(maxsize=2)
def _grid_inputs(g, sets, n):
    """The n envs of a node or sweep case on the device: (both grid forms, range_gt, voxel_size, the row of every env's set)."""
    case = dict(sets=sets, n=n)
    rows = U.case_rows(case)
    tri, rng, vox = U.map_sets(g)
    which = np.array(sets)[rows]
    forms = TS._forms(np.ascontiguousarray(tri[which]), g)
    return forms, torch.tensor(np.ascontiguousarray(rng[which])).to(DEV), torch.tensor(np.ascontiguousarray(vox[which])).to(DEV), rows


def _modes(case):
    return (1, 0) if case["mode"] == 1 else (case["mode"],)  # mode 0 beside the LDS mode it resolves to


# ---------------------------------------------------------------------------
# 1. the node kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid,g", NODE_PARAMS)
def test_blocked_words_equal_the_oracle_in_every_launch_regime(cid, g):
    c = U.NODE_CASES[cid]
    lat = U.lattice(c["dims"])
    shape = U.node_shape(c["n"], lat.num_nodes, c["mode"], g)
    assert _limits_match() and shape.lds == (c["mode"] == 1) and shape.words == lat.words
    forms, rng_t, vox_t, rows = _grid_inputs(g, c["sets"], c["n"])
    for flags in c["flags"]:
        want = U.node_want(g, c["dims"], c["sets"], flags)[rows]
        for name, t in forms.items():
            for mode in _modes(c):
                err, got = TM._launch(lat, t, g, rng_t, vox_t, U.RHO, flags, mode)
                assert err == 0, (flags, name, mode)
                assert np.array_equal(got, want), (flags, name, mode, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("cid,g", NODE_PARAMS)
def test_classes_equal_the_composed_oracle_in_every_launch_regime(cid, g):
    c = U.NODE_CASES[cid]
    lat = U.lattice(c["dims"])
    shape = U.node_shape(c["n"], lat.num_nodes, c["mode"], g, planes=2)
    assert _limits_match() and shape.lds == (c["mode"] == 1) and shape.words == lat.words
    forms, rng_t, vox_t, rows = _grid_inputs(g, c["sets"], c["n"])
    for outside, ground in sorted({(o, gr) for _, o, gr in c["flags"]}):
        want_b, want_c = (w[rows] for w in U.classify_want(g, c["dims"], c["sets"], outside, ground))
        assert not (want_b & want_c).any()
        for name, t in forms.items():
            for mode in _modes(c):
                err, got_b, got_c = TC._classify(lat, t, g, rng_t, vox_t, U.RHO, outside, ground, mode)
                assert err == 0, (outside, ground, name, mode)
                assert np.array_equal(got_b, want_b), (outside, ground, name, mode, np.argwhere(got_b != want_b)[:5].tolist())
                assert np.array_equal(got_c, want_c), (outside, ground, name, mode, np.argwhere(got_c != want_c)[:5].tolist())


# ---------------------------------------------------------------------------
# 2. the swept sphere
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid,g", SWEEP_PARAMS)
def test_sweep_codes_equal_the_oracle_in_every_launch_regime(cid, g):
    c = U.SWEEP_CASES[cid]
    n, k = c["n"], c["k"]
    assert _limits_match()
    forms, rng_t, vox_t, rows = _grid_inputs(g, c["sets"], n)
    which = np.array(c["sets"])[rows]
    frm, to, start = U.leg_pool(g)
    pick = U.pick(k)
    frm_t = torch.tensor(np.ascontiguousarray(frm[which][:, pick])).to(DEV)  # [n, K, 6]: a start per item, row stride 6
    to_t = torch.tensor(np.ascontiguousarray(to[which][:, pick])).to(DEV)    # [n, K, 6]
    start_t = torch.tensor(np.ascontiguousarray(start[which])).to(DEV)       # [n, 6]: one start per env
    assert frm_t.is_contiguous() and to_t.is_contiguous() and start_t.is_contiguous()
    assert frm_t.stride(1) == 6 and to_t.stride(1) == 6 and start_t.stride(0) == 6  # row strides above 3
    for mode in c["modes"]:
        shape = U.sweep_shape(n, k, mode, g)
        assert shape.lds == (mode == 1 or (mode == 0 and g <= U.map_lds_max_grid()))
    for broadcast, f_t in ((False, frm_t), (True, start_t)):
        for radius in c["radii"]:
            for flags in c["flags"]:
                want, robust = (w[rows] for w in U.sweep_want(g, k, c["sets"], broadcast, radius, flags))
                for name, t in forms.items():
                    for mode in c["modes"]:
                        err, got, guard_ok = TS._launch(t, g, rng_t, vox_t, f_t, to_t, radius, flags, mode)
                        what = (broadcast, radius, flags, name, mode)
                        assert err == 0 and guard_ok, what
                        assert SO.agrees(got, want, robust), (what, np.argwhere(got != want)[:5].tolist())
    if g > U.map_lds_max_grid():  # mode 1 is refused before anything is launched
        err, got, guard_ok = TS._launch(forms["i8"], g, rng_t, vox_t, frm_t, to_t, c["radii"][0], c["flags"][0], 1)
        assert err == INVALID and guard_ok and (got == 0xA5).all()


# ---------------------------------------------------------------------------
# 3. the frontier viewpoints
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _view_inputs(cid):
    """A viewpoint case on the device: (both grid forms, dict of the launch's tensors and scalars, the oracle's rows)."""
    c = U.VIEW_CASES[cid]
    s, w = U.view_case_data(cid)
    rows = np.array(c["sets"])[U.case_rows(c)]
    t = c["t"]
    forms = TS._forms(np.ascontiguousarray(s["tri"][rows]), c["g"])
    dev = {k: torch.tensor(np.ascontiguousarray(v)).to(DEV) for k, v in (("range_gt", s["range_gt"][rows]), ("voxel_size", s["voxel_size"][rows]),
                                                                          ("field", s["field"][rows].view(np.int32)),
                                                                          ("targets", s["targets"][rows, :t]))}
    want = {k: w[k][rows, :t] for k in ("node", "cost", "count")}
    return forms, dev, want


def _view_launch(tri_t, c, s, dev, mode, chunk):
    """gnbv_frontier_viewpoints at the C ABI into buffers pre-filled with 0x5A5A5A5A, one guard row before and one after every
    output -> (return code, node, cost, count, the guard rows untouched)."""
    from gennbv_amd import _lib
    n, t, g = c["n"], c["t"], c["g"]
    node = torch.full((n + 2, t), FILL, dtype=torch.int32, device=DEV)
    cost = torch.full((n + 2, t), FILL, dtype=torch.int32, device=DEV)
    count = torch.full((n + 2, t, 2), FILL, dtype=torch.int32, device=DEV)
    i8 = tri_t.dtype == torch.int8
    row = int(tri_t.stride(0))
    a = _lib.GnbvFrontView(n=n, t=t, g=g, tri_i8=tri_t.data_ptr() if i8 else None, tri_i8_row_stride=row if i8 else 0,
                           tri_f32=None if i8 else tri_t.data_ptr(), tri_f32_row_stride=0 if i8 else row, range_gt=dev["range_gt"].data_ptr(),
                           voxel_size=dev["voxel_size"].data_ptr(), nx=s["dims"][0], ny=s["dims"][1], nz=s["dims"][2],
                           lo=(C.c_double * 3)(*s["lo"]), h=(C.c_double * 3)(*s["h"]), field=dev["field"].data_ptr(),
                           targets=dev["targets"].data_ptr(), r_min=s["r_min"], r_max=s["r_max"], max_unknown=s["max_unknown"],
                           node_out=node[1:].data_ptr(), cost_out=cost[1:].data_ptr(), count_out=count[1:].data_ptr(), chunk=chunk, mode=mode)
    err = _lib.load().gnbv_frontier_viewpoints(C.byref(a), None)
    torch.cuda.synchronize()
    node, cost, count = node.cpu().numpy(), cost.cpu().numpy().view(np.uint32), count.cpu().numpy()
    guard_ok = all(bool((x[0].view(np.uint32) == FILL).all() and (x[-1].view(np.uint32) == FILL).all()) for x in (node, cost, count))
    return err, node[1:-1], cost[1:-1], count[1:-1], guard_ok


@pytest.mark.parametrize("cid", sorted(U.VIEW_CASES))
def test_viewpoints_equal_the_oracle_in_every_launch_regime(cid):
    c = U.VIEW_CASES[cid]
    s, _ = U.view_case_data(cid)
    forms, dev, want = _view_inputs(cid)
    assert _limits_match()
    for name, tri_t in forms.items():
        for mode, chunk in c["runs"]:
            shape = U.view_shape(c["n"], c["t"], mode, c["g"], chunk)
            assert shape.lds == (mode == 1) and shape.lds_bytes <= U.K_LDS_BYTES
            err, node, cost, count, guard_ok = _view_launch(tri_t, c, s, dev, mode, chunk)
            what = (name, mode, chunk)
            assert err == 0 and guard_ok, what
            assert np.array_equal(node, want["node"]), (what, np.argwhere(node != want["node"])[:5].tolist())
            assert np.array_equal(cost, want["cost"]), (what, np.argwhere(cost != want["cost"])[:5].tolist())
            assert np.array_equal(count, want["count"]), (what, np.argwhere(count != want["count"])[:5].tolist())
        if c["g"] > U.view_lds_max_grid():  # the planes do not fit: mode 1 is refused before anything is launched
            err, node, cost, count, guard_ok = _view_launch(tri_t, c, s, dev, 1, 0)
            assert err == INVALID and guard_ok
            assert (node.view(np.uint32) == FILL).all() and (cost == FILL).all() and (count.view(np.uint32) == FILL).all()

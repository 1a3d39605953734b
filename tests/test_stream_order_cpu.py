"""The census of the stream-order tests: every function of include/gennbv_hip.h that takes a stream is bound with a pointer as its last
argument and has a case in tests/test_stream_order_gpu.py (or a stated reason why not).  A new entry point without a stream case fails
here, on a machine without a GPU."""
import ctypes as C

from gennbv_amd import _lib
from tests import stream_order_util as U
from tests import test_stream_order_gpu as G

# entry point -> what stands in the way of a stream case (keep it short: a reason names an obstacle, not a plan)
EXEMPT = {}


def test_header_parser_sees_every_declaration():
    fns = U.header_functions()
    assert set(fns) == set(_lib.SIGNATURES), sorted(set(fns) ^ set(_lib.SIGNATURES))
    for name, params in fns.items():
        assert len(params) == len(_lib.SIGNATURES[name][1]), (name, params)
    streamed = U.stream_entry_points()
    assert len(streamed) > 70 and "gnbv_update_occ_grid" in streamed and "gnbv_tour_route" in streamed
    for name in ("gnbv_abi_version", "gnbv_voxel_workspace_bytes", "gnbv_flight_lds_max_nodes", "gnbv_prob_code_tables", "gnbv_linear_fold_ok"):
        assert name in fns and name not in streamed


def test_every_streamed_entry_point_is_bound_with_a_pointer_last():
    for name in U.stream_entry_points():
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        args = _lib.SIGNATURES[name][1]
        assert args and args[-1] is C.c_void_p, f"{name}: the last bound argument must be the stream pointer"


def test_every_streamed_entry_point_has_a_stream_case():
    streamed = set(U.stream_entry_points())
    covered = G.covered_entry_points()
    assert covered <= streamed, f"cases name functions without a stream parameter: {sorted(covered - streamed)}"
    assert set(EXEMPT) <= streamed and not (set(EXEMPT) & covered), "EXEMPT lists only streamed entry points without a case"
    assert all(isinstance(r, str) and r.strip() for r in EXEMPT.values())
    missing = streamed - covered - set(EXEMPT)
    assert not missing, f"no stream-order case (tests/test_stream_order_gpu.py CASES) for: {sorted(missing)}"


def test_the_case_table_is_well_formed():
    assert G.FORKS <= set(G.CASES)
    for name, (entries, make) in G.CASES.items():
        assert entries and callable(make), name

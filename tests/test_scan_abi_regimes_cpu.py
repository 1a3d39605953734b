"""CPU: every case of tests/test_scan_abi_gpu.py reaches the regime of csrc/scan.hip its id names.  kSortTile, kLeaf and
blocks_per_env are restated in tests/scan_abi_util.py and evaluated from n, the shapes and the numpy oracle's sets; no GPU is
involved, so a case that has gone vacuous shows up wherever the suite runs."""
import numpy as np
import pytest

from tests import scan_abi_util as U


@pytest.mark.parametrize("cid", sorted(U.CASES))
def test_case_reaches_its_regime(cid):
    info = U.check_regime(cid)
    print(cid, info)


def test_sort_geometry_thresholds():
    """Where the radix sort and the trees change path: tiles of 2048 keys, 256-entry scan chunks (16 digits x tiles), leaves of 32."""
    assert [U.blocks_per_env(n) for n in (1, 6, 16, 17, 50, 1023, 1024, 5000)] == [256, 256, 256, 241, 82, 5, 4, 4]
    assert [U.tiles_of(c) for c in (0, 1, 2048, 2049, 32768, 32769)] == [0, 1, 1, 2, 16, 17]
    assert [U.scan_chunks(c) for c in (1, 32768, 32769, 34817, 65536, 65537)] == [1, 1, 2, 2, 2, 3]
    assert [U.tree_pow2(c) for c in (1, 32, 33, 64, 65, 1024, 1025)] == [1, 1, 2, 2, 4, 32, 64]
    assert U.tiles_of(855_000) == 418 and U.blocks_per_env(50) == 82 and U.scan_chunks(855_000) == 27  # the evaluation of DESIGN.md
    assert U.clear_trips(1024, 4096) == 2 and U.clear_trips(6, 4096) == 1


def test_chamfer_shapes_straddle_the_tile_and_the_workgroup():
    sizes = {s for nm in U.CHAMFER_SHAPES for s in nm}
    assert {U.K_NN_TILE - 1, U.K_NN_TILE, U.K_NN_TILE + 1} <= sizes and U.K_NN_PER_WG == 1024
    assert any(m > 2 * U.K_NN_TILE for _, m in U.CHAMFER_SHAPES) and any(n > 2 * U.K_NN_PER_WG for n, _ in U.CHAMFER_SHAPES)
    assert any(m == 1 for _, m in U.CHAMFER_SHAPES) and any(n % 4 for n, _ in U.CHAMFER_SHAPES)


def test_numpy_packer_states_the_header():
    """pack_gt against check_gt_invariants on sizes around a leaf, in a permuted order and with a taller heap; the checker rejects a
    heap whose parent is not the union of its children."""
    rs = np.random.RandomState(0)
    clouds = [rs.rand(m, 3).astype(U.f32) for m in (1, 32, 33, 100, 1025)]
    perms = [rs.permutation(y.shape[0]) for y in clouds]
    for g in (U.pack_gt(clouds), U.pack_gt(clouds, perms), U.pack_gt(clouds, perms, extra_levels=2), U.pack_from_gt_tree(clouds)):
        U.check_gt_invariants(g, clouds)
    g = U.pack_gt(clouds)
    g.nodes[int(g.node_start[4]) + 1, 0, 0] += 0.5
    with pytest.raises(AssertionError):
        U.check_gt_invariants(g, clouds)

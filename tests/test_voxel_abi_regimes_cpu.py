"""CPU: every launch-regime case of tests/test_voxel_abi_gpu.py reaches the branch of csrc/voxel.hip its id names.  The dispatch
quantities are restated in tests/voxel_abi_util.py and evaluated from n, the shapes and the oracle's masks; no GPU is involved, so a
case that has gone vacuous shows up wherever the suite runs."""
import pytest

from tests import voxel_abi_util as U


@pytest.mark.parametrize("cid", sorted(U.LAUNCH_CASES))
def test_case_reaches_its_regime(cid):
    info = U.check_regime(cid)
    print(cid, info)


def test_dispatch_thresholds():
    """launch_masks: 512 / 1024 / 2048 envs are where k_hit_list, k_raycast and k_hit_mask drop to one workgroup per env."""
    d = U.dispatch
    assert [d(n, 16, 8, 12, True).fchunks for n in (1, 32, 33, 100, 511, 512, 513)] == [16, 16, 16, 6, 2, 1, 1]
    assert [d(n, 16, 8, 12, False).splits for n in (1, 128, 129, 180, 1023, 1024)] == [8, 8, 8, 6, 2, 1]
    assert [d(n, 16, 8, 12, False).chunks for n in (128, 129, 1024, 2047, 2048)] == [16, 16, 2, 2, 1]
    assert d(3, 93, 8, 12, True).path == "list" and d(3, 94, 8, 12, True).path == "large"  # (hit mask + word list + pixel queue in 160 KiB)
    assert not d(3, 105, 8, 12, False).windowed and d(3, 106, 8, 12, False).path_windowed
    assert not d(3, 109, 8, 12, False).hit_windowed and d(3, 110, 8, 12, False).hit_windowed
    assert U.chunk_ranges(96, 16)[11:13] == [(88, 96), (96, 96)] and U.chunk_ranges(96, 16)[15] == (120, 96)
    assert U.mask_words(16) == 128 and U.mask_words(72) == 11712 and U.mask_words(64) == 8192

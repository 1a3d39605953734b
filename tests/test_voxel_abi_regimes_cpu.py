"""CPU: every launch-regime case of tests/test_voxel_abi_gpu.py reaches the branch of csrc/voxel.hip its id names.  The dispatch
quantities are restated in tests/voxel_abi_util.py and evaluated from n, the shapes and the oracle's masks; no GPU is involved, so a
case that has gone vacuous shows up wherever the suite runs.

The restatement is held against the library's own decisions: csrc/voxel_plan.h is the host code that plans every mask launch, and
tests/voxel_plan_dump.cpp, compiled here with the host compiler under the address and undefined-behaviour sanitizers, prints its
plans.  One run of the program covers every tuple the tests below ask about."""
import json
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest

from tests import voxel_abi_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
LARGE = {None: -1, "0": 0, "1": 1}
# GENNBV_VOXEL_SLAB_PLANES as tests/test_voxel_gpu.py sets it (g, planes): heights that do not divide the grid among them
SLAB_OVERRIDES = [(16, 3), (20, 2), (64, 8), (33, 32), (128, 48), (16, 5), (64, 16)]
WORKSPACE_SHAPES = [(1, 16, 8, 12), (3, 33, 7, 9), (100, 64, 240, 320), (513, 16, 8, 12), (2, 128, 60, 80), (64, 203, 1, 1)]


@pytest.mark.parametrize("cid", sorted(U.LAUNCH_CASES))
def test_case_reaches_its_regime(cid):
    info = U.check_regime(cid)
    print(cid, info)


def _thresholds(d):
    """launch_masks: 512 / 1024 / 2048 envs are where k_hit_list, k_raycast and k_hit_mask drop to one workgroup per env."""
    assert [d(n, 16, 8, 12, True).fchunks for n in (1, 32, 33, 100, 511, 512, 513)] == [16, 16, 16, 6, 2, 1, 1]
    assert [d(n, 16, 8, 12, False).splits for n in (1, 128, 129, 180, 1023, 1024)] == [8, 8, 8, 6, 2, 1]
    assert [d(n, 16, 8, 12, False).chunks for n in (128, 129, 1024, 2047, 2048)] == [16, 16, 2, 2, 1]
    assert d(3, 93, 8, 12, True).path == "list" and d(3, 94, 8, 12, True).path == "large"  # (hit mask + word list + pixel queue in 160 KiB)
    assert not d(3, 105, 8, 12, False).windowed and d(3, 106, 8, 12, False).path_windowed
    assert not d(3, 109, 8, 12, False).hit_windowed and d(3, 110, 8, 12, False).hit_windowed


def test_dispatch_thresholds():
    _thresholds(U.dispatch)
    assert U.chunk_ranges(96, 16)[11:13] == [(88, 96), (96, 96)] and U.chunk_ranges(96, 16)[15] == (120, 96)
    assert U.mask_words(16) == 128 and U.mask_words(72) == 11712 and U.mask_words(64) == 8192


# ---------------------------------------------------------------------------
# the real plan
# ---------------------------------------------------------------------------
def _first_odd_g_without_a_slab():
    """The first odd G (G^2 odd: slabs of 32 planes) whose one aligned slab group exceeds a workgroup's LDS."""
    return next(g for g in range(17, 1025, 2) if U.slab_geometry(g).lds > U.LDS_MAX)


def _case_runs():
    for cid in sorted(U.LAUNCH_CASES):
        kw = U.LAUNCH_CASES[cid][1]
        for full_ws, large in U.workspaces_of(cid):
            yield kw["n"], kw["g"], kw["h"], kw["w"], full_ws, large


def _tuples():
    """Every (n, g, h, w, has_lists, large, slab override) the tests below look up."""
    seen = []

    def recording(n, g, h, w, full_ws, large=None):
        seen.append((n, g, h, w, full_ws, large, 0))
        return U.dispatch(n, g, h, w, full_ws, large)
    _thresholds(recording)
    seen += [run + (0,) for run in _case_runs()]
    g_out = _first_odd_g_without_a_slab()
    seen += [(3, g, 8, 12, True, "1", 0) for g in (16, 64, 100, 128)] + [(3, g, 8, 12, True, "1", k) for g, k in SLAB_OVERRIDES]
    seen += [(n, g, 8, 12, True, None, 0) for n in (3, 600) for g in (g_out - 2, g_out)] + [(3, g_out, 8, 12, True, "0", 0)]
    seen += [s + (True, None, 0) for s in WORKSPACE_SHAPES]
    return sorted(set(seen), key=repr)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """(n, g, h, w, has_lists, large, slab override) -> the plan csrc/voxel_plan.h makes, from ONE run of the sanitised dump program."""
    gxx, hipcc = shutil.which("g++"), shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cc = [gxx] if gxx else [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("voxel_plan") / "voxel_plan_dump")
    subprocess.run(cc + ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(HERE, "voxel_plan_dump.cpp"), "-o", exe], check=True)
    tuples = _tuples()
    text = "".join(f"{n} {g} {h} {w} {int(full_ws)} {LARGE[large]} {k}\n" for n, g, h, w, full_ws, large, k in tuples)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])  # (a sanitizer report goes to stderr)
    lines = run.stdout.splitlines()
    assert len(lines) == len(tuples)
    return {t: SimpleNamespace(**json.loads(l)) for t, l in zip(tuples, lines)}


def _as_dispatch(p):
    """A plan in the terms of U.dispatch."""
    return SimpleNamespace(path=p.regime, fchunks=p.fchunks, chunks=p.chunks, splits=p.splits, env_groups=p.env_groups, words=p.words,
                           hit_windowed=p.hit_windows > 1, path_windowed=p.path_windows > 1, windowed=p.hit_windows > 1 or p.path_windows > 1)


def test_plan_matches_the_restatement_for_every_gpu_case(plans):
    """Every run of every LAUNCH_CASES entry: regime, workgroups per env, words and window flags of the real plan == U.dispatch."""
    fields = ("path", "fchunks", "chunks", "splits", "env_groups", "words", "hit_windowed", "path_windowed", "windowed")
    runs = list(_case_runs())
    assert len(runs) == sum(len(U.workspaces_of(cid)) for cid in U.LAUNCH_CASES) >= len(U.LAUNCH_CASES)
    for n, g, h, w, full_ws, large in runs:
        got, want = _as_dispatch(plans[(n, g, h, w, full_ws, large, 0)]), U.dispatch(n, g, h, w, full_ws, large)
        assert [getattr(got, f) for f in fields] == [getattr(want, f) for f in fields], (n, g, h, w, full_ws, large)


def test_plan_thresholds(plans):
    """What test_dispatch_thresholds asserts of the restatement, asserted of the real plan."""
    _thresholds(lambda n, g, h, w, full_ws, large=None: _as_dispatch(plans[(n, g, h, w, full_ws, large, 0)]))


def _assert_slab(p, g, k=0):
    s = U.slab_geometry(g, k)
    assert p.regime == "large", (g, k)
    assert (p.slab_align, p.slab_planes, p.slabs, p.slab_lds, p.slab_slices) == (s.align, s.planes, s.slabs, s.lds, s.slices), (g, k)
    assert p.slab_planes % s.align == 0 and (p.slabs - 1) * p.slab_planes < g <= p.slabs * p.slab_planes and p.slab_lds <= U.LDS_MAX
    assert p.ray_grid == p.env_groups * 8 * p.slabs * p.slab_slices and p.hit_grid == p.env_groups * 8 * p.fchunks


def test_plan_slab_geometry(plans):
    """k_ray_slab's slabs against U.slab_geometry: by size, with the overrides the GPU tests set, and where no slab fits."""
    for g in (16, 64, 100, 128):
        _assert_slab(plans[(3, g, 8, 12, True, "1", 0)], g)
    # (<= 32 KiB = 262 144 bits: the whole 16^3 and 64^3 grids; 26 planes of 100^2 bits in steps of 2; 16 planes of 128^2)
    assert [plans[(3, g, 8, 12, True, "1", 0)].slab_planes for g in (16, 64, 100, 128)] == [16, 64, 26, 16]
    for g, k in SLAB_OVERRIDES:
        _assert_slab(plans[(3, g, 8, 12, True, "1", k)], g, k)
    assert any(g % plans[(3, g, 8, 12, True, "1", k)].slab_planes for g, k in SLAB_OVERRIDES)  # (heights that do not divide the grid)
    assert plans[(3, 20, 8, 12, True, "1", 2)].slab_planes == 2 and plans[(3, 33, 8, 12, True, "1", 32)].slab_planes == 32
    # the fall-through: one aligned group of 32 planes of an odd G no longer fits 160 KiB -> the round-1 window kernels
    g_out = _first_odd_g_without_a_slab()
    assert g_out == 203
    for n in (3, 600):
        _assert_slab(plans[(n, g_out - 2, 8, 12, True, None, 0)], g_out - 2)
        p = plans[(n, g_out, 8, 12, True, None, 0)]
        assert p.regime == "round1" and p.hit_windows > 1 and p.path_windows > 1 and p.slab_lds > U.LDS_MAX and p.zero_coverage
        assert U.dispatch(n, g_out, 8, 12, True).path == "round1" and U.dispatch(n, g_out - 2, 8, 12, True).path == "large"
    # (the same plan as with GENNBV_VOXEL_LARGE=0, bar the slab it looked at)
    p, forced = plans[(3, g_out, 8, 12, True, None, 0)], plans[(3, g_out, 8, 12, True, "0", 0)]
    assert all(getattr(p, f) == getattr(forced, f) for f in vars(p) if not f.startswith("slab"))


def test_plan_windows_and_fills(plans):
    """Windows cover the mask with <= 128 KiB each; the span zeroed in front of the launches lies inside the workspace."""
    for (n, g, h, w, full_ws, large, k), p in plans.items():
        assert p.words == U.mask_words(g) and p.hit_nw * p.hit_windows >= p.words and p.path_nw * p.path_windows >= p.words
        assert p.hit_lds == 4 * p.hit_nw <= U.LDS_MAX and p.path_lds == 4 * (p.path_nw + U.K_QUEUE_CAP + 32) <= U.LDS_MAX
        if p.hit_windows > 1:
            assert 4 * p.hit_nw <= 128 * 1024
        masks, counts = 2 * n * p.words * 4, p.ray_count_ints * 4
        if p.regime == "round1":
            assert (p.zero_offset, p.zero_bytes, p.zero_coverage) == (0, masks if p.splits > 1 else masks // 2, 1)
        else:  # [hit (only when several workgroups OR into it) | path | ray counts] in one fill
            assert full_ws and p.zero_coverage == 0 and p.zero_offset + p.zero_bytes == masks + counts <= p.ws_bytes_hw
            assert p.zero_offset == (masks // 2 if p.regime == "list" and p.fchunks == 1 else 0)


def test_plan_workspace_bytes(plans):
    """gnbv_voxel_workspace_bytes[_hw]: two mask arrays of 64-word-padded rows; + ray counts (padded to 64) + h*w (padded to 64) list
    entries per env."""
    for n, g, h, w in WORKSPACE_SHAPES:
        p = plans[(n, g, h, w, True, None, 0)]
        words = -(-(-(-g ** 3 // 32)) // 64) * 64
        assert p.ws_bytes == 2 * n * words * 4
        assert p.ray_count_ints == -(-n // 64) * 64 and p.ray_list_cap == -(-h * w // 64) * 64
        assert p.ws_bytes_hw == p.ws_bytes + 4 * (p.ray_count_ints + n * p.ray_list_cap)

"""CPU: the numpy reference of gnbv_cover_greedy -- its lazy form equals its exhaustive form; the new entry points are declared,
exported and bound and refuse bad arguments before any launch; ViewPool and PoolCoverPolicy refuse what they cannot run."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import cover_greedy_oracle as CG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, H, W = 16, 24, 32
CFG = TaskConfig(camera_width=W, camera_height=H, grid_size=G)


def test_lazy_reference_equals_exhaustive_reference():
    """300 seeded cases with ties, duplicated and empty masks, no / random / all contacts and 1..8 evaluations per pass: the
    same choices, gains and covered sets, and the bounds at exit are upper bounds of the gains against the final set."""
    rng = np.random.default_rng(0)
    evals = total = 0
    for trial in range(300):
        k, words, waves = int(rng.integers(1, 40)), int(rng.integers(1, 9)), int(rng.integers(1, 9))
        rounds = int(rng.integers(1, k + 4))
        m = CG.random_masks(rng, k, words, rng.choice([0.02, 0.2, 0.5]))
        if k > 3:
            m[rng.integers(k)] = m[rng.integers(k)]
            m[rng.integers(k)] = 0
        cov = CG.random_masks(rng, 1, words, 0.3)[0]
        contact = np.zeros(k, np.uint8)
        if trial % 3 == 1:
            contact = (rng.random(k) < 0.3).astype(np.uint8)
        if trial % 3 == 2:
            contact[:] = 1
        a = CG.exhaustive(m, cov, contact, rounds)
        b = CG.lazy(m, cov, contact, rounds, waves=waves)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), trial
        assert (b[3] >= CG.popcount(m & ~b[2])).all(), trial
        # carried bounds: rounds split over two calls equal one call
        r1 = rounds // 2
        if r1 >= 1:
            c = CG.lazy(m, cov, contact, r1, waves=waves)
            d = CG.lazy(m, c[2], contact, rounds - r1, ub=c[3], waves=waves)
            assert np.array_equal(np.concatenate([c[0], d[0]]), a[0]) and np.array_equal(np.concatenate([c[1], d[1]]), a[1])
            assert np.array_equal(d[2], a[2])
        evals += b[4]
        total += k * rounds
    print("lazy evaluations", evals, "of", total)
    assert evals < total


def test_reference_rules_on_a_hand_made_case():
    m = np.array([[0b0011], [0b1100], [0b0111], [0b0111], [0]], np.uint32)
    none, zero = np.zeros(5, np.uint8), np.zeros(1, np.uint32)
    ch, gn, cov, g0 = CG.exhaustive(m, zero, none, 4)
    assert ch.tolist() == [2, 1, 0, 0] and gn.tolist() == [3, 1, 0, 0] and cov.tolist() == [0b1111]  # tie 2/3 -> 2; repeats at gain 0
    assert g0.tolist() == [2, 2, 3, 3, 0]
    ch, gn, _, _ = CG.exhaustive(m, zero, np.array([0, 0, 1, 1, 0], np.uint8), 2)
    assert ch.tolist() == [0, 1] and gn.tolist() == [2, 2]
    ch, gn, _, _ = CG.exhaustive(m[1:], zero, np.ones(4, np.uint8), 2)  # all in contact: index 0, its true gain
    assert ch.tolist() == [0, 0] and gn.tolist() == [2, 0]


def test_header_declares_and_library_exports_the_new_entry_points():
    from gennbv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gennbv_hip.h")).read()
    assert re.search(r"\bint\s+gnbv_view_cover_masks\s*\(\s*const\s+GnbvMeshScene\s*\*", hdr)
    assert re.search(r"\bint\s+gnbv_cover_greedy\s*\(\s*const\s+GnbvCoverGreedy\s*\*", hdr)
    assert _lib.SIGNATURES["gnbv_view_cover_masks"] == (C.c_int, [C.c_void_p] * 4)
    assert _lib.SIGNATURES["gnbv_cover_greedy"] == (C.c_int, [C.c_void_p] * 2)
    lib = _lib.load()
    assert lib.gnbv_view_cover_masks is not None and lib.gnbv_cover_greedy is not None
    assert lib.gnbv_abi_version() == 5
    body = re.search(r"typedef struct GnbvCoverGreedy \{(.*?)\} GnbvCoverGreedy;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [re.split(r"[\s\*]+", n)[-1] for n in names]
    assert names == [f[0] for f in _lib.GnbvCoverGreedy._fields_]
    from gennbv_amd.csrc import build
    assert "covergreedy.hip" in build.SOURCES


def test_invalid_arguments_are_refused_before_any_launch():
    """Argument checks come first, so the refusals can be seen without a GPU (the pointers are never dereferenced)."""
    from gennbv_amd import _lib
    lib = _lib.load()
    sc, a = _lib.GnbvMeshScene(), _lib.GnbvViewCover()
    assert lib.gnbv_view_cover_masks(None, C.byref(a), 16, None) == 1  # hipErrorInvalidValue
    assert lib.gnbv_view_cover_masks(C.byref(sc), None, 16, None) == 1
    sc.n = 2
    a.n, a.k, a.g, a.h, a.w, a.stride = 2, 1, 16, H, W, 1
    assert lib.gnbv_view_cover_masks(C.byref(sc), C.byref(a), None, None) == 1
    assert lib.gnbv_view_cover_masks(C.byref(sc), C.byref(a), 16, None) == 1  # NULL poses, ...

    def args(**kw):
        c = _lib.GnbvCoverGreedy()
        c.n, c.k, c.words, c.rounds, c.lazy = 2, 3, 8, 2, 1
        c.mask_bits, c.choice, c.gain, c.covered_out = 4096, 4096, 4096, 4096  # (aligned, never dereferenced: a refusal comes first)
        for f, v in kw.items():
            setattr(c, f, v)
        return c
    assert lib.gnbv_cover_greedy(None, None) == 1
    for kw in (dict(n=0), dict(n=65536), dict(k=0), dict(k=4097), dict(rounds=0), dict(rounds=4097), dict(words=0), dict(words=6),
               dict(words=-4), dict(lazy=2), dict(mask_bits=None), dict(choice=None), dict(gain=None), dict(covered_out=None),
               dict(mask_bits=4100), dict(covered_in=4104), dict(covered_out=4100)):
        assert lib.gnbv_cover_greedy(C.byref(args(**kw)), None) == 1, kw


class _Updater:
    def __init__(self, n, packed=True):
        self.packed = packed
        self.gt_bits = torch.full((n, 64), -1, dtype=torch.int32)
        self.scanned_bits = torch.zeros(n, 64, dtype=torch.int32)


class _Env:
    def __init__(self, n, packed=True):
        self.cfg, self.num_envs, self.device = CFG, n, torch.device("cpu")
        self.collision, self.collision_mesh = None, None
        self.updater = _Updater(n, packed)
        self.feed = object()


def test_view_pool_and_policy_refuse_what_they_cannot_run():
    from gennbv_amd import _lib
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.eval.baselines import PoolCoverPolicy
    from gennbv_amd.ops.view_pool import ViewPool
    sc = S.make_scenes(2, G, seed=1)
    mesh = MeshScene.from_boxes(sc, device="cpu")
    words = int(_lib.load().gnbv_grid_bit_words(G))
    gt = torch.zeros(2, words, dtype=torch.int32)
    with pytest.raises(_lib.GennbvHipError):
        ViewPool(mesh, CFG, sc.range_gt, sc.voxel_size, gt, torch.zeros(2, 4, 6))
    with pytest.raises(_lib.GennbvHipError):
        PoolCoverPolicy(_Env(2, packed=False), pool_size=4)
    with pytest.raises(_lib.GennbvHipError):
        PoolCoverPolicy(_Env(2), pool_size=4)  # env.feed has no mesh

    class _CudaMesh:  # the size checks come before anything touches the device
        device, num_envs = torch.device("cuda:0"), 2
    with pytest.raises(_lib.GennbvHipError, match=str(2 * 4 * words * 4)):
        ViewPool(_CudaMesh(), CFG, sc.range_gt, sc.voxel_size, gt, torch.zeros(2, 4, 6), max_bytes=1024)
    with pytest.raises(_lib.GennbvHipError):
        ViewPool(_CudaMesh(), TaskConfig(camera_width=W, camera_height=H, grid_size=129), sc.range_gt, sc.voxel_size, gt, torch.zeros(2, 4, 6))

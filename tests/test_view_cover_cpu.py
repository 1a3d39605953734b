"""CPU: the view-coverage entry point is declared, exported and bound; ViewCover refuses the CPU; OracleGainPolicy's decision
with an injected cover backend (the injection point exists for tests; the product path has no CPU fallback); the headers of
the shared trace are build dependencies."""
import ctypes as C
import os
import re

import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, H, W = 16, 24, 32
CFG = TaskConfig(camera_width=W, camera_height=H, grid_size=G)


def test_header_declares_and_library_exports_view_cover():
    from gennbv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gennbv_hip.h")).read()
    assert re.search(r"\bint\s+gnbv_view_cover\s*\(\s*const\s+GnbvMeshScene\s*\*", hdr)
    assert "typedef struct GnbvViewCover" in hdr
    assert "gnbv_view_cover" in _lib.SIGNATURES
    lib = C.CDLL(_lib.LIB_PATH)
    assert getattr(lib, "gnbv_view_cover") is not None  # AttributeError if the symbol is not exported
    assert _lib.load().gnbv_abi_version() == 5
    # the struct binding follows the header's field order
    body = re.search(r"typedef struct GnbvViewCover \{(.*?)\} GnbvViewCover;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [re.split(r"[\s\*]+", n)[-1] for n in names]
    assert names == [f[0] for f in _lib.GnbvViewCover._fields_]


def test_invalid_arguments_are_refused_before_any_launch():
    """Argument checks come first, so the refusals can be seen without a GPU."""
    from gennbv_amd import _lib
    lib = _lib.load()
    sc, a = _lib.GnbvMeshScene(), _lib.GnbvViewCover()
    assert lib.gnbv_view_cover(None, C.byref(a), None) == 1  # hipErrorInvalidValue
    assert lib.gnbv_view_cover(C.byref(sc), None, None) == 1
    sc.n = 2
    a.n, a.k, a.g, a.h, a.w, a.stride = 3, 1, 16, H, W, 1
    assert lib.gnbv_view_cover(C.byref(sc), C.byref(a), None) == 1  # scene->n != n, and NULL pointers


def test_view_cover_rejects_cpu():
    from gennbv_amd import _lib
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.ops.view_cover import ViewCover
    sc = S.make_scenes(2, G, seed=1)
    mesh = MeshScene.from_boxes(sc, device="cpu")
    with pytest.raises(_lib.GennbvHipError):
        ViewCover(mesh, CFG, sc.range_gt, sc.voxel_size, 4)
    with pytest.raises(_lib.GennbvHipError):
        ViewCover(mesh, CFG, sc.range_gt, sc.voxel_size, 4, device="cpu")
    with pytest.raises(_lib.GennbvHipError):
        mesh.observable_ground_truth(G, torch.zeros(2, 4, 6), CFG, base=sc)


class _Mesh:
    def collide_candidates(self, poses, body, out=None):
        out.copy_((poses[..., 2] < 3.0).to(torch.uint8))  # "everything below 3 m collides"
        return out


class _Updater:
    def __init__(self, n, packed=True):
        self.packed = packed
        self.gt_bits = torch.full((n, 64), -1, dtype=torch.int32)
        self.scanned_bits = torch.zeros(n, 64, dtype=torch.int32)


class _Env:
    def __init__(self, n, collision, packed=True):
        self.cfg, self.num_envs, self.device = CFG, n, torch.device("cpu")
        self.collision, self.collision_mesh = collision, _Mesh()
        self.updater = _Updater(n, packed)
        self.feed = object()


def _backend_from(table, seen):
    def backend(poses, gt_bits, scanned_bits):
        seen.append((poses, gt_bits, scanned_bits))
        return table
    return backend


def test_oracle_policy_picks_argmax_new_gt_ties_low_and_avoids_contacts():
    from gennbv_amd.eval.baselines import LatticeCandidates, OracleGainPolicy
    n, k = 3, 6
    cover = torch.zeros(n, k, 3, dtype=torch.int32)
    cover[0, :, 0] = torch.tensor([1, 9, 3, 9, 0, 2])      # argmax 9 at 1 and 3 -> 1 (tie: lowest)
    cover[1, :, 0] = torch.tensor([0, 0, 0, 0, 0, 7])      # -> 5
    cover[2, :, 0] = torch.tensor([4, 4, 4, 4, 4, 4])      # -> 0
    cover[..., 1] = torch.tensor([100, 0, 0, 0, 0, 0])     # seen_gt and hits must not enter the score
    cover[..., 2] = torch.tensor([0, 0, 0, 0, 1000, 0])
    obs = torch.zeros(n, CFG.obs_dim)
    seen = []
    env = _Env(n, None)
    pol = OracleGainPolicy(env, k=k, seed=5, cover_backend=_backend_from(cover, seen))
    actions, x, y = pol.policy(obs, deterministic=True)
    cand = LatticeCandidates(CFG, k, 5).sample(n)
    assert x is None and y is None
    assert torch.equal(actions, cand[torch.arange(n), torch.tensor([1, 5, 0])])
    assert actions.dtype == torch.int64 and actions.shape == (n, 6)
    lo, up = torch.tensor(CFG.clip_pose_idx_low), torch.tensor(CFG.clip_pose_idx_up)
    assert bool((actions >= lo).all()) and bool((actions <= up).all())
    assert pol.last_cover is cover
    poses, gt_bits, scanned_bits = seen[0]
    assert torch.equal(poses, S.poses_from_actions(cand, CFG).float()) and poses.shape == (n, k, 6)
    assert gt_bits is env.updater.gt_bits and scanned_bits is env.updater.scanned_bits
    a2, state = pol.predict(obs)
    assert state is None and a2.shape == (n, 6) and len(seen) == 2


def test_oracle_policy_never_picks_a_contact_unless_all_are():
    from gennbv_amd.eval.baselines import LatticeCandidates, OracleGainPolicy
    n, k = 4, 8
    obs = torch.zeros(n, CFG.obs_dim)
    gen = torch.Generator().manual_seed(0)
    cover = torch.randint(0, 50, (n, k, 3), generator=gen, dtype=torch.int32)
    for seed in range(6):
        pol = OracleGainPolicy(_Env(n, object()), k=k, seed=seed, cover_backend=_backend_from(cover, []))
        actions = pol(obs)[0]
        cand = LatticeCandidates(CFG, k, seed).sample(n)
        hit = S.poses_from_actions(cand, CFG)[..., 2] < 3.0
        score = torch.where(hit, torch.full_like(cover[..., 0], -1), cover[..., 0]).long()
        want = torch.stack([cand[e, int(torch.nonzero(score[e] == score[e].max())[0])] for e in range(n)])
        assert torch.equal(actions, want)
        chosen_hit = torch.stack([hit[e, int(torch.nonzero(score[e] == score[e].max())[0])] for e in range(n)])
        assert not bool((chosen_hit & ~hit.all(1)).any())
    # avoid_collisions=False: the contacts are not consulted
    pol = OracleGainPolicy(_Env(n, object()), k=k, seed=0, avoid_collisions=False, cover_backend=_backend_from(cover, []))
    cand = LatticeCandidates(CFG, k, 0).sample(n)
    assert torch.equal(pol(obs)[0], cand[torch.arange(n), cover[..., 0].long().argmax(1)])


def test_oracle_policy_refuses_an_unpacked_updater_and_a_feed_without_mesh():
    from gennbv_amd import _lib
    from gennbv_amd.eval.baselines import OracleGainPolicy
    with pytest.raises(_lib.GennbvHipError):
        OracleGainPolicy(_Env(2, None, packed=False), k=4, cover_backend=lambda *a: None)
    with pytest.raises(_lib.GennbvHipError):
        OracleGainPolicy(_Env(2, None), k=4)  # no backend injected and env.feed has no mesh


def test_trace_headers_are_build_dependencies_and_the_trace_is_stated_once():
    from gennbv_amd.csrc import build
    listed = {os.path.normpath(os.path.join(build.HERE, h)) for h in build.HEADERS}
    for src in ("viewcover.hip", "render.hip"):
        assert src in build.SOURCES
        text = open(os.path.join(build.HERE, src)).read()
        incs = re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M)
        assert "raytrace.h" in incs, src
        for inc in incs:
            assert os.path.normpath(os.path.join(build.HERE, inc)) in listed, (src, inc)
        assert "trace_pixel(" in text and "cell_tris" not in text.split("GNBV_API")[0], src  # no second copy of the DDA

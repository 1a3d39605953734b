"""GPU: gnbv_collide_cylinder_batch / MeshScene.collide_candidates ([N,K] poses, one launch) against the K column calls of
MeshScene.collide, bit for bit, and the greedy policy's decisions through either."""
import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import test_collision_gpu as TC
from tests import test_view_gain_gpu as TV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _columns(mesh, poses, body):
    return torch.stack([mesh.collide(poses[:, j], body) for j in range(poses.shape[1])], 1)


@pytest.mark.parametrize("ground", [False, True])
def test_box_scenes_equal_the_column_calls(ground):
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.eval.baselines import LatticeCandidates
    n, k = 16, 32
    cfg = TaskConfig(grid_size=20)
    mesh = MeshScene.from_boxes(S.make_scenes(n, 20, seed=1), device=DEV)
    lc = LatticeCandidates(cfg, k, seed=5)
    poses = lc.poses(lc.sample(n)).to(DEV)
    body = CollisionBody(TC.R, TC.H, ground)
    want = _columns(mesh, poses, body)
    got = mesh.collide_candidates(poses, body)
    assert got.shape == (n, k) and got.dtype == torch.uint8
    assert torch.equal(got, want)
    codes = want.cpu().numpy()
    print("codes", np.bincount(codes.ravel(), minlength=8))
    assert (codes == 0).any() and (codes != 0).any()
    # rows inside a wider buffer (stride 8), a preallocated output, two calls
    wide = torch.full((n, k, 8), float("nan"), device=DEV)
    wide[..., :6] = poses
    out = torch.full((n, k), 77, dtype=torch.uint8, device=DEV)
    assert mesh.collide_candidates(wide[..., :6], body, out=out) is out
    assert torch.equal(out, want)
    assert torch.equal(mesh.collide_candidates(wide[..., :6], body), want)
    # a NaN pose scores 0 and disturbs no other
    bad = poses.clone()
    bad[3, 7, 1] = float("nan")
    bad[5, 0, 4] = float("inf")
    got = mesh.collide_candidates(bad, body)
    assert int(got[3, 7]) == 0 and int(got[5, 0]) == 0
    keep = torch.ones(n, k, dtype=torch.bool, device=DEV)
    keep[3, 7] = keep[5, 0] = False
    assert torch.equal(got[keep], want[keep])
    # K = 1
    assert torch.equal(mesh.collide_candidates(poses[:, 3:4], body), want[:, 3:4])
    assert torch.equal(mesh.collide_candidates(poses[:, 3:4].contiguous(), body), want[:, 3:4])


def test_sphere_and_mixed_scenes_near_the_surface_equal_the_column_calls():
    from gennbv_amd.env.collision import CollisionBody
    tris, ids = TC._test_scenes()  # boxes, rotated boxes, spheres (sphere_triangles), degenerate triangles, an empty env
    mesh = TC._mesh(tris, ids)
    n, k = mesh.num_envs, 48
    gen = torch.Generator().manual_seed(3)
    for lattice in (False, True):
        poses = torch.from_numpy(np.stack([TC._near_surface_poses(tris[e].numpy(), k, gen, lattice) for e in range(n)])).to(DEV)
        for ground in (False, True):
            body = CollisionBody(TC.R, TC.H, ground)
            want = _columns(mesh, poses, body)
            assert torch.equal(mesh.collide_candidates(poses, body), want)
            codes = want.cpu().numpy()
            print("codes", np.bincount(codes.ravel(), minlength=8))
            assert (codes & 1).any() and (codes == 0).any()
            assert (codes[10:12] != 0).any() and (codes[10:12] == 0).any()  # the sphere envs


def test_refusals_by_return_code():
    import ctypes as C
    from gennbv_amd import _lib
    from gennbv_amd.env.mesh_scene import MeshScene
    mesh = MeshScene.from_boxes(S.make_scenes(2, 20, seed=1), device=DEV)
    lib = _lib.load()
    sc, ob = mesh.c_struct(), mesh.objects_c_struct()
    poses = torch.zeros(2, 4, 6, device=DEV)
    out = torch.zeros(2, 4, dtype=torch.uint8, device=DEV)

    def call(k=4, stride=6, radius=0.1, half=0.02, p=poses.data_ptr(), o=out.data_ptr()):
        return lib.gnbv_collide_cylinder_batch(C.byref(sc), C.byref(ob), p, k, stride, radius, half, 0, o, None)
    assert call() == 0
    for kw in (dict(k=0), dict(k=-1), dict(stride=5), dict(radius=0.0), dict(half=float("nan")), dict(p=None), dict(o=None)):
        assert call(**kw) == 1, kw  # hipErrorInvalidValue
    with pytest.raises(_lib.GennbvHipError):
        MeshScene.from_boxes(S.make_scenes(2, 20, seed=1), device="cpu").collide_candidates(torch.zeros(2, 4, 6), None)
    with pytest.raises(_lib.GennbvHipError):
        mesh.collide_candidates(torch.zeros(2, 4, 6), None)  # poses on the host


class _ColumnsOnly:
    """A collision mesh that exposes `collide` alone: the policy falls back to one call per candidate column."""

    def __init__(self, mesh):
        self._mesh = mesh
        self.calls = 0

    def collide(self, poses, body, out=None):
        self.calls += 1
        return self._mesh.collide(poses, body, out=out)


def test_greedy_policy_decides_the_same_through_either_query():
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.eval.baselines import GreedyGainPolicy
    n, k = 8, 32
    env_a, _, _ = TV._closed_env(n=n, collision=CollisionBody(), eval_env=False)
    env_b, _, _ = TV._closed_env(n=n, collision=CollisionBody(), eval_env=False)
    assert hasattr(env_a.collision_mesh, "collide_candidates")
    proxy = _ColumnsOnly(env_b.collision_mesh)
    env_b.collision_mesh = proxy
    pa, pb = GreedyGainPolicy(env_a, k=k, seed=7), GreedyGainPolicy(env_b, k=k, seed=7)
    assert pa.avoid_collisions and pb.avoid_collisions
    oa, ob = env_a.reset(), env_b.reset()
    for step in range(5):
        a, b = pa(oa)[0], pb(ob)[0]
        assert torch.equal(a, b), step
        assert torch.equal(pa._contact, pb._contact.t())
        oa, ob = env_a.step(a)[0], env_b.step(b)[0]
        assert torch.equal(oa, ob)
    assert proxy.calls >= 5 * k
    assert bool(pa._contact.any())  # some candidate did collide: the query mattered

"""GPU: gnbv_view_gain_slab / ViewGainSlab (csrc/viewgain.hip: the rays' fates, then slabs of x-planes; grids up to 128^3)
against the CPU oracle (tests/view_gain_oracle.py) and against the shipped LDS kernel, exactly; make_view_gain; the greedy
baseline at 128^3.  The inputs are built as tests/test_view_gain_gpu.py builds its own."""
import ctypes as C

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from tests import test_view_gain_gpu as TV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slab_op(cfg, scene, n, k, stride, range_m, chunk=0, slab=0, with_c2w=True):
    from gennbv_amd.ops.view_gain import ViewGainSlab
    return ViewGainSlab(n, k, cfg, scene.range_gt, scene.voxel_size, stride=stride, range_m=range_m, device=DEV,
                        with_c2w=with_c2w, chunk=chunk, slab=slab)


def _inputs(g, cam, n, k, occ, kind, seed=2):
    cfg = TV._cfg(cam[0], cam[1], g)
    scene = S.make_scenes(n, g, seed=seed)
    tri = torch.zeros(n, g ** 3, dtype=torch.int8) if occ is None else TV._random_tri(n, g, occ, seed=g + n)
    poses = TV._lattice_poses(cfg, n, k, seed=g) if kind == "lattice" else TV._outside_poses(n, k)
    return cfg, scene, tri, poses


CASES = [  # g, (h, w), stride, range, n, k, occupied density (None: all unknown), poses, a slab height that does not divide g
    (65, (60, 80), 4, 50.0, 2, 5, 0.01, "lattice", 24),
    (72, (60, 80), 4, 2.0, 3, 4, 0.05, "lattice", 5),
    (96, (240, 320), 8, 50.0, 1, 5, 0.005, "outside", 5),
    (100, (60, 80), 4, 50.0, 2, 4, None, "lattice", 24),
    (128, (240, 320), 4, 50.0, 1, 5, 0.002, "lattice", 24),
    (128, (400, 400), 8, 50.0, 1, 3, None, "lattice", 5),
    (128, (60, 80), 4, 2.0, 5, 3, 0.05, "lattice", 24),
    (128, (240, 320), 8, 50.0, 1, 7, 0.01, "outside", 5),
    # rays of more than 2^14 steps: the slab set-up's 64-bit form (shorter rays take the 32-bit one)
    (72, (60, 80), 4, 3000.0, 2, 4, 0.02, "lattice", 5),
    # a lattice of exactly one wave (64 rays), and one of 4 800 rays: no whole number of waves, more than one turn of 1 024 lanes
    (65, (8, 8), 1, 50.0, 2, 5, 0.05, "lattice", 24),
    (65, (60, 80), 1, 50.0, 2, 5, 0.05, "lattice", 24),
]


@pytest.mark.parametrize("g,cam,stride,range_m,n,k,occ,kind,odd", CASES)
def test_kernel_equals_oracle(g, cam, stride, range_m, n, k, occ, kind, odd):
    cfg, scene, tri, poses = _inputs(g, cam, n, k, occ, kind)
    assert g % odd != 0
    tri_d, poses_d = tri.to(DEV), poses.to(DEV)
    want = None
    for slab in (0, odd):
        for chunk in (0, 2):
            vg = _slab_op(cfg, scene, n, k, stride, range_m, chunk, slab)
            gain = vg(tri_d, poses_d).cpu().numpy()
            if want is None:
                want = TV._oracle(cfg, scene, tri, vg.c2w.cpu().numpy(), stride, range_m)
                sums = want.sum(axis=(0, 1))
                print("oracle sums", sums)
                assert sums[0] > 0
                assert (sums[1] > 0 and sums[2] > 0) if occ is not None else (sums[1] == 0 and sums[2] == 0)
            print("slab", slab, "chunk", chunk, "gain sums", gain.sum(axis=(0, 1)))
            assert np.array_equal(gain, want), (slab, chunk)


@pytest.mark.parametrize("g,cam,stride,range_m,n,k,occ,kind", [
    (20, (60, 80), 1, 50.0, 1, 5, 0.01, "lattice"),
    (20, (240, 320), 4, 50.0, 1, 7, 0.05, "outside"),
    (20, (60, 80), 4, 50.0, 37, 3, None, "lattice"),
    (33, (240, 320), 8, 50.0, 1, 5, 0.02, "outside"),
    (33, (60, 80), 4, 2.0, 1, 5, 0.10, "lattice"),
    (64, (240, 320), 4, 50.0, 1, 5, 0.005, "lattice"),
    (64, (60, 80), 4, 2.0, 37, 3, 0.05, "lattice"),
    (64, (240, 320), 8, 50.0, 1, 7, 0.02, "outside"),
])
def test_slab_path_equals_the_lds_kernel(g, cam, stride, range_m, n, k, occ, kind):
    """Seams in the middle of grids whose answer the shipped kernel gives."""
    cfg, scene, tri, poses = _inputs(g, cam, n, k, occ, kind)
    tri_d, poses_d = tri.to(DEV), poses.to(DEV)
    _, want, c2w = TV._run(cfg, scene, tri, poses, stride, range_m)
    assert want[..., 0].sum() > 0
    for slab in (1, 3, 7, 16, g):
        vg = _slab_op(cfg, scene, n, k, stride, range_m, chunk=0 if slab != 7 else 2, slab=slab)
        got = vg(tri_d, poses_d)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), slab
        assert np.array_equal(vg.c2w.cpu().numpy().view(np.uint32), c2w.view(np.uint32))


def test_env_batches_equal_the_lds_kernel():
    """Enough rays that the call runs its envs in several batches over the one workspace (one ray per pixel, 24 envs:
    20 bytes x 76 800 rays x 8 candidates per env against the 128 MiB the records of a batch may take)."""
    from gennbv_amd.ops.view_gain import ViewGain
    g, n, k = 20, 24, 8
    cfg, scene, tri, poses = _inputs(g, (240, 320), n, k, 0.03, "lattice")
    tri_d, poses_d = tri.to(DEV), poses.to(DEV)
    want = ViewGain(n, k, cfg, scene.range_gt, scene.voxel_size, stride=1, device=DEV)(tri_d, poses_d)
    vg = _slab_op(cfg, scene, n, k, 1, None, slab=7)
    assert vg.workspace_bytes < n * k * 76800 * 20 // 2  # fewer than half the envs at a time
    assert torch.equal(vg(tri_d, poses_d), want)
    assert int(want[..., 2].sum()) > 0 and int(want[..., 0].sum()) > 0


def test_outputs_overwritten_deterministic_strided_and_fp32():
    g, n, k = 72, 5, 7
    cfg, scene, _, _ = _inputs(g, (60, 80), n, k, None, "lattice", seed=4)
    tri = TV._random_tri(n, g, 0.03, seed=1).to(DEV)
    poses = TV._lattice_poses(cfg, n, k, seed=5).to(DEV)
    vg = _slab_op(cfg, scene, n, k, 4, None, chunk=3)
    vg.gain.fill_(-12345)
    vg.c2w.fill_(float("nan"))
    a = vg(tri, poses).clone()
    assert not bool((a == -12345).any()) and not bool(torch.isnan(vg.c2w).any())
    assert int(a[..., 0].sum()) > 0 and int(a[..., 2].sum()) > 0
    vg.gain.fill_(-12345)
    assert torch.equal(vg(tri, poses), a)
    assert torch.equal(vg(tri, poses), a)
    big = torch.full((n, g ** 3 + 13), 1, dtype=torch.int8, device=DEV)  # rows inside a larger buffer, unaligned stride
    big[:, 5:5 + g ** 3] = tri
    assert torch.equal(vg(big[:, 5:5 + g ** 3], poses), a)
    assert torch.equal(vg(tri.float(), poses), a)
    assert torch.equal(vg(tri.view(n, g, g, g), poses), a)
    for slab, chunk in ((1, 1), (5, 7), (16, 2), (72, 0), (1000, 4)):
        assert torch.equal(_slab_op(cfg, scene, n, k, 4, None, chunk, slab, with_c2w=False)(tri, poses), a), (slab, chunk)


def test_refusals_by_return_code():
    from gennbv_amd import _lib
    from gennbv_amd.ops.view_gain import ViewGainSlab
    g = 72
    scene = S.make_scenes(2, g, seed=1)
    cfg = TV._cfg(60, 80, g)
    with pytest.raises(_lib.GennbvHipError):
        ViewGainSlab(2, 4, cfg, scene.range_gt, scene.voxel_size, device="cpu")
    with pytest.raises(_lib.GennbvHipError):
        ViewGainSlab(2, 4, TV._cfg(60, 80, 129), scene.range_gt, scene.voxel_size, device=DEV)
    vg = ViewGainSlab(2, 4, cfg, scene.range_gt, scene.voxel_size, device=DEV)
    with pytest.raises(_lib.GennbvHipError):
        vg(torch.zeros(2, g ** 3, dtype=torch.int8), torch.zeros(2, 4, 6))
    tri, poses = torch.zeros(2, g ** 3, dtype=torch.int8, device=DEV), torch.zeros(2, 4, 6, device=DEV)
    vg(tri, poses)
    lib = _lib.load()
    need = lib.gnbv_view_gain_slab_workspace_bytes(2, 4, g, 60, 80, 4)
    assert need == vg.workspace_bytes > 0
    assert lib.gnbv_view_gain_slab_workspace_bytes(2, 4, 129, 60, 80, 4) == 0
    ws = vg.workspace.data_ptr()
    assert lib.gnbv_view_gain_slab(C.byref(vg._args), 0, ws, need, None) == 0
    for field, bad in (("stride", 0), ("range", 0.0), ("range", float("inf")), ("k", 0), ("g", 129), ("n", 0)):
        a = _lib.GnbvViewGain()
        C.memmove(C.byref(a), C.byref(vg._args), C.sizeof(a))
        setattr(a, field, bad)
        assert lib.gnbv_view_gain_slab(C.byref(a), 0, ws, need, None) == 1, field  # hipErrorInvalidValue
    assert lib.gnbv_view_gain_slab(C.byref(vg._args), 0, None, need, None) == 1
    assert lib.gnbv_view_gain_slab(C.byref(vg._args), 0, ws, need - 1, None) == 1
    assert lib.gnbv_view_gain_slab(C.byref(vg._args), -1, ws, need, None) == 1
    assert lib.gnbv_view_gain_slab(None, 0, ws, need, None) == 1


def test_make_view_gain_picks_the_path():
    from gennbv_amd.ops.view_gain import ViewGain, ViewGainSlab, make_view_gain
    scene = S.make_scenes(2, 20, seed=1)
    for g, cls in ((20, ViewGain), (64, ViewGain), (65, ViewGainSlab), (128, ViewGainSlab)):
        vg = make_view_gain(2, 4, TV._cfg(60, 80, g), scene.range_gt, scene.voxel_size, device=DEV, slab=5)
        assert type(vg) is cls, g
        assert tuple(vg.gain.shape) == (2, 4, 3)


def _closed_env_128(n, seed=1, max_len=50):
    return TV._closed_env(n=n, g=128, max_len=max_len, seed=seed, eval_env=False)


def test_rollout_grids_at_128_equal_oracle_and_camera_equals_renderer():
    """The grids of a closed-loop rollout at 128^3 after 1, 5 and 12 steps; c2w_out bit-equal to the renderer's camera."""
    from gennbv_amd.eval.baselines import RandomLatticePolicy
    n, k = 3, 4
    env, cfg, scene = _closed_env_128(n)
    pol = RandomLatticePolicy(cfg, n, seed=3)
    obs = env.reset()
    poses = TV._lattice_poses(cfg, n, k, seed=9)
    vg = _slab_op(cfg, scene, n, k, 4, 50.0, chunk=3)
    for step in range(1, 13):
        obs, _, _, _ = env.step(pol(obs)[0])
        if step in (1, 5, 12):
            tri = obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]
            gain = vg(tri, poses.to(DEV)).cpu().numpy()
            want = TV._oracle(cfg, scene, tri.cpu(), vg.c2w.cpu().numpy(), 4, 50.0)
            print("step", step, "oracle sums", want.sum(axis=(0, 1)))
            assert np.array_equal(gain, want), step
            assert want[..., 2].sum() > 0 and want[..., 0].sum() > 0
    c2w = vg.c2w.cpu().numpy()
    for j in range(k):
        cam = env.feed.render(poses[:, j].contiguous().to(DEV))[3].cpu().numpy()
        assert np.array_equal(cam.view(np.uint32), c2w[:, j].view(np.uint32)), j


def test_greedy_policy_at_128_chooses_the_oracle_policy_actions():
    from gennbv_amd.eval.baselines import GreedyGainPolicy
    from gennbv_amd.ops.view_gain import ViewGainSlab
    n, k, stride = 2, 6, 4
    env_a, cfg, scene = _closed_env_128(n)
    env_b, _, _ = _closed_env_128(n)
    pa = GreedyGainPolicy(env_a, k=k, seed=7)
    assert type(pa.gain_backend) is ViewGainSlab
    cams = _slab_op(cfg, scene, n, k, stride, None)  # supplies the camera matrices only

    def backend(tri, poses):
        cams(tri, poses)
        want = TV._oracle(cfg, scene, tri.to(torch.int8).cpu(), cams.c2w.cpu().numpy(), stride, abs(cfg.depth_sense_dist))
        return torch.from_numpy(want).to(tri.device)
    pb = GreedyGainPolicy(env_b, k=k, seed=7, gain_backend=backend)
    oa, ob = env_a.reset(), env_b.reset()
    for step in range(4):
        a, b = pa(oa)[0], pb(ob)[0]
        assert int(pa.last_gain[..., 0].sum()) > 0
        assert torch.equal(pa.last_gain.cpu(), pb.last_gain.cpu()), step
        assert torch.equal(a, b), step
        oa, ob = env_a.step(a)[0], env_b.step(b)[0]
        assert torch.equal(oa, ob)

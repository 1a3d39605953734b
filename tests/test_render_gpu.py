"""GPU: the closed-loop renderer (gnbv_render_depth, csrc/render.hip) against an fp64 brute-force ray / triangle oracle
(tests/render_oracle.py) and against synthetic.render_depth."""
import math

import numpy as np
import pytest
import torch

from tests import render_oracle as RO
from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.mesh_scene import MeshScene, box_triangles, random_rotation, sphere_triangles

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-5  # |d depth| <= REL * |depth| where both hit the same class
SEG_FRAC = 1e-4  # seg may differ at silhouette pixels only, at most this share of the pixels


def _feed(mesh, h, w, with_rgba=True):
    from gennbv_amd.env.render_feed import RenderFeed
    return RenderFeed(mesh, TaskConfig(camera_width=w, camera_height=h), with_rgba=with_rgba)


def _lattice_poses(n, seed, cfg=None):
    cfg = cfg or TaskConfig()
    a = S.sample_actions(n, cfg, torch.Generator().manual_seed(seed))
    return S.poses_from_actions(a, cfg).float()


def _box_mesh(n, seed):
    sc = S.make_scenes(n, 16, seed=seed)
    return sc, MeshScene.from_boxes(sc, device=DEV)


def _rotated_mesh(n, seed):
    """Per env: 2-4 randomly rotated boxes and a UV sphere (arbitrarily oriented triangles)."""
    g = torch.Generator().manual_seed(seed)
    tris, ids = [], []
    for _ in range(n):
        t, i = [], []
        for k in range(int(torch.randint(2, 5, (1,), generator=g))):
            half = 0.5 + torch.rand(3, generator=g, dtype=torch.float64) * 2.0
            b = box_triangles(-half[None], half[None]).double() @ random_rotation(g).T
            centre = torch.cat([(torch.rand(2, generator=g, dtype=torch.float64) - 0.5) * 9.0,
                                2.0 + torch.rand(1, generator=g, dtype=torch.float64) * 4.0])
            t.append((b + centre).float())
            i.append(torch.full((12,), k + 1, dtype=torch.int32))
        c = [float(x) for x in (torch.rand(3, generator=g) - 0.5) * torch.tensor([8.0, 8.0, 2.0]) + torch.tensor([0.0, 0.0, 3.0])]
        s = sphere_triangles(c, 1.0 + float(torch.rand(1, generator=g)) * 1.5, 10, 20)
        t.append(s)
        i.append(torch.full((s.shape[0],), 7, dtype=torch.int32))
        tris.append(torch.cat(t))
        ids.append(torch.cat(i))
    return MeshScene.from_triangles(tris, ids, device=DEV)


def _oracle(mesh, c2w, kinv, h, w):
    tri = [mesh.env_triangles(e)[0] for e in range(mesh.num_envs)]
    ids = [mesh.env_triangles(e)[1] for e in range(mesh.num_envs)]
    return RO.render(tri, ids, c2w, kinv, h, w)


def _compare(depth, seg, t_ref, obj_ref, depth_cap=None):
    """seg: differences only at silhouettes and at most SEG_FRAC of the pixels; depth: REL where the classes agree (off the
    silhouettes; within `depth_cap` metres if given).  Returns the compared mask."""
    obj_k = seg > 0
    obj_r = obj_ref > 0
    sil = RO.silhouette(obj_ref)
    diff = obj_k != obj_r
    assert not (diff & ~sil).any(), f"{int((diff & ~sil).sum())} seg differences off the silhouettes"
    assert diff.float().mean().item() <= SEG_FRAC, f"seg differs at {diff.float().mean().item():.2e} of the pixels"
    tk = -depth.double()
    miss_k, miss_r = torch.isinf(tk), torch.isinf(t_ref)
    same = ~diff & ~sil
    assert torch.equal(miss_k[same], miss_r[same]), "hit / miss differs off the silhouettes"
    cmp = same & ~miss_r
    if depth_cap is not None:
        cmp &= t_ref <= depth_cap
    rel = ((tk - t_ref).abs() / t_ref)[cmp]
    assert cmp.sum() > 0.25 * cmp.numel() and rel.max().item() <= REL, f"max relative depth error {rel.max().item():.3e}"
    return cmp


@pytest.mark.parametrize("kind,n,h,w", [("boxes", 16, 240, 320), ("rotated", 6, 240, 320), ("boxes", 7, 37, 53), ("rotated", 7, 37, 53)])
def test_depth_seg_rgba_against_fp64_oracle(kind, n, h, w):
    mesh = _box_mesh(n, 11)[1] if kind == "boxes" else _rotated_mesh(n, 12)
    poses = _lattice_poses(n, 3).to(DEV)
    feed = _feed(mesh, h, w)
    depth, seg, rgba, c2w = feed.render(poses)
    t_ref, obj_ref = _oracle(mesh, c2w, feed.inv_intri_host, h, w)
    assert (obj_ref > 0).float().mean() > 0.1  # the cameras look at the scene
    _compare(depth, seg, t_ref, obj_ref)
    # rgba: render_depth's shading of the hit object wherever the object ids can be compared (off the silhouettes)
    agree = ((seg > 0) == (obj_ref > 0)) & ~RO.silhouette(obj_ref)
    assert torch.equal(rgba[agree], RO.shade(obj_ref)[agree])


def test_box_scenes_match_synthetic_render_depth():
    n, h, w = 16, 240, 320
    sc, mesh = _box_mesh(n, 21)
    poses = _lattice_poses(n, 5).to(DEV)
    feed = _feed(mesh, h, w)
    depth, seg, rgba, _ = feed.render(poses)
    sc_dev = S.Scene(*[t.to(DEV) for t in (sc.boxes_min, sc.boxes_max, sc.grid_gt, sc.range_gt, sc.voxel_size,
                                           sc.num_valid_voxel_gt, sc.env_origins)])
    d_ref, s_ref, c_ref, _ = S.render_depth(sc_dev, poses, h, w)
    # render_depth's object id per pixel, from its shading (ids <= 8 shade distinctly)
    which = torch.zeros(n, h, w, dtype=torch.int64, device=DEV)
    for k in range(1, sc.boxes_min.shape[1] + 1):
        which[(s_ref > 0) & (c_ref[..., 0] == (k * 29 % 200 + 40))] = k
    t_ref = torch.where(torch.isinf(d_ref), torch.full_like(d_ref, float("inf")), -d_ref).double()
    # render_depth builds its rays with a matrix product (a different rounding of the same directions): the depth tolerance is
    # checked within the sensed range (TaskConfig.depth_sense_dist = 50 m), where a 1-ulp direction difference stays below it
    # a camera inside a box sees the box's bottom face, which lies on the ground plane: face and ground tie there and rounding
    # decides the class in either renderer.  Those envs are left out.
    pos = poses[:, None, :3]
    inside = ((pos > sc_dev.boxes_min) & (pos < sc_dev.boxes_max)).all(-1).any(-1)
    keep = ~inside
    assert keep.sum() >= n // 2
    _compare(depth[keep], seg[keep], t_ref[keep], which[keep], depth_cap=50.0)
    agree = ((seg > 0) == (s_ref > 0)) & ~RO.silhouette(which) & keep[:, None, None]
    assert torch.equal(rgba[agree], c_ref[agree])


def test_c2w_within_one_ulp_of_camera_to_world():
    n = 64
    poses = _lattice_poses(n, 9)
    poses[:4, 4] = torch.tensor([math.pi / 2, -math.pi / 2, 0.0, 0.3]).float()  # straight down, straight up
    poses = poses.to(DEV)
    mesh = _box_mesh(n, 1)[1]
    _, _, _, c2w = _feed(mesh, 8, 8).render(poses)
    ref = S.camera_to_world(poses).float().cpu().numpy()
    got = c2w.cpu().numpy()
    ulp = np.spacing(np.abs(ref).astype(np.float32))
    assert (np.abs(got - ref) <= ulp).all(), np.abs(got - ref).max()


def test_watertight_along_shared_diagonals():
    """Square faces seen head-on with their diagonals on the image diagonals, and triangle fans around the optical axis:
    many rays pass along shared edges.  No background pixel may sit inside the object where the oracle sees the object."""
    h = w = 128
    tris, ids = [], []
    fan = []
    for k in range(16):  # a fan of 16 triangles around the axis x = y = 0, at z = 3
        a0, a1 = 2 * math.pi * k / 16, 2 * math.pi * (k + 1) / 16
        fan.append([[0.0, 0.0, 3.0], [4 * math.cos(a0), 4 * math.sin(a0), 3.0], [4 * math.cos(a1), 4 * math.sin(a1), 3.0]])
    fan = torch.tensor(fan)
    for e in range(6):
        if e % 2 == 0:
            s = 2.0 + e
            tris.append(box_triangles(torch.tensor([[-s, -s, 0.0]]), torch.tensor([[s, s, 2.0 + e * 0.5]])))
            ids.append(torch.ones(12, dtype=torch.int32))
        else:
            tris.append(fan)
            ids.append(torch.full((16,), 3, dtype=torch.int32))
    mesh = MeshScene.from_triangles(tris, ids, device=DEV)
    # straight down from above the centre, yaw 0 / 45 / 90 deg: the face diagonals lie on the image diagonals at yaw 0 and 90
    yaws = [0.0, 0.0, math.pi / 4, math.pi / 4, math.pi / 2, math.pi / 2]
    poses = torch.tensor([[0.0, 0.0, 10.0, 0.0, math.pi / 2, y] for y in yaws]).float().to(DEV)
    feed = _feed(mesh, h, w)
    depth, seg, _, c2w = feed.render(poses)
    t_ref, obj_ref = _oracle(mesh, c2w, feed.inv_intri_host, h, w)
    obj = (seg > 0).float()[:, None]
    # background pixel with all four neighbours object in the render, where the oracle sees the object
    nb = torch.nn.functional.conv2d(torch.nn.functional.pad(obj, (1, 1, 1, 1)), torch.tensor([[[[0.0, 1, 0], [1, 0, 1], [0, 1, 0]]]], device=DEV))
    holes = (obj == 0) & (nb == 4) & (obj_ref[:, None] > 0)
    assert int(holes.sum()) == 0, f"{int(holes.sum())} pixels fall through shared edges"
    _compare(depth, seg, t_ref, obj_ref)


def test_deterministic_empty_env_and_extreme_pitches():
    h, w = 96, 128
    sc, _ = _box_mesh(4, 4)
    tris = [MeshScene.from_boxes(sc).env_triangles(e)[0] for e in range(3)] + [torch.zeros(0, 3, 3)]
    ids = [MeshScene.from_boxes(sc).env_triangles(e)[1] for e in range(3)] + [torch.zeros(0, dtype=torch.int32)]
    mesh = MeshScene.from_triangles(tris, ids, device=DEV)
    cfg = TaskConfig()
    init = torch.tensor(cfg.init_pose_buf).float()
    poses = torch.stack([init, torch.tensor([0.0, 0.0, 12.0, 0.0, -math.pi / 2, 0.0]),  # init pose (pitch 90: down), sky-facing
                         torch.tensor([-7.0, 1.0, 3.0, 0.0, 0.2, 0.5]), torch.tensor([5.0, -3.0, 4.0, 0.0, 0.3, 2.0])]).float().to(DEV)
    feed = _feed(mesh, h, w)
    a = [x.clone() for x in feed.render(poses)]
    b = feed.render(poses)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    depth, seg, rgba, c2w = a
    # sky-facing: nothing but sky
    assert torch.isinf(depth[1]).all() and (depth[1] < 0).all() and (seg[1] == 0).all()
    # the empty env: ground and sky only, the ground where render_depth puts it
    assert (seg[3] == 0).all()
    o, d = RO.rays(c2w, feed.inv_intri_host, h, w)
    dz = d[3, ..., 2]
    tg = (-o[3, 2] / dz)
    want = torch.where((dz < -1e-6) & (tg > 1e-3), -tg, torch.full_like(tg, -float("inf")))
    assert torch.equal(depth[3], want)
    assert (rgba[3] == torch.tensor([90, 120, 70, 255], dtype=torch.uint8, device=DEV)).all()
    t_ref, obj_ref = _oracle(mesh, c2w, feed.inv_intri_host, h, w)
    _compare(depth, seg, t_ref, obj_ref)
    assert (seg[0] > 0).any()  # the init pose looks down onto the boxes

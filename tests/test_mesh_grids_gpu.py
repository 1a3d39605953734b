"""GPU: the five kernels that read a GnbvMeshScene -- render, view cover, collide, sweep, voxelize -- on cell grids the builder
never makes (tests/mesh_grid_util.py).  The lists of a grid are a conservative superset and nothing more (include/gennbv_hip.h),
so every output must be the same bits on every variant; against fp64 the existing tests' constants and comparisons are imported,
not restated.  No tolerance is added here.  Each test first re-asserts, on the inputs it uses, the regime counts of
tests/test_mesh_grids_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from gennbv_amd.env.config import TaskConfig
from tests import mesh_grid_util as U
from tests import render_oracle as RO
from tests import test_collision_gpu as TC
from tests import test_render_gpu as TR
from tests import test_view_cover_gpu as VC
from tests import voxelize_oracle as VO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMPTY = 2  # the env without triangles of mesh_grid_util.scene_triangles
GROUND_RGBA = [90, 120, 70, 255]


@pytest.fixture(scope="module")
def scene():
    """(tris, ids, {variant: MeshScene on the CPU}, {variant: the same on the GPU})"""
    tris, ids = U.scene_triangles()
    cpu = U.variants(tris, ids)
    return tris, ids, cpu, {k: U.to_device(m, DEV) for k, m in cpu.items()}


def _render(mesh, poses, h, w, fov=None):
    from gennbv_amd.env.render_feed import RenderFeed
    cfg = TaskConfig(camera_width=w, camera_height=h) if fov is None else TaskConfig(camera_width=w, camera_height=h, horizontal_fov=fov)
    feed = RenderFeed(mesh, cfg)
    return [x.clone() for x in feed.render(poses)], feed.inv_intri_host


def _same_image(got, ref, off_sil, tag):
    for x, y, what in zip((got[0], got[1], got[3]), (ref[0], ref[1], ref[3]), ("depth_raw", "seg_raw", "c2w")):
        assert torch.equal(x, y), f"{tag}: {what} differs at {int((x != y).sum())} elements"
    # the closest t is computed per triangle, so a grid may only change which of two exactly tying triangles wins
    assert torch.equal(got[2][off_sil], ref[2][off_sil]), f"{tag}: rgba differs off the silhouettes"


# ---------------------------------------------------------------------------------------------------------------
# render
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", U.CAMERAS)
def test_render_is_the_same_image_on_every_grid(scene, h, w):
    _, _, cpu, dev = scene
    poses = U.render_poses(seed=h)
    U.check_render_inputs(cpu, poses)
    poses = poses.to(DEV)
    ref, kinv = _render(dev["default"], poses, h, w)
    t_ref, obj_ref = TR._oracle(dev["default"], ref[3], kinv, h, w)
    off_sil = ~RO.silhouette(obj_ref)
    assert (obj_ref > 0).float().mean() > 0.1
    for name in U.VARIANTS:
        got, _ = _render(dev[name], poses, h, w)
        _same_image(got, ref, off_sil, name)
        TR._compare(got[0], got[1], t_ref, obj_ref)
        agree = ((got[1] > 0) == (obj_ref > 0)) & off_sil
        assert torch.equal(got[2][agree], RO.shade(obj_ref)[agree]), name
        # the env without triangles: ground and sky only, the ground where synthetic.render_depth puts it
        assert (got[1][EMPTY] == 0).all() and (got[2][EMPTY] == torch.tensor(GROUND_RGBA, dtype=torch.uint8, device=DEV)).all(), name
        o, d = RO.rays(got[3], kinv, h, w)
        dz = d[EMPTY, ..., 2]
        tg = -o[EMPTY, 2] / dz
        assert torch.equal(got[0][EMPTY], torch.where((dz < -1e-6) & (tg > 1e-3), -tg, torch.full_like(tg, -float("inf")))), name


def test_render_walks_hundreds_of_thin_cells_to_the_same_image():
    """The long thin scene at res >= 256 along the tube against the same triangles in one cell: rays cross more than 200 cells
    before they hit the far end (counted in fp64 in tests/test_mesh_grids_cpu.py and again here)."""
    h, w = U.CAMERAS[1]
    cpu = U.thin_variants()
    r = cpu["fine"].cell_res[0].tolist()
    assert r[0] >= 256 and max(r[1:]) <= 8 and int(cpu["one"].cell_res.max()) == 1
    poses = U.thin_poses().to(DEV)
    fine, kinv = _render(U.to_device(cpu["fine"], DEV), poses, h, w, U.THIN_FOV)
    one, _ = _render(U.to_device(cpu["one"], DEV), poses, h, w, U.THIN_FOV)
    t_ref, obj_ref = TR._oracle(U.to_device(cpu["fine"], DEV), fine[3], kinv, h, w)
    o, d = RO.rays(fine[3], kinv, h, w)
    steps = np.stack([U.dda_steps(cpu["fine"], e, o[e].cpu().numpy(), d[e].reshape(-1, 3).cpu().numpy(), t_ref[e].reshape(-1).cpu().numpy())
                      for e in range(3)])
    far = (steps > 200) & (obj_ref.reshape(3, -1).cpu().numpy() > 0)
    print("longest walk per camera", steps.max(1), "rays above 200 steps", (steps > 200).sum(1), "ending on an object", far.sum(1))
    assert (steps > 200).sum() > 100 and far.sum() > 20
    _same_image(fine, one, ~RO.silhouette(obj_ref), "fine vs one")
    for got in (fine, one):
        TR._compare(got[0], got[1], t_ref, obj_ref)


def test_render_raw_abi_with_padded_pose_rows_and_no_rgba(scene):
    """gnbv_render_depth itself: poses_row_stride = 11 with NaN in the padding columns, rgba = NULL, n = 1, on a shuffled grid --
    bit-equal to the wrapper's result."""
    from gennbv_amd import _lib
    tris, ids, _, _ = scene
    mesh = U.variants([tris[0]], [ids[0]], device=DEV, names=("shuffled",))["shuffled"]
    h, w = U.CAMERAS[0]
    pose = U.lattice_poses(1, 1, 4)[:, 0].to(DEV)
    ref, kinv = _render(mesh, pose, h, w)
    rows = torch.full((1, 11), float("nan"), device=DEV)
    rows[:, :6] = pose
    depth = torch.full((1, h, w), float("nan"), device=DEV)
    seg, c2w = torch.full_like(depth, float("nan")), torch.full((1, 4, 4), float("nan"), device=DEV)
    sc = mesh.c_struct()
    assert sc.n == 1
    rc = _lib.load().gnbv_render_depth(C.byref(sc), rows.data_ptr(), 11, kinv.data_ptr(), h, w, c2w.data_ptr(), depth.data_ptr(),
                                       seg.data_ptr(), None, _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(depth, ref[0]) and torch.equal(seg, ref[1]) and torch.equal(c2w, ref[3])
    assert (ref[1] > 0).any() and not (ref[1] > 0).all()


# ---------------------------------------------------------------------------------------------------------------
# view cover
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
def test_view_cover_and_masks_are_the_same_on_every_grid(scene, stride):
    from gennbv_amd import _lib
    from gennbv_amd.ops.view_cover import ViewCover
    _, _, cpu, dev = scene
    g, h, w, k = 20, 60, 80, 8
    cfg = VC._cfg(h, w, g)
    n = cpu["default"].num_envs
    rng, vox = cpu["default"].grid_spec(g, torch.tensor([U.VOXEL_RANGE] * n))
    poses = VC._look_at_poses(cfg, n, k, seed=7 + stride)[1].to(DEV)
    rs = np.random.RandomState(stride)
    lib, st = _lib.load(), _lib.stream_ptr(torch.device(DEV))
    ref = None
    for name in U.VARIANTS:
        mesh = dev[name]
        vc = ViewCover(mesh, cfg, rng, vox, k, stride=stride)
        if ref is None:
            gt, scanned = VC._bool_to_bits(rs.rand(n, g ** 3) < 0.6, vc.words), VC._bool_to_bits(rs.rand(n, g ** 3) < 0.3, vc.words)
            ones = torch.full_like(gt, -1)
        cover = vc(poses, gt, scanned).clone()
        seen = vc.accumulate(poses, gt, torch.zeros_like(gt)).clone()
        a = _lib.GnbvViewCover()
        C.memmove(C.byref(a), C.byref(vc._args), C.sizeof(a))
        masks = torch.full((n, k, vc.words), -12345, dtype=torch.int32, device=DEV)
        a.poses, a.gt_bits, a.scanned_bits, a.cover, a.seen_bits = poses.data_ptr(), ones.data_ptr(), None, None, None
        sc = mesh.c_struct()
        assert lib.gnbv_view_cover_masks(C.byref(sc), C.byref(a), masks.data_ptr(), st) == 0
        if ref is None:
            ref = (cover, seen, masks)
            assert int(cover[..., 0].sum()) > 0 and bool((cover[..., 0] < cover[..., 1]).any())
        for x, y, what in zip((cover, seen, masks), ref, ("cover", "seen_bits", "mask_bits")):
            assert torch.equal(x, y), f"{name}: {what} differs"
        assert int(cover[EMPTY].sum()) == 0 and int(masks[EMPTY].abs().sum()) == 0, name  # the env without triangles
        if stride == 1:  # the masks (all-ones ground truth) are the hit masks of the update on this variant's own image
            for j in range(k):
                _, hit, _ = VC._hit_mask_of_update(mesh, cfg, rng, vox, poses[:, j].contiguous())
                assert np.array_equal(VC._bits_to_bool(masks[:, j].contiguous(), g), hit), (name, j)
                assert j > 0 or hit.sum() > 0


# ---------------------------------------------------------------------------------------------------------------
# collide
# ---------------------------------------------------------------------------------------------------------------
def _body(r, h, ground=False, sweep=False):
    from gennbv_amd.env.collision import CollisionBody
    return CollisionBody(r, h, ground, sweep)


@pytest.fixture(scope="module")
def collision_oracle(scene):
    from tests.collision_oracle import CollisionOracle
    tris, ids, _, _ = scene
    return CollisionOracle([t.numpy() for t in tris], [i.numpy() for i in ids])


@pytest.mark.parametrize("ground", [False, True])
@pytest.mark.parametrize("body", [U.DRONE, U.LARGE])
def test_collide_gives_the_same_codes_on_every_grid(scene, collision_oracle, body, ground):
    tris, _, cpu, dev = scene
    poses = U.collide_poses(tris)
    n, k = poses.shape[:2]
    if body == U.LARGE:
        print(U.check_walk_regimes(cpu, poses))
    p_dev = torch.from_numpy(poses).to(DEV)
    ref = dev["default"].collide_candidates(p_dev, _body(*body, ground)).clone()
    for name in U.VARIANTS:
        got = dev[name].collide_candidates(p_dev, _body(*body, ground))
        assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} codes differ from default's"
    codes = ref.cpu().numpy()
    want = TC._compare(collision_oracle, dev["default"], np.repeat(np.arange(n), k), poses.reshape(n * k, 6), codes.reshape(-1), body[0], body[1],
                       ground)
    assert (want == 0).sum() > 20 and (want & TC.SURFACE).sum() > 20
    assert (codes[EMPTY] & ~np.uint8(TC.GROUND) == 0).all() and ((codes[EMPTY] != 0).any() == ground)  # no triangles: 0 or the ground bit


def test_collide_finds_the_one_triangle_at_the_end_of_the_walk():
    """Hand cases of wave_any_listed_tri: on `one` the only triangle the body touches is stored last, behind more than 2 048
    entries; on `fine` it is listed only in the top layer of the large body's range (more than 64 cells per layer), in the last
    64-cell batch.  Moved 1 mm clear, the same placements give 0."""
    wt, wi, centre = U.walk_scene_triangles()
    names = [v for v in U.VARIANTS if v != "overlisted"]  # (one env only: "every triangle in every cell" would be 10 M entries)
    cpu = U.variants(wt, wi, names=names)
    U.check_walk_hand_cases(cpu["one"], cpu["fine"], centre)
    for name in names:
        mesh = U.to_device(cpu[name], DEV)
        for r, h in (U.DRONE, U.LARGE):
            for clear in (False, True):
                p = torch.from_numpy(U.walk_hand_poses(centre, h, clear)).to(DEV)
                code = int(mesh.collide(p, _body(r, h))[0])
                assert code == (0 if clear else TC.SURFACE), (name, r, h, clear, code)


def test_collide_finds_the_one_triangle_in_every_batch_of_the_walk():
    """The large body's side against the small triangle, all around it and at every height: the only triangle it touches is listed
    in the first, the second, ... 64-cell batch of the body's range (counted on the host).  A walk that skips or cuts short any
    batch reports such a body free."""
    wt, wi, centre = U.walk_scene_triangles()
    names = [v for v in U.VARIANTS if v != "overlisted"]
    cpu = U.variants(wt, wi, names=names)
    touch, clear = U.walk_side_poses(centre, False), U.walk_side_poses(centre, True)
    print("batches that hold the touched triangle:", U.check_walk_batches(cpu["fine"], touch))
    p = torch.from_numpy(np.stack([touch, clear])).to(DEV).permute(1, 0, 2).contiguous()[None]  # [1, 144 * 2, 6]: touch, clear, ...
    p = p.reshape(1, -1, 6)
    want = torch.tensor([TC.SURFACE, 0], dtype=torch.uint8, device=DEV).repeat(touch.shape[0])[None]
    for name in names:
        got = U.to_device(cpu[name], DEV).collide_candidates(p, _body(*U.LARGE))
        assert torch.equal(got, want), (name, torch.nonzero(got != want)[:5].tolist())


# ---------------------------------------------------------------------------------------------------------------
# sweep
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ground", [False, True])
@pytest.mark.parametrize("radius", [None, 1.0])  # the drone's path radius; a sphere whose pieces span hundreds of `fine` cells
def test_sweep_gives_the_codes_of_the_exhaustive_list_on_every_grid(scene, radius, ground):
    """The flights of tests/test_sweep_gpu.py's one-vs-fine test, on every variant.  At radius 1 a piece's range holds more than 64
    cells, most of them cells of the previous piece's range (the seen / prev exclusion of wave_any_listed_tri)."""
    from gennbv_amd.env.collision import CollisionBody
    from tests.sweep_oracle import PATH, PATH_GROUND
    tris, _, cpu, dev = scene
    a, b = U.sweep_flights(tris)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    body = _body(*U.DRONE, ground, True) if radius is None else CollisionBody(*U.DRONE, ground, True, sweep_radius=radius)
    if radius is not None:  # the sphere alone spans more than 64 cells of fine in two of the envs
        spans = [int((2 * radius / cpu["fine"].cell_size[e]).floor().prod()) for e in range(cpu["fine"].num_envs) if e != EMPTY]
        assert sorted(spans)[-2] > U.K_WAVE, spans
    ref = dev["one"].sweep_candidates(ta, tb, body).clone()
    assert bool((ref & PATH).any()) and not bool((ref & PATH).all())
    for name in U.VARIANTS:
        got = dev[name].sweep_candidates(ta, tb, body)
        assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} codes differ from one's"
    assert not bool((ref[EMPTY] & PATH).any()) and bool((ref[EMPTY] & PATH_GROUND).any()) == ground  # no triangles


# ---------------------------------------------------------------------------------------------------------------
# voxelize
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [20, 33])
def test_voxelize_gives_the_same_grid_on_every_grid(scene, g):
    _, _, cpu, dev = scene
    n = cpu["default"].num_envs
    rng, vox = cpu["default"].grid_spec(g, torch.tensor([U.VOXEL_RANGE] * n))
    if g == 20:  # the flush ran on `one`: a brick with more than kCap - kBlock candidates, from a list longer than kCap
        print("most candidates of one brick:", U.check_brick_regime(cpu["one"], rng.numpy(), vox.numpy(), g))
        assert int(np.diff(cpu["one"].cell_start.numpy()).max()) > U.K_CAP
    ref = None
    for name in U.VARIANTS:
        grid = torch.full((n, g, g, g), float("nan"), device=DEV)
        dev[name].voxelize_into(grid, rng.to(DEV), vox.to(DEV))
        if ref is None:
            ref = grid
            assert not torch.isnan(ref).any() and torch.all((ref == 0) | (ref == 1))
        assert torch.equal(grid, ref), f"{name}: {int((grid != ref).sum())} voxels differ from default's"
    assert int(ref[EMPTY].sum()) == 0 and all(int(ref[e].sum()) > 0 for e in range(n) if e != EMPTY)
    if g == 20:
        got = ref.cpu()
        for e in range(n):
            t = VO.tau(rng[e].numpy())
            sep = VO.separation(cpu["default"].env_triangles(e)[0], rng[e].numpy(), vox[e].numpy(), g, reach=2 * t)
            fn, fp_far, _ = VO.check(got[e], sep, t)
            assert fn == 0 and fp_far == 0, (e, fn, fp_far)

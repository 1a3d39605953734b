"""CPU: the cell-grid variants of tests/mesh_grid_util.py are valid, conservative grids; the inputs of tests/test_mesh_grids_gpu.py
reach the regimes that file claims (counted with the kernels' own formulas); and the fp64 oracles alone stay inside the existing
tests' caps on those inputs."""
import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.mesh_scene import EPS_ABS, EPS_REL, MeshScene
from tests import mesh_grid_util as U
from tests import render_oracle as RO
from tests import voxelize_oracle as VO


@pytest.fixture(scope="module")
def scene():
    tris, ids = U.scene_triangles()
    return tris, ids, U.variants(tris, ids)


def _exact_pairs(m, e):
    """(cell, tri) pairs of env e whose closed cell box meets the closed triangle (13-axis separating-axis test, fp64): the set
    mesh_grid_util.brute_force_cells computes, found among the cells each triangle's AABB meets."""
    t = m.env_triangles(e)[0].double()
    first = int(m.tri_count[:e].sum())
    r = m.cell_res[e].numpy().astype(np.int64)
    lo32, sz32 = m.cell_lo[e], m.cell_size[e]
    face = [(lo32[a] + torch.arange(int(r[a]) + 1, dtype=torch.float32) * sz32[a]) for a in range(3)]  # cell_box's lower faces, fp32
    upper = [(face[a][:-1] + sz32[a]).double().numpy() for a in range(3)]
    lower = [face[a][:-1].double().numpy() for a in range(3)]
    tmin, tmax = t.amin(1).numpy(), t.amax(1).numpy()
    i0 = np.stack([np.searchsorted(upper[a], tmin[:, a], "left") for a in range(3)], -1)  # first cell with upper >= tmin
    i1 = np.stack([np.searchsorted(lower[a], tmax[:, a], "right") - 1 for a in range(3)], -1)  # last cell with lower <= tmax
    i0, i1 = np.clip(i0, 0, r - 1), np.clip(i1, 0, r - 1)
    cell, tri = U._entries_of_ranges(i0, np.maximum(i1, i0), r, 0)
    ijk = np.stack([cell % r[0], (cell // r[0]) % r[1], cell // (r[0] * r[1])], -1)
    blo = torch.from_numpy(np.stack([lower[a][ijk[:, a]] for a in range(3)], -1))
    bhi = torch.from_numpy(np.stack([upper[a][ijk[:, a]] for a in range(3)], -1))
    gap = VO._sat_gap(t[tri], 0.5 * (blo + bhi), 0.5 * (bhi - blo))
    keep = (gap <= 0).numpy()
    return set(zip(cell[keep].tolist(), (tri[keep] + first).tolist()))


def test_the_fast_exact_overlap_is_the_brute_force_one(scene):
    m = scene[2]["default"]
    for e in (0, 3):
        assert _exact_pairs(m, e) == U.brute_force_cells(m, e)


@pytest.mark.parametrize("name", U.VARIANTS)
def test_every_variant_lists_a_superset_of_the_exact_overlap(scene, name):
    m = scene[2][name]
    for e in range(m.num_envs):
        exact, listed = _exact_pairs(m, e), U.listed(m, e)
        assert exact <= listed, f"{name} env {e}: {len(exact - listed)} overlapping (cell, triangle) pairs not listed"
        assert bool(exact) == (int(m.tri_count[e]) > 0)
        if int(m.tri_count[e]):  # the grid's box holds every vertex
            v = m.env_triangles(e)[0].reshape(-1, 3)
            lo, hi = m.cell_lo[e], m.cell_lo[e] + m.cell_size[e] * m.cell_res[e].float()
            assert (v > lo).all() and (v < hi).all()


@pytest.mark.parametrize("name", U.VARIANTS)
def test_every_variant_is_a_consistent_grid(scene, name):
    tris, _, vs = scene
    m, d = vs[name], vs["default"]
    assert torch.equal(m.tris, d.tris) and torch.equal(m.tri_obj, d.tri_obj) and torch.equal(m.tri_count, d.tri_count)
    for a in (m.cell_lo, m.cell_size, m.cell_res, m.cell_base, m.cell_start, m.cell_tris):
        assert a.is_contiguous()
    assert m.cell_lo.dtype == m.cell_size.dtype == torch.float32
    assert m.cell_res.dtype == m.cell_base.dtype == m.cell_start.dtype == m.cell_tris.dtype == torch.int32
    start = m.cell_start.numpy().astype(np.int64)
    cells = start.size - 1
    assert start[0] == 0 and (np.diff(start) >= 0).all() and start[-1] == m.cell_tris.numel()
    ncell = m.cell_res.numpy().astype(np.int64).prod(-1)
    base = m.cell_base.numpy().astype(np.int64)
    used = np.zeros(cells, np.int64)
    first = 0
    for e in range(m.num_envs):
        cnt = int(m.tri_count[e])
        assert (ncell[e] > 0) == (cnt > 0) and 0 <= base[e] and base[e] + ncell[e] <= cells
        assert bool((m.cell_size[e] > 0).all())
        used[base[e]:base[e] + ncell[e]] += 1
        t = m.cell_tris[int(start[base[e]]):int(start[base[e] + ncell[e]])].numpy()
        assert t.size == 0 or (t.min() >= first and t.max() < first + cnt), "an env lists another env's triangle"
        assert np.unique(t).size == cnt  # every triangle is listed somewhere
        first += cnt
    assert used.max() == 1  # the env blocks do not overlap
    assert (np.diff(start)[used == 0] == 0).all()  # unused cells are empty


def test_the_variants_are_what_their_names_say(scene):
    _, _, vs = scene
    d = vs["default"]
    assert int(vs["one"].cell_res.max()) == 1 and int(vs["fine"].cell_res.max()) >= 48
    # loose: unequal resolutions, cell edges more than a factor 4 apart, res == 1 on two axes in one env, the builder's padding
    lo = vs["loose"]
    with_tris = [e for e in range(lo.num_envs) if int(lo.tri_count[e])]
    assert any((lo.cell_res[e] == 1).sum() == 2 for e in with_tris)
    for e in with_tris:
        sz = lo.cell_size[e]
        assert float(sz.max() / sz.min()) > 4.0
        assert len(set(lo.cell_res[e].tolist())) >= 2
    # overlisted: a superset of default with the same geometry; every cell of one env lists every triangle
    ov = vs["overlisted"]
    assert torch.equal(ov.cell_res, d.cell_res) and torch.equal(ov.cell_lo, d.cell_lo)
    full = 0
    for e in with_tris:
        a, b = U.listed(d, e), U.listed(ov, e)
        assert a < b
        full += len(b) == int(d.cell_res[e].prod()) * int(d.tri_count[e])
    assert full == 1
    # shuffled: the same sets per cell, not ascending, about a tenth listed twice
    sh = vs["shuffled"]
    for e in with_tris:
        assert U.listed(sh, e) == U.listed(d, e)
        cell, tri = U.env_entries(sh, e)
        same_cell = cell[1:] == cell[:-1]
        assert (np.diff(tri)[same_cell] < 0).mean() > 0.2
        extra = tri.size / U.env_entries(d, e)[1].size - 1.0
        assert 0.05 < extra < 0.15, extra
    # scattered: default's lists, blocks in reverse order with unused cells between, the empty env between two others
    sc = vs["scattered"]
    base = sc.cell_base[with_tris].tolist()
    assert base == sorted(base, reverse=True) and len(set(base)) == len(base)
    assert sc.cell_start.numel() > d.cell_start.numel() + U.GAP
    assert any(int(sc.tri_count[e]) == 0 and 0 < e < sc.num_envs - 1 for e in range(sc.num_envs))
    for e in with_tris:
        assert U.env_entries(sc, e)[1].tolist() == U.env_entries(d, e)[1].tolist()


def test_the_walk_regimes_are_reached(scene):
    tris, _, vs = scene
    print(U.check_walk_regimes(vs, U.collide_poses(tris)))
    wt, wi, centre = U.walk_scene_triangles()
    wv = U.variants(wt, wi, names=("one", "fine"))
    U.check_walk_hand_cases(wv["one"], wv["fine"], centre)
    print("batches that hold the touched triangle:", U.check_walk_batches(wv["fine"], U.walk_side_poses(centre, False)))


def test_the_voxelizer_regimes_are_reached(scene):
    _, _, vs = scene
    one = vs["one"]
    rng, vox = one.grid_spec(20, torch.tensor([U.VOXEL_RANGE] * one.num_envs))
    print("most candidates of one brick at g = 20:", U.check_brick_regime(one, rng.numpy(), vox.numpy(), 20))
    longest = int(np.diff(one.cell_start.numpy()).max())
    assert longest > U.K_CAP > U.K_BLOCK  # one cell's list needs several chunks of the k0 loop


def _cpu_render_oracle(m, poses, h, w, fov=None):
    kinv = S.inverse_intrinsics(h, w) if fov is None else S.inverse_intrinsics(h, w, fov)
    c2w = S.camera_to_world(poses).float()  # within 1 ulp of the kernel's (tests/test_render_gpu.py)
    tri = [m.env_triangles(e)[0] for e in range(m.num_envs)]
    ids = [m.env_triangles(e)[1] for e in range(m.num_envs)]
    return c2w, kinv, RO.render(tri, ids, c2w, kinv, h, w)


def test_the_render_inputs_are_inside_the_loose_box_and_the_oracle_keeps_enough_pixels(scene):
    _, _, vs = scene
    for h, w in U.CAMERAS:
        poses = U.render_poses(seed=h)
        U.check_render_inputs(vs, poses)
        _, _, (t_ref, obj_ref) = _cpu_render_oracle(vs["default"], poses, h, w)
        cmp = ~RO.silhouette(obj_ref) & ~torch.isinf(t_ref)
        share = cmp.float().mean().item()
        print(h, w, "compared share", share, "object share", (obj_ref > 0).float().mean().item())
        assert share > 0.4  # tests/test_render_gpu.py::_compare needs more than 0.25
        assert (obj_ref > 0).float().mean() > 0.1
        assert bool((obj_ref[2] == 0).all())  # the env without triangles
        if h % 2 == 0:  # the level camera: where the principal point lies on a pixel row, a row of rays with dz == 0 exactly
            assert bool((RO.rays(S.camera_to_world(poses).float(), S.inverse_intrinsics(h, w), h, w)[1][3, ..., 2] == 0).any())


def test_the_thin_scene_walks_hundreds_of_cells():
    tv = U.thin_variants()
    fine = tv["fine"]
    r = fine.cell_res[0].tolist()
    assert r[0] >= 256 and r[1] <= 8 and r[2] <= 8, r
    assert int(tv["one"].cell_res.max()) == 1
    h, w = U.CAMERAS[1]
    poses = U.thin_poses()
    c2w, kinv, (t_ref, obj_ref) = _cpu_render_oracle(fine, poses, h, w, U.THIN_FOV)
    o, d = RO.rays(c2w, kinv, h, w)
    steps = np.stack([U.dda_steps(fine, e, o[e].numpy(), d[e].reshape(-1, 3).numpy(), t_ref[e].reshape(-1).numpy()) for e in range(3)])
    hit_far = (steps > 200) & (obj_ref.reshape(3, -1).numpy() > 0)
    print("longest walk", steps.max(1), "rays above 200 steps", (steps > 200).sum(1), "of them ending on an object", hit_far.sum(1))
    assert steps.max() > 200 and (steps > 200).sum() > 100 and hit_far.sum() > 20
    cmp = ~RO.silhouette(obj_ref) & ~torch.isinf(t_ref)
    assert cmp.float().mean().item() > 0.4


def test_the_fp32_walk_drifts_less_than_the_builders_padding():
    """csrc/raytrace.h adds tdx to tmx once per cell crossed, in fp32; a triangle is listed with a padding of EPS_REL of the env's
    largest extent + EPS_ABS.  The walk is sound while the boundary crossings it computes stay within that padding of the true ones.
    Here the x crossings of the thin scene's rays are accumulated as the kernel does, at the builder's upper limit of 1 024 cells on
    the axis, and compared with the fp64 crossings of the same fp32 grid: the drift, as a distance along the axis, is printed and must
    stay below the padding (the condition of soundness, not a measured figure)."""
    f32 = np.float32
    t, i = U.thin_scene_triangles()
    m = MeshScene.from_triangles(t, i, cells_per_triangle=800.0, max_cells_per_axis=1024)
    rx = int(m.cell_res[0, 0])
    assert rx == 1024
    lx, sx = f32(m.cell_lo[0, 0]), f32(m.cell_size[0, 0])
    ext = (m.cell_size[0] * m.cell_res[0].float()).max().item()
    eps = (ext - 4 * EPS_ABS) / (1 + 4 * EPS_REL) * EPS_REL + EPS_ABS  # MeshScene._bin: the box is the bounds grown by 2 eps a side
    h, w = U.CAMERAS[1]
    poses = U.thin_poses()
    o, d = RO.rays(S.camera_to_world(poses).float(), S.inverse_intrinsics(h, w, U.THIN_FOV), h, w)
    worst = 0.0
    for e in range(poses.shape[0]):
        ox, dx = f32(o[e, 0]), d[e].reshape(-1, 3)[:, 0].numpy().astype(f32)
        assert (dx > 0).all()
        ix = (f32(1.0) / dx).astype(f32)
        t_in = np.maximum(((lx - ox) * ix).astype(f32), f32(1e-3))  # the x slab's entry (the later of the slabs enters no earlier)
        px = (ox + (dx * t_in).astype(f32)).astype(f32)
        c0 = np.clip(np.floor(((px - lx).astype(f32) / sx).astype(f32)).astype(np.int64), 0, rx - 1)
        tm0 = (((lx + ((c0 + 1).astype(f32) * sx).astype(f32)).astype(f32) - ox).astype(f32) * ix).astype(f32)
        td = (sx / np.abs(dx)).astype(f32)
        steps = np.concatenate([tm0[:, None], np.broadcast_to(td[:, None], (dx.size, rx - 1))], 1)
        tm = np.cumsum(steps, axis=1, dtype=f32)  # sequential fp32 additions, as the kernel's tmx += tdx
        k = np.arange(rx)[None, :]
        exact = (float(lx) + (c0[:, None] + 1 + k) * float(sx) - float(ox)) / dx.astype(np.float64)[:, None]
        inside = c0[:, None] + 1 + k <= rx
        worst = max(worst, float((np.abs(tm.astype(np.float64) - exact) * dx.astype(np.float64)[:, None])[inside].max()))
    print(f"largest drift of an x crossing over up to {rx} steps: {worst:.3e} m; padding {eps:.3e} m; margin x{eps / worst:.1f}")
    assert worst < eps


def test_the_collision_oracle_is_robust_on_the_chosen_poses(scene):
    from tests.collision_oracle import CollisionOracle
    tris, ids, _ = scene
    oracle = CollisionOracle([t.numpy() for t in tris], [i.numpy() for i in ids])
    poses = U.collide_poses(tris)
    n, k = poses.shape[:2]
    env = np.repeat(np.arange(n), k)
    for r, h in (U.DRONE, U.LARGE):
        for ground in (False, True):
            want, robust = oracle.robust_codes(env, poses.reshape(n * k, 6), r, h, ground)
            print(r, h, ground, "robust", robust.mean(), "codes", np.bincount(want, minlength=8).tolist())
            assert robust.mean() >= 0.97  # tests/test_collision_gpu.py::_compare's min_robust
            assert (want == 0).sum() > 20 and (want & 1).sum() > 20  # free and touching poses both occur


def test_the_collision_oracle_decides_the_walk_placements():
    from tests.collision_oracle import SURFACE, CollisionOracle
    wt, wi, centre = U.walk_scene_triangles()
    oracle = CollisionOracle([t.numpy() for t in wt], [i.numpy() for i in wi])
    for clear in (False, True):
        p = np.concatenate([U.walk_side_poses(centre, clear), U.walk_hand_poses(centre, U.LARGE[1], clear)])
        want, robust = oracle.robust_codes(np.zeros(len(p), np.int64), p, *U.LARGE)
        assert robust.all() and (want == (0 if clear else SURFACE)).all()
        p = U.walk_hand_poses(centre, U.DRONE[1], clear)
        want, robust = oracle.robust_codes(np.zeros(1, np.int64), p, *U.DRONE)
        assert robust.all() and (want == (0 if clear else SURFACE)).all()


def test_the_builder_keeps_its_lists_ascending_and_free_of_duplicates(scene):
    """What `shuffled` departs from: the kernels do not need it (include/gennbv_hip.h), the builder still provides it."""
    _, _, vs = scene
    for name in ("default", "one", "fine"):
        for e in range(vs[name].num_envs):
            cell, tri = U.env_entries(vs[name], e)
            assert (np.diff(tri)[cell[1:] == cell[:-1]] > 0).all()
    assert EPS_REL == 1e-4 and EPS_ABS == 1e-5  # the padding rule the header names

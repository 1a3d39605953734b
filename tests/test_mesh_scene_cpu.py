"""CPU: MeshScene (gennbv_amd/env/mesh_scene.py) -- box triangulation and the conservative cell lists of the renderer."""
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.mesh_scene import MeshScene, box_triangles, random_rotation, sphere_triangles
from tests.mesh_grid_util import brute_force_cells as _brute_force_cells, listed as _listed  # (shared with test_mesh_grids_cpu.py)


def _areas_normals(t):
    c = torch.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], dim=-1).double()
    return 0.5 * c.norm(dim=-1), c


def test_from_boxes_area_normals_and_ids():
    sc = S.make_scenes(6, 16, seed=5)
    # one env without any box, one more unused box slot
    sc.boxes_min[2], sc.boxes_max[2] = 1e6, -1e6
    sc.boxes_min[3, 1], sc.boxes_max[3, 1] = 1e6, -1e6
    m = MeshScene.from_boxes(sc)
    assert m.num_envs == 6 and int(m.tri_count[2]) == 0 and m.cell_res[2].tolist() == [0, 0, 0]
    for e in range(6):
        t, ids = m.env_triangles(e)
        valid = (sc.boxes_min[e] <= sc.boxes_max[e]).all(-1)
        assert t.shape[0] == 12 * int(valid.sum())
        ext = (sc.boxes_max[e] - sc.boxes_min[e]).double()[valid]
        want = 2 * (ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 0] * ext[:, 2]).sum()
        area, nrm = _areas_normals(t)
        assert torch.allclose(area.sum(), want, rtol=1e-6)
        # outward: the normal points away from the centre of the triangle's box
        k = ids.long() - 1
        centre = 0.5 * (sc.boxes_min[e, k] + sc.boxes_max[e, k]).double()
        assert ((nrm * (t.double().mean(1) - centre)).sum(-1) > 0).all()
        assert sorted(set(ids.tolist())) == [int(i) + 1 for i in torch.nonzero(valid).flatten()]


def test_cell_lists_are_a_superset_of_the_exact_overlap():
    g = torch.Generator().manual_seed(3)
    rot = random_rotation(g)
    box = box_triangles(torch.tensor([[-2.0, -1.0, -0.5]]), torch.tensor([[2.0, 1.5, 3.0]])).double()
    box = (box @ rot.T + torch.tensor([1.0, -2.0, 4.0], dtype=torch.float64)).float()
    sph = sphere_triangles((2.0, 2.0, 2.0), 1.5, 8, 12)
    soup = (torch.rand(40, 3, 3, generator=g) - 0.5) * 8.0
    scenes = [torch.cat([box, sph]), soup, torch.zeros(0, 3, 3)]
    ids = [torch.ones(s.shape[0], dtype=torch.int32) for s in scenes]
    m = MeshScene.from_triangles(scenes, ids)
    for e in range(2):
        r = m.cell_res[e].tolist()
        assert min(r) >= 2 and max(r) <= 64
        exact, listed = _brute_force_cells(m, e), _listed(m, e)
        assert exact and exact <= listed, f"env {e}: {len(exact - listed)} overlapping (cell, triangle) pairs not listed"
        # conservative, not everything: the padding adds a thin shell only
        assert len(listed) < 3 * len(exact)
        # each env's cells cover every one of its vertices
        t, _ = m.env_triangles(e)
        lo, hi = m.cell_lo[e], m.cell_lo[e] + m.cell_size[e] * m.cell_res[e].float()
        assert (t.reshape(-1, 3) > lo).all() and (t.reshape(-1, 3) < hi).all()
    assert m.cell_res[2].tolist() == [0, 0, 0] and int(m.cell_start[-1]) == m.cell_tris.numel()


def test_resolution_rule_is_capped():
    big = sphere_triangles((0.0, 0.0, 5.0), 4.0, 40, 80)  # 6240 triangles
    m = MeshScene.from_triangles([big], [torch.ones(big.shape[0], dtype=torch.int32)])
    r = m.cell_res[0].tolist()
    assert r[0] == r[1] == r[2] and abs(r[0] ** 3 / (2 * big.shape[0]) - 1) < 0.2  # ~2 cells per triangle, cubic cells
    m = MeshScene.from_triangles([big], [torch.ones(big.shape[0], dtype=torch.int32)], cells_per_triangle=100)
    assert m.cell_res[0].tolist() == [64, 64, 64]
    small = MeshScene.from_triangles([big[:10]], [torch.ones(10, dtype=torch.int32)])
    assert int(small.cell_res[0].prod()) <= 4 * 2 * 10


@pytest.mark.parametrize("bad", ["nan", "shape", "ids_len", "ids_float", "id_zero", "env_count"])
def test_malformed_input_is_rejected(bad):
    t = [torch.rand(4, 3, 3)]
    i = [torch.ones(4, dtype=torch.int32)]
    if bad == "nan":
        t[0][1, 2, 0] = float("nan")
    elif bad == "shape":
        t = [torch.rand(4, 3)]
    elif bad == "ids_len":
        i = [torch.ones(3, dtype=torch.int32)]
    elif bad == "ids_float":
        i = [torch.ones(4)]
    elif bad == "id_zero":
        i = [torch.zeros(4, dtype=torch.int32)]
    else:
        i = i + i
    with pytest.raises(ValueError):
        MeshScene.from_triangles(t, i)

"""CPU: the mesh-to-env set-up path -- env/mesh_io.load_obj, MeshScene.surface_points and MeshScene.grid_spec /
ground_truth's input checks (the voxelizer itself runs on the GPU: tests/test_voxelize_gpu.py)."""
import math

import pytest
import torch

from gennbv_amd import _lib
from gennbv_amd.env import synthetic as S
from gennbv_amd.env.mesh_io import load_obj
from gennbv_amd.env.mesh_scene import MeshScene, box_triangles, sphere_triangles


def _write(tmp_path, text, name="m.obj"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_obj_quads_ngons_and_vertex_reference_forms(tmp_path):
    p = _write(tmp_path, """# a quad, a pentagon and a triangle in every reference form
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vn 0 0 1
f 1/1/1 2/1/1 3/1/1 4/1/1
v 0 0 1
v 1 0 1
v 2 1 1
v 1 2 1
v 0 1 1
f 5//1 6//1 7//1 8//1 9//1
f 1/1 2 5
usemtl foo
s off
l 1 2
""")
    tris, ids = load_obj(p, recenter=False)
    assert tris.dtype == torch.float32 and ids.dtype == torch.int32
    assert tris.shape == (2 + 3 + 1, 3, 3) and ids.tolist() == [1] * 6
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [2, 1, 1], [1, 2, 1], [0, 1, 1.0]])
    want = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7), (4, 7, 8), (0, 1, 4)]  # fans around the first vertex
    for t, w in zip(tris, want):
        assert torch.equal(t, v[list(w)])


def test_obj_negative_indices_are_relative(tmp_path):
    p = _write(tmp_path, "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\nv 0 0 5\nf -4/1/1 -3//2 -1\n")
    tris, _ = load_obj(p, recenter=False)
    assert torch.equal(tris[0], torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0.0]]))
    assert torch.equal(tris[1], torch.tensor([[0, 0, 0], [1, 0, 0], [0, 0, 5.0]]))


def test_obj_groups_number_in_order_of_first_appearance(tmp_path):
    p = _write(tmp_path, """v 0 0 0
v 1 0 0
v 0 1 0
f 1 2 3
o roof
f 1 2 3
g walls
f 1 2 3
f 1 2 3
o roof
f 1 2 3
g door
f 1 2 3
""")
    _, ids = load_obj(p, recenter=False)
    assert ids.tolist() == [1, 1, 2, 2, 1, 3]


def test_obj_y_up_and_recentering(tmp_path):
    p = _write(tmp_path, "v 1 2 3\nv 5 2 3\nv 1 6 -1\nf 1 2 3\n")
    raw, _ = load_obj(p, recenter=False)
    assert torch.equal(raw[0], torch.tensor([[1, 2, 3], [5, 2, 3], [1, 6, -1.0]]))
    yup, _ = load_obj(p, up="y", recenter=False)
    # (x, y, z) -> (x, -z, y): a proper rotation (+90 deg about x), the file's up (+y) becomes +z
    assert torch.equal(yup[0], torch.tensor([[1, -3, 2], [5, -3, 2], [1, 1, 6.0]]))
    c, _ = load_obj(p)
    p_ = c.reshape(-1, 3)
    assert float(p_[:, 2].min()) == 0.0
    assert float(p_[:, 0].min()) == -float(p_[:, 0].max()) and float(p_[:, 1].min()) == -float(p_[:, 1].max())
    assert torch.allclose(c - c[0, 0], raw - raw[0, 0])  # a translation only
    cy, _ = load_obj(p, up="y")
    q = cy.reshape(-1, 3)
    assert float(q[:, 2].min()) == 0.0 and float(q[:, 2].max()) == 4.0  # y spanned 2..6
    assert float(q[:, 0].min()) == -2.0 and float(q[:, 0].max()) == 2.0


@pytest.mark.parametrize("text,line,what", [
    ("v 0 0 0\nv 1 0\n", 2, "x y z"),
    ("v 0 0 0\nv 1 0 zz\n", 2, "bad vertex"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\n\n# c\nf 1 2\n", 6, "at least 3"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 4, "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", 4, "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -4\n", 4, "out of range"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x/1\n", 4, "bad vertex reference"),
])
def test_obj_errors_name_the_line(tmp_path, text, line, what):
    p = _write(tmp_path, text)
    with pytest.raises(ValueError, match=rf"m\.obj:{line}: .*{what}"):
        load_obj(p)


def test_obj_bad_up_axis(tmp_path):
    with pytest.raises(ValueError):
        load_obj(_write(tmp_path, "v 0 0 0\n"), up="x")


# ---------------------------------------------------------------------------------------------------------------
def _two_env_mesh():
    lo = torch.tensor([[-3.0, -2.0, 0.0], [1.0, 1.0, 0.0]])
    hi = torch.tensor([[-1.0, 2.0, 4.0], [3.5, 2.0, 2.5]])
    boxes = box_triangles(lo, hi)
    sphere = sphere_triangles([0.5, -1.0, 3.0], 1.5, 6, 12)
    tris = [boxes, torch.cat([sphere, boxes[:12]])]
    ids = [torch.ones(t.shape[0], dtype=torch.int32) for t in tris]
    return MeshScene.from_triangles(tris, ids)


def _dist_to_triangle(p, t):
    """(distance to the plane, barycentric coordinates of the projection) of points p [P,3] on triangles t [P,3,3], fp64."""
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    n = torch.linalg.cross(b - a, c - a, dim=-1)
    n = n / n.norm(dim=-1, keepdim=True)
    plane = ((p - a) * n).sum(-1).abs()
    # barycentric coordinates of the projection
    q = p - ((p - a) * n).sum(-1, keepdim=True) * n
    v0, v1, v2 = b - a, c - a, q - a
    d00, d01, d11 = (v0 * v0).sum(-1), (v0 * v1).sum(-1), (v1 * v1).sum(-1)
    d20, d21 = (v2 * v0).sum(-1), (v2 * v1).sum(-1)
    den = d00 * d11 - d01 * d01
    v = (d11 * d20 - d01 * d21) / den
    w = (d00 * d21 - d01 * d20) / den
    return plane, torch.stack([1 - v - w, v, w], -1)


def test_surface_points_lie_on_their_triangles_and_follow_area():
    m = _two_env_mesh()
    pts = m.surface_points(20000, seed=3)
    assert len(pts) == 2
    for e in range(2):
        p = pts[e].double()
        assert pts[e].dtype == torch.float32 and p.shape == (20000, 3)
        t = m.env_triangles(e)[0].double()
        # nearest triangle of every point: on it within 1e-6 m
        area = 0.5 * torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], dim=-1).norm(dim=-1)
        best = torch.full((p.shape[0],), float("inf"), dtype=torch.float64)
        owner = torch.zeros(p.shape[0], dtype=torch.int64)
        for k in range(t.shape[0]):
            plane, bary = _dist_to_triangle(p, t[k].expand(p.shape[0], 3, 3))
            inside = (bary >= -1e-6).all(-1)
            d = torch.where(inside, plane, torch.full_like(plane, float("inf")))
            better = d < best
            owner = torch.where(better, torch.full_like(owner, k), owner)
            best = torch.minimum(best, d)
        assert float(best.max()) <= 1e-6, float(best.max())
        # counts per triangle follow the area: chi-square with T - 1 degrees of freedom, far below its 1e-6 tail
        cnt = torch.bincount(owner, minlength=t.shape[0]).double()
        exp = area / area.sum() * p.shape[0]
        chi2 = float(((cnt - exp) ** 2 / exp).sum())
        dof = t.shape[0] - 1
        assert chi2 < dof + 8 * math.sqrt(2 * dof), (chi2, dof)


def test_surface_points_are_seeded():
    m = _two_env_mesh()
    a, b, c = m.surface_points(500, seed=7), m.surface_points(500, seed=7), m.surface_points(500, seed=8)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])


def test_surface_points_empty_env_and_zero_area():
    flat = torch.tensor([[[0.0, 0, 1], [1, 0, 1], [2, 0, 1]]])  # collinear: zero area
    m = MeshScene.from_triangles([torch.zeros(0, 3, 3), flat], [torch.zeros(0, dtype=torch.int32), torch.ones(1, dtype=torch.int32)])
    p = m.surface_points(50)
    assert p[0].shape == (0, 3)
    assert p[1].shape == (50, 3) and torch.all(p[1][:, 1] == 0) and torch.all(p[1][:, 2] == 1)
    assert float(p[1][:, 0].min()) >= 0 and float(p[1][:, 0].max()) <= 2


# ---------------------------------------------------------------------------------------------------------------
def test_grid_spec_default_range_follows_the_reference_frame():
    m = _two_env_mesh()
    rng, vox = m.grid_spec(33)
    for e in range(2):
        t = m.env_triangles(e)[0].reshape(-1, 3)
        mx, my, mz = float(t[:, 0].abs().max()), float(t[:, 1].abs().max()), float(t[:, 2].max())
        assert rng[e].tolist() == [mx, -mx, my, -my, mz, 0.0]
    want = torch.stack([rng[:, 0] - rng[:, 1], rng[:, 2] - rng[:, 3], rng[:, 4] - rng[:, 5]], -1) / 32
    assert torch.equal(vox, want) and rng.dtype == torch.float32 and vox.dtype == torch.float32


def test_grid_spec_explicit_range_is_used_as_is_and_matches_make_scenes():
    sc = S.make_scenes(3, 20, seed=2)
    m = MeshScene.from_boxes(sc)
    rng, vox = m.grid_spec(20, sc.range_gt)
    assert torch.equal(rng, sc.range_gt) and torch.equal(vox, sc.voxel_size)


def test_grid_spec_and_ground_truth_refuse_bad_input():
    m = _two_env_mesh()
    with pytest.raises(ValueError):
        m.grid_spec(1)
    with pytest.raises(ValueError):
        m.grid_spec(2000)
    with pytest.raises(ValueError, match="range_gt must be"):
        m.grid_spec(16, torch.zeros(3, 6))
    bad = torch.tensor([[1.0, -1, 1, -1, 1, 0], [1.0, 1, 1, -1, 1, 0]])  # x max == min in env 1
    with pytest.raises(ValueError, match="max > min"):
        m.grid_spec(16, bad)
    with pytest.raises(ValueError, match="max > min"):
        m.ground_truth(16, bad)
    # an env without triangles, or flat on an axis, needs an explicit range
    tri = torch.tensor([[[1.0, -1, 2], [2, 1, 2], [1, 1, 3]]])
    one = torch.ones(1, dtype=torch.int32)
    empty = MeshScene.from_triangles([tri, torch.zeros(0, 3, 3)], [one, torch.zeros(0, dtype=torch.int32)])
    with pytest.raises(ValueError, match="env 1 has no triangles"):
        empty.ground_truth(16)
    rng, _ = empty.grid_spec(16, torch.tensor([[4.0, -4, 4, -4, 4, 0]] * 2))
    assert rng.shape == (2, 6)
    on_ground = MeshScene.from_triangles([torch.tensor([[[1.0, -1, 0], [2, 1, 0], [1, 1, 0]]])], [one])
    with pytest.raises(ValueError, match="zero extent"):
        on_ground.grid_spec(16)
    # valid input on a CPU scene: no CPU fallback
    with pytest.raises(_lib.GennbvHipError):
        m.ground_truth(16)


def test_default_env_origins_are_make_scenes_layout():
    sc = S.make_scenes(7, 8, seed=1)
    assert torch.equal(S.default_env_origins(7), sc.env_origins)

"""CPU: the collision oracle on hand cases and against dense point sampling, MeshScene.objects() and CollisionBody."""
import math

import numpy as np
import pytest
import torch

from tests.collision_oracle import GROUND, SURFACE, CollisionOracle, axes, hand_cases, lowest_point


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_oracle_hand_cases(case):
    name, tris, ids, pose, r, h, ground, expected = case
    o = CollisionOracle([tris], [ids])
    code = o.codes([0], np.array([pose], np.float32), float(np.float32(r)), float(np.float32(h)), ground)
    assert int(code[0]) == expected, name


def test_ground_depths_in_the_docs():
    """fp32(0.1) = r: pitch 60 deg clears the ground, 75 deg reaches 1.8 mm below it, 90 deg about 1e-9 m."""
    r, z = float(np.float32(0.1)), float(np.float32(0.1))
    deg = lambda x: float(np.float32(math.radians(x)))  # noqa: E731
    assert lowest_point([0, 0, z, 0, deg(60), 0], r, 0.02) > 3e-3
    assert -1.9e-3 < lowest_point([0, 0, z, 0, deg(75), 0], r, 0.02) < -1.7e-3
    assert -1e-9 < lowest_point([0, 0, z, 0, float(np.float32(math.pi / 2)), 0], r, 0.02) < -5e-10


def test_axis_is_quat_from_euler_xyz():
    """a = Rz(yaw) Ry(pitch) Rx(roll) e_z, written out as in the contract."""
    rs = np.random.RandomState(0)
    p = rs.uniform(-3, 3, (50, 6)).astype(np.float32)
    a = axes(p)
    for k in range(50):
        r_, p_, y_ = (float(x) for x in p[k, 3:6])
        Rx = np.array([[1, 0, 0], [0, math.cos(r_), -math.sin(r_)], [0, math.sin(r_), math.cos(r_)]])
        Ry = np.array([[math.cos(p_), 0, math.sin(p_)], [0, 1, 0], [-math.sin(p_), 0, math.cos(p_)]])
        Rz = np.array([[math.cos(y_), -math.sin(y_), 0], [math.sin(y_), math.cos(y_), 0], [0, 0, 1]])
        np.testing.assert_allclose(a[k], (Rz @ Ry @ Rx)[:, 2], atol=1e-15)


def test_oracle_against_dense_point_sampling():
    """One-sided: a sampled triangle point inside the solid cylinder forces (S)."""
    rs = np.random.RandomState(1)
    r, h = 0.1, 0.05
    m = 400
    tris = (rs.uniform(-0.3, 0.3, (m, 3, 3))).astype(np.float32)
    poses = np.zeros((m, 6), np.float32)
    poses[:, 3:6] = rs.uniform(-math.pi, math.pi, (m, 3))
    k = 40
    u, v = np.meshgrid(np.linspace(0, 1, k + 1), np.linspace(0, 1, k + 1))
    keep = (u + v) <= 1
    u, v = u[keep], v[keep]
    a = axes(poses)
    forced = 0
    for i in range(m):
        t = tris[i].astype(np.float64)
        pts = t[0] + u[:, None] * (t[1] - t[0]) + v[:, None] * (t[2] - t[0])
        s = pts @ a[i]
        perp = pts - s[:, None] * a[i]
        inside = (np.abs(s) <= h) & ((perp * perp).sum(1) <= r * r)
        code = CollisionOracle([tris[i:i + 1]], [np.ones(1, np.int32)]).codes([0], poses[i:i + 1], r, h)[0]
        if inside.any():
            forced += 1
            assert code & SURFACE, i
    assert forced > 50


def test_objects_index_on_a_cpu_scene():
    from gennbv_amd.env.mesh_scene import MeshScene, box_triangles, sphere_triangles
    b = box_triangles(torch.tensor([[0., 0, 0], [2, 2, 2]]), torch.tensor([[1., 1, 1], [3, 4, 5]]))
    s = sphere_triangles((5.0, 0.0, 1.0), 1.0, 6, 8)
    t0 = torch.cat([b[12:], s, b[:12]])  # ids not sorted in triangle order
    i0 = torch.cat([torch.full((12,), 7), torch.full((s.shape[0],), 3), torch.full((12,), 9)]).int()
    t2 = b[:12]
    i2 = torch.full((12,), 1, dtype=torch.int32)
    mesh = MeshScene.from_triangles([t0, torch.zeros(0, 3, 3), t2], [i0, torch.zeros(0, dtype=torch.int32), i2])
    o = mesh.objects()
    assert o is mesh.objects()  # built once
    assert o["env_obj_start"].tolist() == [0, 3, 3, 4]
    assert o["obj_id"].tolist() == [3, 7, 9, 1]
    start = o["obj_tri_start"].tolist()
    base = [0, int(mesh.tri_count[0]), int(mesh.tri_count[0])]
    for k, (e, oid) in enumerate([(0, 3), (0, 7), (0, 9), (2, 1)]):
        tris, ids = mesh.env_triangles(e)
        want = (torch.nonzero(ids == oid).flatten() + base[e]).tolist()
        got = o["obj_tris"][start[k]:start[k + 1]].tolist()
        assert got == want
        v = mesh.tris[got].reshape(-1, 3)
        assert torch.equal(o["obj_aabb"][k], torch.cat([v.amin(0), v.amax(0)]))
    for key in ("env_obj_start", "obj_tri_start", "obj_tris", "obj_id"):
        assert o[key].dtype == torch.int32 and o[key].is_contiguous()


def test_collide_refuses_cpu_scene():
    from gennbv_amd import _lib
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.mesh_scene import MeshScene, box_triangles
    mesh = MeshScene.from_triangles([box_triangles(torch.zeros(1, 3), torch.ones(1, 3))], [torch.ones(12, dtype=torch.int32)])
    with pytest.raises(_lib.GennbvHipError):
        mesh.collide(torch.zeros(1, 6), CollisionBody())


def test_collision_body_validation():
    from gennbv_amd.env.collision import CollisionBody
    b = CollisionBody()
    assert (b.radius, b.half_length, b.ground) == (0.1, 0.02, False)
    assert CollisionBody(0.2, 0.0, True).half_length == 0.0
    for r, h in [(0.0, 0.02), (-0.1, 0.02), (0.1, -1e-3), (float("nan"), 0.02), (0.1, float("inf")), (float("inf"), 0.02)]:
        with pytest.raises(ValueError):
            CollisionBody(r, h)


def test_ground_bit_matches_the_closed_form():
    rs = np.random.RandomState(3)
    p = np.zeros((2000, 6), np.float32)
    p[:, 2] = rs.uniform(0.0, 0.2, 2000)
    p[:, 3:6] = rs.uniform(-math.pi, math.pi, (2000, 3))
    o = CollisionOracle([np.zeros((0, 3, 3), np.float32)], [np.zeros(0, np.int32)])
    code = o.codes(np.zeros(2000, np.int64), p, 0.1, 0.02, ground=True)
    low = np.array([lowest_point(q, 0.1, 0.02) for q in p])
    assert np.array_equal(code == GROUND, low <= 0) and 300 < int((code == GROUND).sum()) < 1900

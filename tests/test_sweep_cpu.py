"""CPU: the fp64 oracle of the swept flight path (tests/sweep_oracle.py) on hand cases with known answers, and
CollisionBody's sweep fields."""
import math

import numpy as np
import pytest

from gennbv_amd.env.collision import CF2X_HALF_LENGTH, CF2X_RADIUS, GROUND, INSIDE, PATH, PATH_GROUND, SURFACE, CollisionBody
from tests import sweep_oracle as SO


@pytest.mark.parametrize("case", SO.hand_cases(), ids=lambda c: c[0])
def test_hand_cases_on_the_oracle(case):
    name, tris, a, b, radius, ground, expected = case
    o = SO.SweepOracle([tris])
    code, robust = o.robust_codes([0], np.array([a], np.float32), np.array([b], np.float32), radius, ground)
    assert bool(robust[0]), name  # every hand case sits 1e-3 m from the boundary, the band is 1e-6 m
    assert int(code[0]) == expected, name


def test_oracle_distance_against_closed_forms():
    # a unit right triangle in the plane z = 0
    t = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float64)
    pt = lambda *p: np.array([p], np.float64)  # noqa: E731
    assert SO.point_triangle(pt(0.25, 0.25, 2.0), t)[0] == pytest.approx(2.0, abs=1e-15)  # above the face
    assert SO.point_triangle(pt(-3.0, -4.0, 0.0), t)[0] == pytest.approx(5.0, abs=1e-15)  # the vertex region
    assert SO.point_triangle(pt(0.5, -2.0, 0.0), t)[0] == pytest.approx(2.0, abs=1e-15)  # an edge region
    assert SO.point_triangle(pt(1.0, 1.0, 0.0), t)[0] == pytest.approx(math.sqrt(0.5), abs=1e-15)  # the hypotenuse
    # segments: piercing, skew above an edge, parallel above the face
    assert SO.segment_triangle(pt(0.2, 0.2, 1.0), pt(0.3, 0.3, -1.0), t)[0] == pytest.approx(0.0, abs=1e-9)
    assert SO.segment_triangle(pt(0.5, -1.0, 0.7), pt(0.5, -1.0, -3.0), t)[0] == pytest.approx(1.0, abs=1e-9)
    assert SO.segment_triangle(pt(-5.0, 0.1, 0.3), pt(5.0, 0.1, 0.3), t)[0] == pytest.approx(0.3, abs=1e-9)
    # a skew segment whose nearest point is interior to it and nearest the vertex (1, 0, 0)
    d = SO.segment_triangle(pt(3.0, -2.0, 1.0), pt(1.0, -2.0, -1.0), t)[0]
    assert d == pytest.approx(math.sqrt(4.5), abs=1e-9)  # |(x, -2, x - 2) - (1, 0, 0)|^2 = (x - 1)^2 + 4 + (x - 2)^2, least at x = 1.5


def test_oracle_gates_and_non_finite():
    box = SO.hand_cases()[0][1]
    o = SO.SweepOracle([box, box])
    a = np.array([[2.0, 0, 5], [2.0, 0, 5], [np.nan, 0, 5]], np.float32)
    b = np.array([[0.0, 0, 5], [0.0, 0, 5], [0.0, 0, 5]], np.float32)
    code, robust = o.robust_codes([0, 1, 1], a, b, 0.1, True, episode_length=[2, 1, 5])
    assert code.tolist() == [PATH, 0, 0] and robust.all()
    # inside the band: not robust
    g = 0.1 + 2e-7
    code, robust = o.robust_codes([0], np.array([[1 + g, -0.5, 5]]), np.array([[1 + g, 0.5, 5]]), 0.1)
    assert not robust[0]


def test_bits_share_one_byte():
    assert (SURFACE, INSIDE, GROUND, PATH, PATH_GROUND) == (1, 2, 4, 8, 16)
    assert (SO.PATH, SO.PATH_GROUND) == (PATH, PATH_GROUND)


def test_collision_body_sweep_fields():
    b = CollisionBody()
    assert b.sweep is False and b.sweep_radius is None
    assert b.path_radius == math.sqrt(CF2X_RADIUS ** 2 + CF2X_HALF_LENGTH ** 2)
    # positional construction is unchanged: radius, half_length, ground come first
    p = CollisionBody(0.3, 0.4, True)
    assert (p.radius, p.half_length, p.ground, p.sweep, p.sweep_radius) == (0.3, 0.4, True, False, None)
    assert p.path_radius == pytest.approx(0.5, abs=1e-15)
    q = CollisionBody(0.3, 0.4, False, True, 0.25)
    assert q.sweep is True and q.sweep_radius == 0.25 and q.path_radius == 0.25
    assert CollisionBody(sweep=1).sweep is True
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            CollisionBody(sweep=True, sweep_radius=bad)
    with pytest.raises(Exception):
        b.sweep = True  # frozen
    assert CollisionBody(sweep=True) == CollisionBody(sweep=True) and CollisionBody(sweep=True) != CollisionBody()


def test_sweep_refuses_cpu_scene():
    import torch

    from gennbv_amd import _lib
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.mesh_scene import MeshScene
    mesh = MeshScene.from_boxes(S.make_scenes(2, 20, seed=1), device="cpu")
    with pytest.raises(_lib.GennbvHipError):
        mesh.sweep(torch.zeros(2, 6), torch.zeros(2, 6), CollisionBody())
    with pytest.raises(_lib.GennbvHipError):
        mesh.sweep_candidates(torch.zeros(2, 6), torch.zeros(2, 4, 6), CollisionBody())

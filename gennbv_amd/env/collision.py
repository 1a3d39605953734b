"""CollisionBody: the drone's collision solid for the closed-loop env's collision termination (csrc/collide.hip).

The reference terminates an episode when the cf2x body reports contact forces (check_termination,
gennbv/env/env_train_gennbv.py:438-457; termination.collision = True in the shipped config).  Here the body is the
`base_link` collision cylinder of resources/robots/drone/cf2x.urdf -- radius 0.1 m, length 0.04 m -- centred at the pose's
(x, y, z) with axis R e_z, R = Rz(yaw) Ry(pitch) Rx(roll); the prop links have no collision geometry.  The objects of the
scene are closed solids (MeshScene.collide).

`ground` (off by default) also counts the half-space z <= 0 as an obstacle.  The lowest lattice z is fp32(0.1) == r, so a
tilted body at that height reaches below the ground: about 1e-9 m at pitch +-90 deg (fp32 pi/2 is not exact) and 1.8 mm at
pitch +-75 deg.  The reference's PhysX shapes use contact_offset 0.01 and rest_offset 0
(legged_gym/env/base/legged_robot_config.py:232-233); whether PhysX reports a force in these cases is not known here, so
the ground stays an opt-in.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

CF2X_RADIUS = 0.1
CF2X_HALF_LENGTH = 0.02

# bits of the contact code (gnbv_collide_cylinder)
SURFACE = 1  # (S) a triangle meets the body
INSIDE = 2  # (I) no triangle does, the centre lies inside an object
GROUND = 4  # (G) the body reaches z <= 0 (ground enabled)


@dataclass(frozen=True)
class CollisionBody:
    """A closed solid cylinder: radius > 0, half_length >= 0 (metres), and whether z <= 0 is an obstacle."""
    radius: float = CF2X_RADIUS
    half_length: float = CF2X_HALF_LENGTH
    ground: bool = False

    def __post_init__(self):
        r, h = float(self.radius), float(self.half_length)
        if not (math.isfinite(r) and math.isfinite(h)):
            raise ValueError(f"CollisionBody: radius and half_length must be finite, got {self.radius}, {self.half_length}")
        if not r > 0.0:
            raise ValueError(f"CollisionBody: radius must be > 0, got {self.radius}")
        if not h >= 0.0:
            raise ValueError(f"CollisionBody: half_length must be >= 0, got {self.half_length}")
        object.__setattr__(self, "radius", r)
        object.__setattr__(self, "half_length", h)
        object.__setattr__(self, "ground", bool(self.ground))

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

`sweep` (off by default) also tests the straight flight from the previous pose to the new one (csrc/sweep.hip,
MeshScene.sweep): the sphere of radius `path_radius` moved along the segment between the two positions.  The body turns in
flight, so the orientation-independent solid is the sphere that bounds the cylinder, sqrt(radius^2 + half_length^2) unless
`sweep_radius` says otherwise; it is conservative -- it never passes a path the cylinder could not fly.  The first pose of an
episode is set, not flown to.  With `ground` on, the lowest lattice layer (z = fp32(0.1)) is unreachable for any
path_radius >= 0.1 (min z - R <= 0 on every flight that starts or ends there): one more reason the ground stays an opt-in.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

CF2X_RADIUS = 0.1
CF2X_HALF_LENGTH = 0.02

# bits of the contact code (gnbv_collide_cylinder)
SURFACE = 1  # (S) a triangle meets the body
INSIDE = 2  # (I) no triangle does, the centre lies inside an object
GROUND = 4  # (G) the body reaches z <= 0 (ground enabled)
# bits of the path code (gnbv_sweep_sphere), in the same byte
PATH = 8  # a triangle comes within path_radius of the straight flight between two poses
PATH_GROUND = 16  # the swept sphere reaches z <= 0 (ground enabled)


@dataclass(frozen=True)
class CollisionBody:
    """A closed solid cylinder: radius > 0, half_length >= 0 (metres), and whether z <= 0 is an obstacle.  `sweep`: the
    flight between consecutive poses is tested too, with the sphere of radius `path_radius` (`sweep_radius`, finite and > 0, or
    the cylinder's bounding sphere)."""
    radius: float = CF2X_RADIUS
    half_length: float = CF2X_HALF_LENGTH
    ground: bool = False
    sweep: bool = False
    sweep_radius: Optional[float] = None

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
        object.__setattr__(self, "sweep", bool(self.sweep))
        if self.sweep_radius is not None:
            sr = float(self.sweep_radius)
            if not (math.isfinite(sr) and sr > 0.0):
                raise ValueError(f"CollisionBody: sweep_radius must be finite and > 0, got {self.sweep_radius}")
            object.__setattr__(self, "sweep_radius", sr)

    @property
    def path_radius(self) -> float:
        """Radius of the sphere swept along a flight: sweep_radius, or the cylinder's bounding sphere sqrt(r^2 + h^2)."""
        if self.sweep_radius is not None:
            return self.sweep_radius
        return math.sqrt(self.radius * self.radius + self.half_length * self.half_length)

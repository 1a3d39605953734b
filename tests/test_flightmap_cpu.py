"""CPU: the numpy oracle of gnbv_flight_blocked_tri (tests/flightmap_oracle.py) on hand-made cases, the entry point's argument
refusals (all made before any launch, so they need no GPU), and the parts of the belief flight that refuse to run off the GPU."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.flight import FlightLattice
from tests import flightmap_oracle as MO

f32, f64 = np.float32, np.float64
INVALID = 1  # hipErrorInvalidValue

# a 4^3 grid of unit voxels over [0, 4]^3: range_min - 0.5 v = 0 on every axis (range_gt rows are max, min per axis)
RANGE = np.array([[3.5, 0.5, 3.5, 0.5, 3.5, 0.5]], f32)
VOX = np.ones((1, 3), f32)


def _grid(fill=-1, occupied=(), unknown=()):
    tri = np.full((1, 4, 4, 4), fill, np.int8)
    for x, y, z in occupied:
        tri[0, x, y, z] = 1
    for x, y, z in unknown:
        tri[0, x, y, z] = 0
    return tri


def _line(xs, y=1.5, z=1.5):
    """A lattice of len(xs) evenly spaced nodes along x at height z: (dims, lo, h)."""
    step = xs[1] - xs[0] if len(xs) > 1 else 0.0
    return (len(xs), 1, 1), np.array([xs[0], y, z], f64), np.array([step, 0.0, 0.0], f64)


def test_voxel_frame_is_pose_to_idx_s():
    o, v = MO.voxel_frame(RANGE[0], VOX[0])
    assert o.tolist() == [0.0, 0.0, 0.0] and v.tolist() == [1.0, 1.0, 1.0]
    r = np.array([7.3, -7.3, 7.3, -7.3, 11.9, 0.1], f32)
    vs = np.array([0.77, 0.77, 0.6], f32)
    o, v = MO.voxel_frame(r, vs)
    want = [f64(f32(r[2 * a + 1]) - f32(f32(0.5) * vs[a])) for a in range(3)]  # the subtraction in fp32, then widened
    assert o.tolist() == want and v.tolist() == [f64(x) for x in vs]
    assert o[0] != f64(r[1]) - 0.5 * f64(vs[0])  # not the fp64 difference


def test_one_occupied_voxel_and_nodes_on_both_sides_of_rho():
    tri = _grid(occupied=[(2, 1, 1)])  # the voxel [2, 3] x [1, 2] x [1, 2]
    rho = 0.5
    # along x through the voxel's middle: the gap to the face x = 2 is 2 - p, to the face x = 3 it is p - 3 (binary fractions: exact)
    xs = [1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75]
    dims, lo, h = _line(xs)
    got = MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, rho)[0]
    # gap 0.5 == rho touches (<=) from below; from above, 3.5 - rho = 3.0 puts the window's first voxel at 3: voxel 2 is not in it
    assert got.tolist() == [False, True, True, True, True, True, True, True, True, False, False]
    # off the corner: the node (1.75, 0.75, 0.75) has gaps (0.25, 0.25, 0.25), distance sqrt(3) / 4 = 0.433...
    dims, lo, h = (1, 1, 1), np.array([1.75, 0.75, 0.75]), np.zeros(3)
    assert MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, 0.4375)[0, 0]
    assert not MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, 0.4325)[0, 0]
    assert not MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, 0.25)[0, 0]  # inside every axis window, outside the ball
    # an unknown voxel blocks only by flag; a free one never
    tri = _grid(unknown=[(2, 1, 1)])
    dims, lo, h = _line([1.25, 1.75])
    assert MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, rho)[0].tolist() == [False, False]
    assert MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, rho, unknown_blocks=True)[0].tolist() == [False, True]
    # the int8 extremes keep their signs
    tri = _grid(fill=-128, occupied=[(2, 1, 1)])
    tri[tri > 0] = 127
    assert MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, rho, unknown_blocks=True)[0].tolist() == [False, True]


def test_the_outside_rule():
    tri = _grid()
    rho = 0.5
    xs = [0.25, 0.5, 0.75, 3.25, 3.5, 3.75, 4.5]
    want = [True, False, False, False, False, True, True]  # p - rho < 0 or p + rho > 4, strictly
    for i, x in enumerate(xs):
        dims, lo, h = (1, 1, 1), np.array([x, 1.5, 1.5]), np.zeros(3)
        assert MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, rho, outside_blocks=True)[0, 0] == want[i], x
        assert not MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, rho)[0, 0]
    # any axis
    dims, lo, h = (1, 1, 1), np.array([1.5, 1.5, 3.75]), np.zeros(3)
    assert MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, rho, outside_blocks=True)[0, 0]


def test_the_ground_rule():
    tri = _grid()
    for z, want in ((0.25, True), (0.5, True), (0.75, False)):  # p_z - rho <= 0
        dims, lo, h = (1, 1, 1), np.array([1.5, 1.5, z]), np.zeros(3)
        assert MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, 0.5, ground=True)[0, 0] == want
        assert not MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, 0.5)[0, 0]


def test_an_empty_window_is_free_whatever_the_grid_holds():
    tri = _grid(fill=1)  # all occupied
    rho = 0.5
    # -0.75: i1 = floor(-0.25) < 0, empty.  -0.5: i1 = floor(0.0) = 0, voxel 0 at gap 0.5 == rho, touched.  4.5: i0 = floor(4.0) = 4 > G - 1,
    # empty although the ball reaches the face x = 4: the rule is the window's, not the ball's.
    for p, want in (([-0.75, 1.5, 1.5], False), ([-0.5, 1.5, 1.5], True), ([4.25, 1.5, 1.5], True), ([4.5, 1.5, 1.5], False),
                    ([4.75, 1.5, 1.5], False), ([1.5, 9.0, 1.5], False), ([1.5, 1.5, -3.0], False)):
        dims, lo, h = (1, 1, 1), np.array(p, f64), np.zeros(3)
        assert MO.blocked_bool(tri, RANGE, VOX, dims, lo, h, rho)[0, 0] == want, p


def test_pack_words_sets_the_padding():
    b = np.zeros((2, 40), bool)
    b[0, [0, 31, 32]] = True
    w = MO.pack_words(b)
    assert w.dtype == np.uint32 and w.shape == (2, 2)
    assert w[0].tolist() == [0x80000001, 0xFFFFFF01] and w[1].tolist() == [0, 0xFFFFFF00]


# ---------------------------------------------------------------------------
# the C ABI refuses before it launches
# ---------------------------------------------------------------------------
def test_argument_refusals_at_the_c_abi():
    from gennbv_amd import _lib
    lib = _lib.load()
    assert lib.gnbv_abi_version() == 5
    cap = int(lib.gnbv_flightmap_lds_max_grid())
    lds = lambda g: 4 * ((2 * ((g ** 3 + 63) // 64) + 31) // 32 * 32)  # noqa: E731  whole ballots, whole groups of 32 words
    assert lds(cap) <= 160 * 1024 < lds(cap + 1) and cap == 109
    lo, h = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(0.5, 0.5, 0.5)
    fake = 0x1000  # never dereferenced: every call below is refused before a launch

    def call(i8=fake, i8_stride=8 ** 3, f32_=None, f32_stride=0, g=8, rng=fake, vox=fake, n=2, nx=9, ny=7, nz=5, lo_=lo, h_=h, rho=0.4,
             out=fake, mode=0):
        return lib.gnbv_flight_blocked_tri(i8, i8_stride, f32_, f32_stride, g, rng, vox, n, nx, ny, nz, lo_, h_, rho, 0, 0, 0, out, mode, None)
    nan_lo, bad_h = (C.c_double * 3)(0.0, math.nan, 0.0), (C.c_double * 3)(0.5, 0.0, 0.5)
    for kw in (dict(g=0), dict(g=129, i8_stride=129 ** 3), dict(rho=0.0), dict(rho=-1.0), dict(rho=math.inf), dict(rho=math.nan),
               dict(nx=0), dict(ny=1025), dict(nz=-1), dict(rng=None), dict(vox=None), dict(out=None), dict(lo_=None), dict(h_=None),
               dict(i8=None), dict(f32_=fake, f32_stride=8 ** 3), dict(mode=-1), dict(mode=3), dict(n=0), dict(i8_stride=8 ** 3 - 1),
               dict(i8=None, f32_=fake, f32_stride=8 ** 3 - 1), dict(lo_=nan_lo), dict(h_=bad_h),
               dict(g=cap + 1, i8_stride=(cap + 1) ** 3, mode=1)):
        assert call(**kw) == INVALID, kw


def test_belief_field_and_map_planner_refuse_what_they_cannot_run():
    from gennbv_amd import _lib
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.eval.baselines import MapGreedyPolicy
    from gennbv_amd.ops.flight_field import BeliefFlightField, FlightField
    assert issubclass(BeliefFlightField, FlightField) and BeliefFlightField.belief is True and not getattr(FlightField, "belief", False)
    lat = FlightLattice(TaskConfig(), stride=5)
    rng, vox = torch.tensor([[8.0, -8.0, 8.0, -8.0, 12.0, 0.0]] * 2), torch.full((2, 3), 0.8)
    with pytest.raises(_lib.GennbvHipError):
        BeliefFlightField(2, lat, CollisionBody(sweep=True), rng, vox, 20, device="cpu")
    for kw in (dict(unknown="maybe"), dict(outside="wall"), dict(map_mode=3)):
        with pytest.raises(ValueError):
            BeliefFlightField(2, lat, CollisionBody(sweep=True), rng, vox, 20, device="cpu", **kw)
    # the planner: an env without a belief field -- none at all, or a mesh-based one
    cfg = TaskConfig()
    for flight in (None, types.SimpleNamespace(num_envs=2), types.SimpleNamespace(num_envs=2, belief=False)):
        env = types.SimpleNamespace(cfg=cfg, num_envs=2, flight=flight, collision=None, device="cpu")
        with pytest.raises(_lib.GennbvHipError):
            MapGreedyPolicy(env, k=4, gain_backend=lambda tri, poses: None)

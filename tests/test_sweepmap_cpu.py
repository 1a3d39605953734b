"""CPU: the numpy oracle of gnbv_sweep_tri (tests/sweepmap_oracle.py) on hand-made cases, its robust share on the very inputs the
GPU tests use (tests/sweepmap_cases.py), the entry point's argument refusals (all made before any launch, so they need no GPU),
and the argument errors of BeliefFlightField's shortcut."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env.config import TaskConfig
from gennbv_amd.env.flight import FlightLattice
from tests import sweepmap_cases as SC
from tests import sweepmap_oracle as SO

f32, f64 = np.float32, np.float64
INVALID = 1  # hipErrorInvalidValue

# a 4^3 grid of unit voxels over [0, 4]^3: range_min - 0.5 v = 0 on every axis (range_gt rows are max, min per axis)
RANGE = np.array([[3.5, 0.5, 3.5, 0.5, 3.5, 0.5]], f32)
VOX = np.ones((1, 3), f32)
R = 0.5
EPS = 1e-3


def _grid(fill=-1, occupied=(), unknown=()):
    tri = np.full((1, 4, 4, 4), fill, np.int8)
    for x, y, z in occupied:
        tri[0, x, y, z] = 1
    for x, y, z in unknown:
        tri[0, x, y, z] = 0
    return tri


def _codes(tri, legs, radius=R, **flags):
    """Codes and robust flags of a list of (a, b) legs in the one env."""
    a = np.array([[l[0] for l in legs]], f32)
    b = np.array([[l[1] for l in legs]], f32)
    code, robust = SO.codes(tri, RANGE, VOX, a, b, radius, **flags)
    return code[0].tolist(), robust[0]


def test_one_occupied_voxel_beside_a_face_an_edge_and_a_corner():
    tri = _grid(occupied=[(2, 1, 1)])  # the box [2, 3] x [1, 2] x [1, 2]
    legs = []
    for d in (R - EPS, R + EPS):
        # beside the face x = 2, flown along y; beside the edge (x = 2, z = 1), flown along y; past the corner (2, 1, 1), flown
        # along (1, -1, 0), which is perpendicular to the corner's diagonal: the least distance is d at the leg's middle
        legs.append(([2 - d, 0.5, 1.5], [2 - d, 2.5, 1.5]))
        q = d / math.sqrt(2.0)
        legs.append(([2 - q, 0.5, 1 - q], [2 - q, 2.5, 1 - q]))
        q = d / math.sqrt(3.0)
        legs.append(([2 - q - 1, 1 - q + 1, 1 - q], [2 - q + 1, 1 - q - 1, 1 - q]))
    code, robust = _codes(tri, legs)
    assert code == [1, 1, 1, 0, 0, 0] and robust.all()
    # the least distances themselves
    a = np.array([[l[0] for l in legs]], f32)
    b = np.array([[l[1] for l in legs]], f32)
    d = SO.min_dist(tri, RANGE, VOX, a, b)[False][0]
    assert np.abs(d - np.array([R - EPS] * 3 + [R + EPS] * 3)).max() < 1e-6  # (fp32 legs)
    assert np.array_equal(d, SO.min_dist(tri, RANGE, VOX, a, b)[True][0])  # no unknown voxel: the flag changes nothing


def test_axis_parallel_zero_length_and_outside_starts():
    tri = _grid(occupied=[(2, 1, 1)])
    legs = [([0.5, 1.5, 1.5], [3.5, 1.5, 1.5]),              # along x, through the voxel
            ([0.5, 2 + R - EPS, 1.5], [3.5, 2 + R - EPS, 1.5]),  # along x, beside the face y = 2
            ([0.5, 2 + R + EPS, 1.5], [3.5, 2 + R + EPS, 1.5]),
            ([1.5 + EPS, 1.5, 1.5], [1.5 + EPS, 1.5, 1.5]),  # zero length: the ball test
            ([1.5 - EPS, 1.5, 1.5], [1.5 - EPS, 1.5, 1.5]),
            ([-2.0, 1.5, 1.5], [2.0, 1.5, 1.5]),             # starts outside the grid, ends on the face
            ([-2.0, 1.5, 1.5], [1.0, 1.5, 1.5]),             # starts outside, stops a metre short
            ([-2.0, 1.5, 1.5], [-1.0, 1.5, 1.5]),            # wholly outside
            ([2.5, 1.5, 9.0], [2.5, 1.5, 2 + R - EPS]),      # comes down from above the grid to just within R of the top face
            ([2.5, 1.5, 9.0], [2.5, 1.5, 2 + R + EPS]),
            ([math.nan, 1.5, 1.5], [2.5, 1.5, 1.5])]         # a non-finite coordinate: code 0
    code, robust = _codes(tri, legs)
    assert code == [1, 1, 0, 1, 0, 1, 0, 0, 1, 0, 0] and robust.all()
    # an all-occupied grid blocks everything that comes within R of it, and nothing else
    code, robust = _codes(_grid(fill=1), [([-2.0, 1.5, 1.5], [-R - EPS, 1.5, 1.5]), ([-2.0, 1.5, 1.5], [-R + EPS, 1.5, 1.5])])
    assert code == [0, 1] and robust.all()
    # an empty grid has no distance
    d = SO.min_dist(_grid(), RANGE, VOX, np.zeros((1, 1, 3), f32), np.ones((1, 1, 3), f32))
    assert np.isinf(d[False]).all() and np.isinf(d[True]).all()


def test_the_outside_and_ground_rules():
    tri = _grid()
    legs = [([1.0, 1.5, 1.5], [3.5 - EPS, 1.5, 1.5]),   # max + R stays below 4
            ([1.0, 1.5, 1.5], [3.5 + EPS, 1.5, 1.5]),   # max + R > 4
            ([0.5 - EPS, 1.5, 1.5], [2.0, 1.5, 1.5]),   # min - R < 0
            ([0.5, 1.5, 1.5], [2.0, 1.5, 1.5]),         # min - R == 0: strictly, so inside
            ([1.5, 1.5, 1.0], [1.5, 3.75, 1.0]),        # any axis
            ([1.5, 1.5, 0.5 + EPS], [1.5, 2.5, 2.0]),   # min z - R > 0
            ([1.5, 1.5, 2.0], [1.5, 2.5, 0.5]),         # min z - R == 0: <=, so the ground
            ([1.5, 1.5, 0.25], [1.5, 2.5, 2.0])]
    assert _codes(tri, legs)[0] == [0] * 8
    assert _codes(tri, legs, outside_blocks=True)[0] == [0, 2, 2, 0, 2, 0, 0, 2]
    assert _codes(tri, legs, ground=True)[0] == [0, 0, 0, 0, 0, 0, 4, 4]
    code, robust = _codes(tri, legs, outside_blocks=True, ground=True)
    assert code == [0, 2, 2, 0, 2, 0, 4, 6] and robust.all()


def test_an_unknown_voxel_under_both_flags():
    tri = _grid(unknown=[(2, 1, 1)])
    legs = [([0.5, 1.5, 1.5], [1.5 + EPS, 1.5, 1.5]), ([0.5, 1.5, 1.5], [1.5 - EPS, 1.5, 1.5])]
    assert _codes(tri, legs)[0] == [0, 0]
    code, robust = _codes(tri, legs, unknown_blocks=True)
    assert code == [1, 0] and robust.all()
    # the int8 extremes keep their signs
    tri = _grid(fill=-128, occupied=[(2, 1, 1)])
    tri[tri > 0] = 127
    assert _codes(tri, legs, unknown_blocks=True)[0] == [1, 0]


@pytest.mark.parametrize("g", [12, 8])
def test_robust_share_of_the_gpu_inputs(g):
    """At most 1 % of the items of every randomized case may be non-robust, on the very inputs tests/test_sweepmap_gpu.py uses; and
    the cases reach what they are there for."""
    frm, to, start = SC.legs(g)
    assert np.isnan(to[:, 39, 1]).all() and (frm[:, 37, :3] == to[:, 37, :3]).all()
    for broadcast in (False, True):
        for radius in SC.RADII:
            for flags in SC.FLAGS:
                code, robust = SC.want(g, broadcast, radius, flags)
                assert code.shape == (SC.N_ENVS, SC.K) and (~robust).sum() <= 0.01 * robust.size, (broadcast, radius, flags)
                assert (code[:, 39] == 0).all()  # the NaN item
    plain, _ = SC.want(g, False, 0.23, (0, 0, 0))
    assert not plain[1].any() and not plain[2].any()  # all free, all unknown: nothing blocks
    assert (plain[3, :28] == 1).all() and (plain[3, 29:31] == 0).all()  # all occupied: every leg that meets the grid
    assert 3 < (plain[0] == 1).sum() and 3 < (plain[5] == 1).sum() < SC.K - 3 and 3 < (plain[4] == 1).sum() < SC.K - 3
    thin, _ = SC.want(g, False, 0.06, (0, 0, 0))
    assert (thin[5] == 1).sum() < (plain[5] == 1).sum()  # the radius matters
    unk, _ = SC.want(g, False, 0.23, (1, 0, 0))
    assert (unk[2, :28] == 1).all() and ((unk & 1) >= (plain & 1)).all() and (unk[5] != plain[5]).any()
    full, _ = SC.want(g, False, 0.23, (0, 1, 1))
    assert (full & 2).any() and (full & 4).any() and ((full & 2) == 0).any() and ((full & 4) == 0).any()
    assert ((full[4] & 2) != 0).sum() >= SC.K - 4  # the small grid: almost every leg leaves it


# ---------------------------------------------------------------------------
# the C ABI refuses before it launches
# ---------------------------------------------------------------------------
def test_argument_refusals_at_the_c_abi():
    from gennbv_amd import _lib
    lib = _lib.load()
    assert lib.gnbv_abi_version() == 5
    cap = int(lib.gnbv_sweepmap_lds_max_grid())
    lds = lambda g: 4 * ((2 * ((g ** 3 + 63) // 64) + 31) // 32 * 32)  # noqa: E731  whole ballots, whole groups of 32 words
    assert lds(cap) <= 160 * 1024 < lds(cap + 1) and cap == 109 == int(lib.gnbv_flightmap_lds_max_grid())
    fake = 0x1000  # never dereferenced: every call below is refused before a launch

    def call(i8=fake, i8_stride=8 ** 3, f32_=None, f32_stride=0, g=8, rng=fake, vox=fake, n=2, frm=fake, f_env=6, f_item=0, to=fake, k=4,
             to_row=6, radius=0.4, out=fake, mode=0):
        return lib.gnbv_sweep_tri(i8, i8_stride, f32_, f32_stride, g, rng, vox, n, frm, f_env, f_item, to, k, to_row, radius, 0, 0, 0, out,
                                  mode, None)
    for kw in (dict(i8=None), dict(f32_=fake, f32_stride=8 ** 3),  # neither, both
               dict(rng=None), dict(vox=None), dict(frm=None), dict(to=None), dict(out=None),
               dict(n=0), dict(n=-1), dict(k=0), dict(k=-3), dict(g=0), dict(g=129, i8_stride=129 ** 3),
               dict(i8_stride=8 ** 3 - 1), dict(i8=None, f32_=fake, f32_stride=8 ** 3 - 1),
               dict(radius=0.0), dict(radius=-1.0), dict(radius=math.inf), dict(radius=math.nan),
               dict(mode=-1), dict(mode=3), dict(g=cap + 1, i8_stride=(cap + 1) ** 3, mode=1),
               dict(to_row=2), dict(f_env=2), dict(f_item=2), dict(f_item=-6), dict(n=2 ** 20, k=2 ** 11)):
        assert call(**kw) == INVALID, kw


def test_belief_field_shortcut_argument_errors():
    from gennbv_amd import _lib
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.eval.baselines import MapGreedyPolicy
    from gennbv_amd.ops.flight_field import BeliefFlightField
    lat = FlightLattice(TaskConfig(), stride=5)
    rng, vox = torch.tensor([[8.0, -8.0, 8.0, -8.0, 12.0, 0.0]] * 2), torch.full((2, 3), 0.8)
    body = CollisionBody(sweep=True)
    for margin in (-body.path_radius, -1.0, math.nan, math.inf):  # the swept radius must be finite and > 0
        with pytest.raises(ValueError):
            BeliefFlightField(2, lat, body, rng, vox, 20, device="cpu", shortcut=True, shortcut_margin=margin)
    with pytest.raises(_lib.GennbvHipError):  # GPU only, with the shortcut as without
        BeliefFlightField(2, lat, body, rng, vox, 20, device="cpu", shortcut=True, shortcut_margin=0.05)
    # the planner's shortcut needs the field's snapshot
    flight = types.SimpleNamespace(num_envs=2, belief=True, shortcut=False)
    env = types.SimpleNamespace(cfg=TaskConfig(), num_envs=2, flight=flight, collision=None, device="cpu")
    with pytest.raises(_lib.GennbvHipError):
        MapGreedyPolicy(env, k=4, gain_backend=lambda tri, poses: None, shortcut=True)

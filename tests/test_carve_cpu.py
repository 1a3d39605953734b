"""CPU: the oracle of the measured-frame view gain (tests/carve_oracle.py) against the view-gain oracles, the case table of
tests/carve_cases.py shown non-degenerate by the oracle alone, the refusals of the new GnbvViewGain fields (all made before any
launch, so they need no GPU), and CarvedMap's merge rule."""
import ctypes as C

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from oracle import oracle as O
from tests import carve_cases as CC
from tests import carve_oracle as CO
from tests import gain_masks_oracle as MO
from tests import view_gain_oracle as VO

INVALID = 1  # hipErrorInvalidValue


def _render(scene, poses):
    d, s, _, _ = S.render_depth(scene, poses, CC.H, CC.W, with_rgba=False)
    return d, s


def _update(scene, cfg, depth, seg, poses):
    """The voxel update of one frame by the CPU oracle (bit-equal to the updater's: tests/test_voxel_update_*)."""
    n, g = depth.shape[0], cfg.grid_size
    dp, sp = O.post_process_depth(depth.numpy(), seg.numpy(), cfg.depth_sense_dist)
    prob, scan = np.zeros((n, g, g, g), np.float32), np.zeros((n, g, g, g), np.float32)
    c2w = S.camera_to_world(poses).float().numpy()
    tri, _ = O.update_occ_grid(dp, sp, c2w, S.inverse_intrinsics(CC.H, CC.W, cfg.horizontal_fov).numpy(), poses[:, :3].numpy(),
                               scene.range_gt.numpy(), scene.voxel_size.numpy(), scene.grid_gt.numpy(), prob, scan)
    return torch.from_numpy(tri)


_BUILT = {}


def built(case):
    if case not in _BUILT:
        b = CC.build(case, _render, _update)
        b["c2w"] = S.camera_to_world(b["poses"].view(-1, 6)).float().view(CC.N, case[2], 4, 4).numpy()
        _BUILT[case] = b
    return _BUILT[case]


def _oracle_args(b):
    return (b["scene"].range_gt.numpy(), b["scene"].voxel_size.numpy(), b["kinv"], CC.H, CC.W, b["stride"], CC.RANGE)


def test_ray_lengths_are_the_updaters_depth_on_surface_rays():
    raw = np.array([-3.5, -12.0, -12.000001, -49.9, -50.0, -60.0, 3.0, 0.0, -0.0, np.nan, np.inf, -np.inf, -1e-3, 1e-30, -3e38],
                   np.float32)
    length, surface = CO.ray_lengths(raw, -50.0, 12.0)
    assert surface.tolist() == [True, True, False, False, False, False, True, False, False, False, False, False, True, True, False]
    dp, _ = O.post_process_depth(raw, np.zeros_like(raw), -50.0)
    assert np.array_equal(length[surface], dp[surface])  # exactly the depth the updater's A1 gives the pixel
    assert (length[~surface] == np.float32(12.0)).all()


@pytest.mark.parametrize("case", [(7, 1, 3), (16, 3, 1)])
def test_all_miss_depth_is_the_view_gain_oracle(case):
    b = built(case)
    miss = np.full((CC.N, b["k"], CC.H, CC.W), -np.inf, np.float32)
    args = _oracle_args(b)
    gain, ub, hb, carve = CO.measured(b["tri"].numpy(), b["c2w"], miss, *args, b["sense"])
    assert np.array_equal(gain, VO.view_gain(b["tri"].numpy(), b["c2w"], *args))
    ub0, hb0 = MO.masks(b["tri"].numpy(), b["c2w"], *args)
    assert np.array_equal(ub, ub0) and np.array_equal(hb, hb0)
    union = MO.unpack(np.bitwise_or.reduce(ub0, axis=1))[:, :b["g"] ** 3]
    assert np.array_equal(carve, union) and carve.any()


@pytest.mark.parametrize("case", CC.CASES)
def test_case_is_not_degenerate(case):
    b = built(case)
    classes = CC.ray_classes(b, b["c2w"])
    print(case, classes)
    for name in CC.CLASSES:
        assert classes[name] > 0, (case, name, classes)
    args = _oracle_args(b)
    gain, ub, hb, carve = CO.measured(b["tri"].numpy(), b["c2w"], b["depth"].numpy(), *args, b["sense"])
    ub0, hb0 = MO.masks(b["tri"].numpy(), b["c2w"], *args)
    assert carve.any() and (gain[..., 0] > 0).any() and (gain[..., 2] > 0).any()
    assert not np.array_equal(ub, ub0) and not np.array_equal(hb, hb0)
    assert not np.array_equal(carve, MO.unpack(np.bitwise_or.reduce(ub0, axis=1))[:, :b["g"] ** 3])
    assert not (carve & (b["tri"].numpy() != 0)).any()  # only unknown voxels
    assert np.array_equal(MO.unpack(np.bitwise_or.reduce(ub, axis=1))[:, :b["g"] ** 3], carve)
    assert not (hb & ~ub).any()


def test_struct_fields_follow_the_header():
    import os
    import re
    from gennbv_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gennbv_hip.h")).read()
    body = re.search(r"typedef struct GnbvViewGain \{(.*?)\} GnbvViewGain;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f[0] for f in _lib.GnbvViewGain._fields_]
    names = []  # "const float *a, *b" -> a, b
    for decl in body.split(";"):
        parts = decl.strip().split(",")
        if parts[0]:
            names.append(re.sub(r"[\s\*]", "", parts[0].rsplit(" ", 1)[-1]))
            names += [re.sub(r"[\s\*]", "", p) for p in parts[1:]]
    assert names == fields
    assert fields[-6:] == ["depth_raw", "depth_env_stride", "depth_cand_stride", "depth_sense_dist", "carve_i8", "carve_row_stride"]
    assert _lib.load().gnbv_abi_version() == 5


TRI = 0x100000  # the made-up address of tri_i8


def _args(**kw):
    """A GnbvViewGain in depth mode that every entry point accepts, on made-up non-NULL pointers (a launch would follow: the calls
    below are all refused before one).  That the base values ARE accepted cannot be shown without a launch:
    tests/test_carve_gpu.py test_the_refusal_tests_base_arguments_are_accepted makes the same struct on real buffers, where all
    four entry points return 0, so a refusal here is the changed field's."""
    from gennbv_amd import _lib
    a = _lib.GnbvViewGain()
    a.n, a.k, a.g, a.h, a.w, a.stride, a.range, a.chunk, a.ablate = 2, 3, 20, 60, 80, 4, 50.0, 0, 0
    a.poses = a.range_gt = a.voxel_size = a.inv_intri = a.gain = 0x1000
    a.tri_i8, a.tri_row_stride = TRI, 20 ** 3
    a.depth_raw, a.depth_env_stride, a.depth_cand_stride, a.depth_sense_dist = 0x800000, 3 * 4800, 4800, -50.0
    a.carve_i8, a.carve_row_stride = 0x200000, 20 ** 3
    for f, v in kw.items():
        setattr(a, f, v)
    return a


REFUSED = [
    dict(depth_env_stride=4799), dict(depth_env_stride=0), dict(depth_cand_stride=4799), dict(depth_cand_stride=0),
    dict(depth_cand_stride=-4800), dict(depth_sense_dist=0.0), dict(depth_sense_dist=1.0), dict(depth_sense_dist=float("nan")),
    dict(depth_sense_dist=float("-inf")), dict(depth_raw=None), dict(ablate=1), dict(ablate=2), dict(carve_row_stride=7999),
    dict(carve_row_stride=0),
    # overlaps of the row ranges of carve_i8 and tri_i8 that are not the whole alias: tri rows are [TRI, TRI + 16000)
    dict(carve_i8=TRI + 1), dict(carve_i8=TRI + 15999), dict(carve_i8=TRI - 15999), dict(carve_i8=TRI + 8000),
    dict(carve_i8=TRI, carve_row_stride=8016),
]


def _entry_points():
    from gennbv_amd import _lib
    lib = _lib.load()
    ws = int(lib.gnbv_view_gain_slab_workspace_bytes(2, 3, 20, 60, 80, 4))
    assert ws > 0
    return {
        "gnbv_view_gain": lambda a: lib.gnbv_view_gain(C.byref(a), None),
        "gnbv_view_gain_masks": lambda a: lib.gnbv_view_gain_masks(C.byref(a), 252, 0x400000, 0x500000, None),
        "gnbv_view_gain_slab": lambda a: lib.gnbv_view_gain_slab(C.byref(a), 0, 0x10000000, ws, None),
        "gnbv_view_gain_slab_masks": lambda a: lib.gnbv_view_gain_slab_masks(C.byref(a), 0, 0x10000000, ws, 252, 0x400000, 0x500000, None),
    }


@pytest.mark.parametrize("name", ["gnbv_view_gain", "gnbv_view_gain_masks", "gnbv_view_gain_slab", "gnbv_view_gain_slab_masks"])
def test_refusals_before_any_launch(name):
    call = _entry_points()[name]
    for kw in REFUSED:
        assert call(_args(**kw)) == INVALID, (name, kw)
    # carve_i8 == tri_i8 with k > 1: one workgroup no longer owns the env in the one-launch kernels (the slab entry points
    # accept it; that is shown where a launch can follow, on the GPU)
    if "slab" not in name:
        assert call(_args(carve_i8=TRI)) == INVALID
    # carve_i8 without depth_raw, whatever else is set
    assert call(_args(depth_raw=None, depth_env_stride=0, depth_cand_stride=0, depth_sense_dist=0.0)) == INVALID


def test_carved_map_refuses_the_cpu():
    from gennbv_amd import _lib
    from gennbv_amd.ops.carve import CarvedMap
    sc = S.make_scenes(2, 16, seed=1)
    with pytest.raises(_lib.GennbvHipError, match="GPU only"):
        CarvedMap(2, CC.cfg_of(16), sc.range_gt, sc.voxel_size, device="cpu")


def test_merge_rule():
    from gennbv_amd.ops.carve import merge_observation
    rs = np.random.RandomState(3)
    n, g3 = 4, 5 ** 3
    m0 = rs.choice(np.array([-1, 0, 1], np.int8), size=(n, g3))
    tri = rs.choice(np.array([-1, 0, 0, 1], np.int8), size=(n, g3))
    reset = np.array([0, 1, 0, 1], np.uint8)
    want = CO.merge(m0, tri, reset)
    # by hand: a reset env is its fresh grid; elsewhere the observation wins where it has a class, the map survives where not
    assert np.array_equal(want[1], tri[1]) and np.array_equal(want[3], tri[3])
    for e in (0, 2):
        assert np.array_equal(want[e][tri[e] != 0], tri[e][tri[e] != 0]) and np.array_equal(want[e][tri[e] == 0], m0[e][tri[e] == 0])
    assert (want[0] != tri[0]).any() and (want[0] != m0[0]).any()
    for t in (torch.from_numpy(tri), torch.from_numpy(tri).float() * 0.5, torch.from_numpy(tri).view(n, 5, 5, 5),
              torch.from_numpy(tri * np.int8(7))):
        got = merge_observation(torch.from_numpy(m0.copy()), t, torch.from_numpy(reset))
        assert np.array_equal(got.numpy(), want)
    wide = torch.zeros(n, g3 + 9)
    wide[:, 4:4 + g3] = torch.from_numpy(tri).float()  # the grid slice of a flat observation: strided rows
    assert np.array_equal(merge_observation(torch.from_numpy(m0.copy()), wide[:, 4:4 + g3], torch.from_numpy(reset).bool()).numpy(), want)
    assert np.array_equal(merge_observation(torch.from_numpy(m0.copy()), torch.from_numpy(tri)).numpy(), CO.merge(m0, tri))
    assert np.array_equal(CO.merge(m0, tri), np.where(tri != 0, tri, m0))

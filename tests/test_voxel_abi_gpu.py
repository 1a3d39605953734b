"""GPU: the occupancy-grid update of csrc/voxel.hip at its C ABI -- gnbv_update_occ_grid, gnbv_update_occ_grid_packed and
gnbv_update_occ_grid_coded through ctypes on buffers the test places itself -- against the CPU oracle, bit for bit, after every call
of a short sequence with a reset: probability grid (the coded one decoded on the device and on the host), scanned set, tri-class
rows (fp32 and int8, the bytes between strided rows included), coverage count, hit and path masks.

Frames come from tests/voxel_abi_util.py, not from synthetic.make_scenes: random depth per pixel, and a range, offset and
anisotropy of its own for every env.  Every launch-regime case first asserts, from n and the oracle's masks, that it reaches the
branch its id names (tests/test_voxel_abi_regimes_cpu.py runs the same assertions without a GPU).  The layout cases are all legal
inputs: offsets keep every array naturally aligned for its element type."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import voxel_abi_util as U
from tests.voxel_abi_util import CLEAN, DEV, INVALID, f32

pytestmark = pytest.mark.gpu


def _run(kind, case, ref, full_ws=True, flags=None, d=None, **layout):
    """The whole sequence of a case through one entry point; every call against the oracle.  Returns the outputs per call."""
    call = U.VoxelCall(kind, case, full_ws=full_ws, **layout)
    outs = []
    for s in range(len(case.frames)):
        fl = 0 if (flags is None or kind != "coded") else flags[s]
        assert call.step(s, fl) == 0, s
        cleaned = bool(fl & CLEAN) and (d is None or d.path != "round1")  # (the round-1 kernels zero what they need themselves)
        o = call.outputs(masks=not cleaned)
        U.compare(call, o, ref[s], f"{kind} call {s}", masks=not cleaned)
        if cleaned:  # the contract of GNBV_VOXEL_WS_CLEAN: masks and ray counts are zero again
            head = 2 * case.n * U.mask_words(case.g) * 4 + ((case.n + 63) & ~63) * 4
            assert not call.ws.read()[0, :head].any(), f"call {s}: the workspace is not left clean"
        if kind == "coded" and o.overflow is not None:
            assert o.overflow == 0
        outs.append(o)
    return outs


# ---------------------------------------------------------------------------
# launch regimes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(U.LAUNCH_CASES))
def test_launch_regime(cid, monkeypatch):
    """One case per launch regime of launch_masks and the mask kernels (the id names it; tests/voxel_abi_util.py: LAUNCH_CASES and
    check_regime).  list-*: k_hit_list + k_ray_list on the full workspace.  round1-*: k_hit_mask + k_raycast through the mask-only
    workspace, and the same inputs on the full workspace, with equal results.  large-*: k_hit_atomic + k_ray_slab forced at G = 16.
    The coded cases make their first two calls with GNBV_VOXEL_WS_CLEAN (the workspace must come out zero, and the following calls
    right) and the rest without (masks compared); at n >= 512 the hit masks are plain stores, never memset.
    Oracle figures (hit voxels of the loaded env, two calls): round1-g32-n1024-two-queue-rounds 5281 / 5373 > kQueueCap = 4096;
    list-n2-several-items-per-workgroup: 6 ... 15 items on an XCD with 5 workgroups, mean ray count 3450 > 5 * 384."""
    kind = U.LAUNCH_CASES[cid][0]
    U.check_regime(cid)
    case, ref = U.launch_case(cid)
    flags = [CLEAN, CLEAN] + [0] * (len(case.frames) - 2) if len(case.frames) > 2 else [CLEAN, 0]
    runs = []
    for full_ws, large in U.workspaces_of(cid):
        if large is not None:
            monkeypatch.setenv("GENNBV_VOXEL_LARGE", large)
        d = U.dispatch(case.n, case.g, case.h, case.w, full_ws, large)
        runs.append(_run(kind, case, ref, full_ws=full_ws, flags=flags, d=d))
    for s, (a, b) in enumerate(zip(runs[0], runs[-1])):  # mask-only against full workspace
        U.same_outputs(a, b, f"call {s}: mask-only and full workspace")


@pytest.mark.parametrize("kind,full_ws,large", [("f32", True, None), ("packed", False, None), ("coded", True, None), ("coded", True, "1")])
def test_every_env_uses_its_own_frame(kind, full_ws, large, monkeypatch):
    """Fails if a kernel took range_gt / voxel_size (or anything else per env) from another env.  Construction: envs 0 and 1 get the
    SAME depth and seg images, camera matrix and pose in every call; only their range_gt (shifted by (0.37, -0.21, 0.55), the upper
    corner by (1.9, 0.8, -0.7)) and with it their voxel_size differ.  The oracle's hit and path masks of the two envs differ -- asserted
    -- and the kernels must match the oracle for both; envs 2 .. 9 are unrelated (nine envs: more than one XCD group), and env 1's
    ground truth differs from env 0's, so the scanned sets do too."""
    if large is not None:
        monkeypatch.setenv("GENNBV_VOXEL_LARGE", large)
    case = U.make_case(n=10, g=16, h=24, w=32, seed=77, twins=True, binary=kind != "f32", outside_share=0.0)
    ref = U.run_oracle(case)
    U.assert_masks_not_vacuous(ref)
    for f in case.frames:
        assert f.depth[0].tobytes() == f.depth[1].tobytes() and f.c2w[0].tobytes() == f.c2w[1].tobytes() and f.poses[0].tobytes() == f.poses[1].tobytes()
    assert case.scene.range_gt[0].tobytes() != case.scene.range_gt[1].tobytes()
    for o in ref:
        assert o.hit[0].sum() > 20 and o.hit[1].sum() > 20
        assert (o.hit[0] != o.hit[1]).sum() > 20 and (o.path[0] != o.path[1]).sum() > 20 and (o.scan[0] != o.scan[1]).any()
    _run(kind, case, ref, full_ws=full_ws)


# ---------------------------------------------------------------------------
# layout regimes: pointer alignment and row strides pick the vec4 / vec16 / scalar grid-update kernels
# ---------------------------------------------------------------------------
@U.cached
def _layout_case(kind, g):
    case = U.make_case(n=3, g=g, h=8, w=12, seed=100 + g, binary=kind != "f32")
    ref = U.run_oracle(case)
    U.assert_masks_not_vacuous(ref)
    return case, ref


@U.cached
def _aligned_outputs(kind, g, use_tri, use_tri8):
    case, ref = _layout_case(kind, g)
    return _run(kind, case, ref, use_tri=use_tri, use_tri8=use_tri8)


def _vec4_of(call):
    ptrs = [call.tri.ptr, call.prob.ptr] + ([call.scan.ptr, call.gt.ptr] if call.kind == "f32" else [])
    return U.grid_vec4(call.g3, call.tri.stride, *ptrs)


F32_LAYOUTS = {"tri_row_stride%4": dict(tri_stride=3), "tri_out+4": dict(tri_off=4), "prob_grid+4": dict(prob_off=4),
               "scanned_gt_grid+4": dict(scan_off=4), "grid_gt+4": dict(gt_off=4)}


@pytest.mark.parametrize("g", [16, 10])
@pytest.mark.parametrize("kind,name", [("f32", k) for k in F32_LAYOUTS] + [("packed", k) for k in list(F32_LAYOUTS)[:3]])
def test_unaligned_fp32_layouts_take_the_scalar_grid_update(kind, name, g):
    """fp32 and packed entry points: a tri row stride that is no multiple of 4, or ONE of the grid pointers 4 bytes off a 16-byte
    boundary, drops the call to the scalar k_grid_update / k_grid_update_packed; every output equals the oracle and the aligned
    (float4) run of the same inputs.  G = 16: G^3 % 16 == 0; G = 10: G^3 % 16 == 8."""
    case, ref = _layout_case(kind, g)
    layout = dict(F32_LAYOUTS[name])
    if "tri_stride" in layout:
        layout["tri_stride"] = g ** 3 + 3
    probe = U.VoxelCall(kind, case, **layout)
    assert not _vec4_of(probe) and _vec4_of(U.VoxelCall(kind, case)), "the layout must change the dispatch"
    outs = _run(kind, case, ref, **layout)
    for s, (a, b) in enumerate(zip(outs, _aligned_outputs(kind, g, True, False))):
        U.same_outputs(a, b, f"call {s}: {name} against the aligned layout")


def _other_tri_lut():
    """Not of the run shape gnbv_prob_code_tables gives (+1 / 0 / -1 runs per base): the classes alternate with the code, so the codes
    of a three-call sequence (0, 1, 2 path steps; 128 after a hit) already use all three."""
    return ((np.arange(256) * 7 + 1) % 3 - 1).astype(f32)


# name -> (layout, voxels per lane at G = 16, at G = 10)
CODED_LAYOUTS = {
    "int8-only-aligned": (dict(use_tri=False), 16, 4),
    "prob_code+4": (dict(use_tri=False, prob_off=4), 4, 4),
    "tri_i8+4": (dict(use_tri=False, tri8_off=4), 4, 4),
    "tri_i8_row_stride%16==4": (dict(use_tri=False, tri8_stride=4), 4, 4),
    "prob_code+1": (dict(use_tri=False, prob_off=1), 1, 1),
    "tri_i8+1": (dict(use_tri=False, tri8_off=1), 1, 1),
    "tri_i8_row_stride+1": (dict(use_tri=False, tri8_stride=1), 1, 1),
    "tri_out-alone": (dict(use_tri=True, use_tri8=False), 4, 4),
    "tri_out-and-tri_i8": (dict(use_tri=True, use_tri8=True), 4, 4),
    "tri_out+4-and-tri_i8": (dict(use_tri=True, use_tri8=True, tri_off=4), 1, 1),
    "overflow-null": (dict(use_tri=False, use_overflow=False), 16, 4),
    "replacement-tri_lut-misaligned": (dict(use_tri=True, use_tri8=True, prob_off=1, tri_lut=_other_tri_lut()), 1, 1),
}


@pytest.mark.parametrize("g", [16, 10])
@pytest.mark.parametrize("name", list(CODED_LAYOUTS))
def test_coded_layouts_pick_16_4_or_1_voxels_per_lane(name, g):
    """gnbv_update_occ_grid_coded: tri_out NULL and everything 16-byte aligned -> 16 voxels per lane (G^3 % 16 == 0), a code or int8
    pointer / int8 row stride that is a multiple of 4 only -> 4, an odd one -> 1; tri_out alone, both outputs, overflow NULL, and a
    replacement tri_lut (classes alternating with the code: the table reads, not the byte-parallel classes) on a misaligned layout.  Every output
    equals the oracle and the aligned run of the same inputs; with the replacement table the tri rows equal tri_lut[code]."""
    layout, vpl16, vpl10 = CODED_LAYOUTS[name]
    layout = dict(layout)
    if "tri8_stride" in layout:
        layout["tri8_stride"] = g ** 3 + 16 + layout["tri8_stride"]
    case, ref = _layout_case("coded", g)
    probe = U.VoxelCall("coded", case, **layout)
    vpl = U.coded_vpl(probe.g3, probe.prob.ptr, probe.tri.ptr if probe.tri else 0, probe.tri.stride if probe.tri else 0,
                      probe.tri8.ptr if probe.tri8 else 0, probe.tri8.stride if probe.tri8 else 0)
    assert vpl == (vpl16 if g == 16 else vpl10)
    outs = _run("coded", case, ref, **layout)
    if "tri_lut" not in layout:
        for s, (a, b) in enumerate(zip(outs, _aligned_outputs("coded", g, True, True))):
            U.same_outputs(a, b, f"call {s}: {name} against the aligned layout")
    else:
        assert len(np.unique(outs[-1].tri)) == 3


@pytest.mark.parametrize("kind", ["f32", "packed", "coded"])
@pytest.mark.parametrize("stride", [3, 6, 7])
def test_pose_row_stride(kind, stride):
    """poses_xyz rows 3, 6 (the env's pose buffer) or 7 floats apart; the floats between the rows hold a sentinel."""
    case, ref = _layout_case(kind, 16)
    outs = _run(kind, case, ref, pose_stride=stride)
    for s, (a, b) in enumerate(zip(outs, _aligned_outputs(kind, 16, kind != "coded", kind == "coded"))):
        U.same_outputs(a, b, f"call {s}: pose stride {stride}")


# ---------------------------------------------------------------------------
# refusals: non-zero return, nothing launched
# ---------------------------------------------------------------------------
def _refusals(kind, a, call):
    g3, lib = call.g3, call.lib
    required = ["depth_raw", "seg_raw", "c2w", "inv_intri", "poses_xyz", "range_gt", "voxel_size", "coverage_count", "workspace"]
    required += {"f32": ["grid_gt", "prob_grid", "scanned_gt_grid", "tri_out"], "packed": ["gt_bits", "prob_grid", "scanned_bits", "tri_out"],
                 "coded": ["gt_bits", "prob_code", "scanned_bits", "tri_lut"]}[kind]
    rows = [(f"{k} NULL", {k: None}) for k in required]
    rows += [("g = 1", dict(g=1)), ("g = 1025", dict(g=1025)), ("poses_row_stride = 2", dict(poses_row_stride=2)),
             ("workspace one byte short", dict(workspace_bytes=int(lib.gnbv_voxel_workspace_bytes(a["n"], a["g"])) - 1)),
             ("workspace + 64", dict(workspace=a["workspace"] + 64)),
             ("depth_raw + 4 with w % 4 == 0", dict(depth_raw=a["depth_raw"] + 4)), ("seg_raw + 4 with w % 4 == 0", dict(seg_raw=a["seg_raw"] + 4)),
             ("depth_raw + 8 with w % 4 == 0", dict(depth_raw=a["depth_raw"] + 8))]
    if kind == "coded":
        rows += [("tri_out and tri_i8 NULL", dict(tri_out=None, tri_i8=None)), ("tri_i8_row_stride = g3 - 1", dict(tri_i8_row_stride=g3 - 1)),
                 ("tri_row_stride = g3 - 1", dict(tri_row_stride=g3 - 1))]
    else:
        rows += [("tri_row_stride = g3 - 1", dict(tri_row_stride=g3 - 1))]
    return rows


@pytest.mark.parametrize("kind", ["f32", "packed", "coded"])
def test_refused_calls_return_an_error_and_launch_nothing(kind):
    """One table per entry point: NULL for each required pointer, g in {1, 1025}, a pose stride of 2, tri rows shorter than G^3, a
    workspace one byte short or off its 256-byte alignment, depth_raw / seg_raw off the 16-byte alignment the 16-byte pixel requests
    need (w % 4 == 0); coded: no tri output at all, int8 rows shorter than G^3.  Every call returns hipErrorInvalidValue and leaves
    every output buffer and the workspace byte for byte as they were; the unmodified arguments then make a valid call."""
    case, ref = _layout_case(kind, 16)
    assert case.w % 4 == 0
    call = U.VoxelCall(kind, case, use_tri=True, use_tri8=(kind == "coded"))
    call.load(case.frames[0], None)
    base = call.args(None, CLEAN if kind == "coded" else 0)
    before = call.snapshot()
    for what, change in _refusals(kind, base, call):
        a = dict(base)
        a.update(change)
        assert call.call(a) == INVALID, what
        assert call.snapshot() == before, f"{what}: the refused call wrote something"
    assert call.call(base) == 0
    U.compare(call, call.outputs(masks=kind != "coded"), ref[0], "the valid call", masks=kind != "coded")


def test_refused_coded_call_leaves_a_clean_workspace_clean():
    """gnbv_update_occ_grid_coded checked tri_i8_row_stride only after the mask launches: a refused GNBV_VOXEL_WS_CLEAN call with
    frame A left A's hit / path bits and ray counts in a workspace whose contract is "the call leaves them zero", and the next CLEAN
    call ORed them into frame B's masks.  Now: refused call with frame A on a fresh zero workspace, then a valid CLEAN call with
    frame B -- every output equals the oracle's for frame B alone."""
    case, _ = _layout_case("coded", 16)
    call = U.VoxelCall("coded", case, use_tri=True, use_tri8=True)
    call.load(case.frames[0], None)
    a = call.args(None, CLEAN)
    a["tri_i8_row_stride"] = call.g3 - 1
    assert call.call(a) == INVALID
    assert not call.ws.read().any(), "the refused call touched the workspace"
    only_b = U.SimpleNamespace(**vars(case))
    only_b.frames, only_b.resets = [case.frames[1]], [None]
    ref_b = U.run_oracle(only_b)
    U.assert_masks_not_vacuous(ref_b)
    call.load(case.frames[1], None)
    assert call.call(call.args(None, CLEAN)) == 0
    U.compare(call, call.outputs(masks=False), ref_b[0], "frame B after the refused call", masks=False)
    assert not call.ws.read()[0, :2 * case.n * U.mask_words(case.g) * 4 + 256].any()


# ---------------------------------------------------------------------------
# gnbv_rgb_to_gray, gnbv_grid_tri_cls
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,oh,ow,pad", [(3, 240, 320, 64, 64, 0), (2, 37, 53, 64, 64, 5), (4, 5, 7, 3, 2, 3), (129, 5, 7, 64, 64, 0)])
def test_rgb_to_gray_bit_exact_vs_oracle(n, h, w, oh, ow, pad):
    """Nearest resize + grayscale against oracle.rgb_to_gray64: down- and up-scaling with non-integer ratios, rows pad floats longer
    than oh*ow (the padding keeps its sentinel), channel values 0 and 255, and 129 * 64 * 64 > 2048 * 256 outputs (threads stride)."""
    L, lib = U.libs()
    assert n != 129 or n * oh * ow > U.GRID_STRIDE_THREADS
    rs = np.random.RandomState(n * h + w)
    rgba = rs.randint(0, 256, (n, h, w, 4), dtype=np.uint8)
    rgba[..., :3][rs.rand(n, h, w) < 0.1] = 0
    rgba[..., :3][rs.rand(n, h, w) < 0.1] = 255
    rgba[0, 0, 0, :3] = (255, 0, 255)
    assert (rgba[..., :3] == 0).any() and (rgba[..., :3] == 255).any()
    src = torch.from_numpy(rgba).to(DEV)
    gray = U.Rows(n, oh * ow, f32, stride=oh * ow + pad)
    L.check(lib.gnbv_rgb_to_gray(src.data_ptr(), n, h, w, oh, ow, gray.ptr, oh * ow + pad, None), "gnbv_rgb_to_gray")
    torch.cuda.synchronize()
    want = orc.rgb_to_gray64(rgba, oh, ow).reshape(n, -1)
    assert len(np.unique(want)) > 10
    assert gray.read().tobytes() == want.tobytes()
    assert gray.padding_intact()


def test_rgb_to_gray_refusals():
    _, lib = U.libs()
    src = torch.zeros(2 * 5 * 7 * 4, dtype=torch.uint8, device=DEV)
    gray = U.Rows(2, 6, f32)
    before = gray.snapshot()
    assert lib.gnbv_rgb_to_gray(src.data_ptr(), 2, 5, 7, 3, 2, gray.ptr, 5, None) == INVALID  # rows shorter than oh*ow
    assert lib.gnbv_rgb_to_gray(None, 2, 5, 7, 3, 2, gray.ptr, 6, None) == INVALID
    assert lib.gnbv_rgb_to_gray(src.data_ptr(), 2, 5, 7, 3, 2, None, 6, None) == INVALID
    torch.cuda.synchronize()
    assert gray.snapshot() == before


@pytest.mark.parametrize("count", [0, 1, 2048 * 256 + 37])
@pytest.mark.parametrize("t_occ,t_free", [(0.5, 0.0), (0.75, -0.25)])
def test_grid_tri_cls_vs_numpy(count, t_occ, t_free):
    """(v > t_occ) - (v < t_free) in fp32: values exactly on both thresholds and one ulp around them, +-0, NaN, +-inf; no element,
    one, and more than 2048 * 256 (threads stride); default and other thresholds."""
    L, lib = U.libs()
    to, tf = f32(t_occ), f32(t_free)
    special = np.asarray([to, tf, np.nextafter(to, f32(2)), np.nextafter(to, f32(-2)), np.nextafter(tf, f32(2)), np.nextafter(tf, f32(-2)),
                          0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -0.05], f32)
    rs = np.random.RandomState(count % 1000)
    v = rs.uniform(-1.0, 1.5, max(count, 1)).astype(f32)
    if count > 1:
        v[rs.choice(count, 20 * special.size, replace=False)] = np.tile(special, 20)
        v[:special.size], v[-special.size:] = special, special
    elif count == 1:
        v[0] = to
    src = torch.from_numpy(v).to(DEV)
    out = U.Rows(1, max(count, 1), f32, init=np.full((1, max(count, 1)), 9.0, f32))
    L.check(lib.gnbv_grid_tri_cls(src.data_ptr(), count, C.c_float(to), C.c_float(tf), out.ptr, None), "gnbv_grid_tri_cls")
    torch.cuda.synchronize()
    want = np.full(max(count, 1), 9.0, f32)
    with np.errstate(invalid="ignore"):
        want[:count] = ((v > to).astype(f32) - (v < tf).astype(f32))[:count]
    assert out.read().reshape(-1).tobytes() == want.tobytes()
    assert out.padding_intact()
    if count > 1:
        assert set(np.unique(want).tolist()) == {-1.0, 0.0, 1.0}

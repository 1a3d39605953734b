"""GPU: every C entry point and every Python operator runs on the CALLER's stream (the harness and the
protocol are tests/stream_order_util.py).

One case = one or more entry points driven at their smallest interesting shape, through the project's own Python wrapper where one
exists (so the wrapper's stream handle and the library's launches are judged by the same run) and through ctypes where none does.
For each case the module fixture makes the two default-stream reference runs (real inputs A, decoy inputs D) with the recording
proxy installed; the tests then
  * run the delayed-input protocol on a side stream (`test_c_layer_keeps_to_the_stream`): the stream still held when the call
    returns, the outputs bit-equal to the default-stream run;
  * check the handles the proxy recorded (`test_python_layer_passes_the_callers_stream`): the side stream's on the side stream,
    the default stream's before and AFTERWARDS (a handle cached at construction or at first use fails one of the two).
CASES is also the table the census (tests/test_stream_order_cpu.py) holds against include/gennbv_hip.h; importing this module does
not touch the GPU.
"""
import ctypes as C
import math

import pytest
import torch

from tests import stream_order_util as U

pytestmark = pytest.mark.gpu
DEV = U.DEV

CASES = {}  # name -> (entry points the case must be seen to call, maker)
FORKS = {"encoder_train", "rollout_plan"}  # cases whose wrapper forks and joins side streams of its own on purpose


def case(name, *entries):
    def reg(fn):
        assert name not in CASES
        CASES[name] = (tuple(entries), fn)
        return fn
    return reg


def covered_entry_points():
    return {e for entries, _ in CASES.values() for e in entries}


# ------------------------------------------------------------------------------------------------------------------------ helpers
def _cfg(h, w, g):
    from gennbv_amd.env.config import TaskConfig
    return TaskConfig(camera_width=w, camera_height=h, grid_size=g)


def _dev(t):
    return t.to(DEV).contiguous()


def _bufs(A):
    """input buffers shaped like the staged set"""
    return {k: torch.empty_like(v) for k, v in A.items()}


def _on(fn):
    """call(stream) of a wrapper that takes the current stream"""
    def call(stream):
        with torch.cuda.stream(stream):
            out = fn()
        return out if isinstance(out, dict) else None
    return call


def _rand(seed, *shape, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return _dev(lo + (hi - lo) * torch.rand(*shape, generator=g))


def _randint(seed, lo, hi, *shape, dtype=torch.int32):
    g = torch.Generator().manual_seed(seed)
    return _dev(torch.randint(lo, hi, shape, generator=g).to(dtype))


def _frames(n, g, h, w):
    """(cfg, scene, two rendered frames as dicts of device tensors): real and decoy camera input of the same scene"""
    from gennbv_amd.env import synthetic as S
    cfg = _cfg(h, w, g)
    scene = S.make_scenes(n, g, seed=2)
    out = []
    for f in S.make_frames(scene, cfg, 2, seed=3, with_rgba=True):
        out.append({"depth": _dev(f.depth_raw.float()), "seg": _dev(f.seg_raw.float()), "rgba": _dev(f.rgba),
                    "c2w": _dev(S.camera_to_world(f.poses).float()), "poses": _dev(f.poses.float())})
    return cfg, scene, out


def _mesh(n, g, seed=2):
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.mesh_scene import MeshScene
    scene = S.make_scenes(n, g, seed=seed)
    return scene, MeshScene.from_boxes(scene, device=DEV)


def _scene_poses(seed, n, k):
    """[N,K,6] poses in and around the boxes of make_scenes (xy in +-5 m, z 0..7 m): some collide, some do not"""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(n, k, 6)
    p[..., 0:2] = (torch.rand(n, k, 2, generator=g) - 0.5) * 10.0
    p[..., 2] = torch.rand(n, k, generator=g) * 7.0
    p[..., 4] = (torch.rand(n, k, generator=g) - 0.5) * math.pi
    p[..., 5] = torch.rand(n, k, generator=g) * 2 * math.pi
    return _dev(p)


def _look_poses(seed, n, k, cfg):
    from gennbv_amd.eval.baselines import LatticeCandidates
    lc = LatticeCandidates(cfg, k, seed, look_at_scene=True)
    return _dev(lc.poses(lc.sample(n)))


def _tri(seed, n, g, occ=0.05, free=0.4):
    """tri-class rows int8 [N, G^3]: a share `occ` occupied (1), `free` of the rest free (-1), the others unknown (0)"""
    gen = torch.Generator().manual_seed(seed)
    r = torch.rand(n, g ** 3, generator=gen)
    return _dev(torch.where(r < occ, 1, torch.where(r < occ + free * (1 - occ), -1, 0)).to(torch.int8))


# ----------------------------------------------------------------------------------------------- A1-A7: the function-granular ops
@case("post_process_depth", "gnbv_post_process_depth")
def _c_post_process_depth():
    from gennbv_amd import utils
    A = {"d": _rand(1, 2, 30, 37, lo=-60.0, hi=0.0), "s": _rand(2, 2, 30, 37, hi=255.0)}
    D = {"d": _rand(3, 2, 30, 37, lo=-60.0, hi=0.0), "s": _rand(4, 2, 30, 37, hi=255.0)}
    I = _bufs(A)

    def run():
        do, so = utils.post_process_depth(I["d"], I["s"])
        return {"depth": do, "seg": so}
    return U.Live(I, A, D, {}, _on(run), ["depth", "seg"])


@case("rgb_to_gray", "gnbv_rgb_to_gray")
def _c_rgb_to_gray():
    from gennbv_amd import utils
    A = {"rgba": _randint(1, 0, 256, 2, 30, 37, 4, dtype=torch.uint8)}
    D = {"rgba": _randint(2, 0, 256, 2, 30, 37, 4, dtype=torch.uint8)}
    I = _bufs(A)
    O = {"gray": torch.empty(2, 1, 8, 8, device=DEV)}
    return U.Live(I, A, D, O, _on(lambda: utils.rgb_to_gray(I["rgba"], 8, 8, out=O["gray"], out_row_stride=64)), ["gray"])


@case("back_projection", "gnbv_back_projection")
def _c_back_projection():
    from gennbv_amd import _lib
    from gennbv_amd.env import synthetic as S
    n, h, w = 2, 30, 37
    _, _, fr = _frames(n, 16, h, w)
    A, D = ({"d": f["depth"].clamp_min(-50.0), "s": f["seg"], "c2w": f["c2w"]} for f in fr)
    I = _bufs(A)
    O = {"world": torch.empty(n, h * w, 3, device=DEV), "fg": torch.empty(n, h * w, dtype=torch.uint8, device=DEV)}
    ki = S.inverse_intrinsics(h, w).contiguous()

    def call(stream):  # (utils.back_projection_fg compacts the points with a boolean index: a host read-back by design)
        _lib.check(_lib.load().gnbv_back_projection(I["d"].data_ptr(), I["s"].data_ptr(), I["c2w"].data_ptr(), ki.data_ptr(), n, h, w,
                                                    O["world"].data_ptr(), O["fg"].data_ptr(), stream.cuda_stream), "gnbv_back_projection")
    return U.Live(I, A, D, O, call, ["world", "fg"])


@case("points_to_idx", "gnbv_points_to_idx")
def _c_points_to_idx():
    from gennbv_amd import utils
    scene, _ = _mesh(2, 16)
    rg, vs = _dev(scene.range_gt), _dev(scene.voxel_size)
    A = {"world": _rand(1, 2, 1111, 3, lo=-6.0, hi=9.0), "fg": _randint(2, 0, 2, 2, 1111, dtype=torch.uint8)}
    D = {"world": _rand(3, 2, 1111, 3, lo=-6.0, hi=9.0), "fg": _randint(4, 0, 2, 2, 1111, dtype=torch.uint8)}
    I = _bufs(A)
    return U.Live(I, A, D, {}, _on(lambda: {"idx": utils.points_to_idx(I["world"], I["fg"], rg, vs, 16)}), ["idx"])


@case("pose_to_idx", "gnbv_pose_to_idx")
def _c_pose_to_idx():
    from gennbv_amd import utils
    scene, _ = _mesh(3, 16)
    rg, vs = _dev(scene.range_gt), _dev(scene.voxel_size)
    A, D = {"p": _rand(1, 3, 3, lo=-6.0, hi=9.0)}, {"p": _rand(2, 3, 3, lo=-6.0, hi=9.0)}
    I = _bufs(A)
    return U.Live(I, A, D, {}, _on(lambda: {"idx": utils.pose_coord_to_idx_3D(I["p"], rg, vs, 16)}), ["idx"])


@case("bresenham3d", "gnbv_bresenham3d")
def _c_bresenham3d():
    from gennbv_amd import utils
    g = 16
    A = {"s": _randint(1, 0, g, 1, 3), "t": _randint(2, -3, g + 3, 70, 3)}
    D = {"s": _randint(3, 0, g, 1, 3), "t": _randint(4, -3, g + 3, 70, 3)}
    I = _bufs(A)

    def run():
        traj, lens = utils.bresenham3D_raw(I["s"], I["t"], g)
        return {"traj": traj, "lens": lens}
    return U.Live(I, A, D, {}, _on(run), ["traj", "lens"])


@case("grid_tri_cls", "gnbv_grid_tri_cls")
def _c_grid_tri_cls():
    from gennbv_amd import utils
    A, D = {"p": _rand(1, 2, 7, 7, 7, lo=-0.3, hi=1.0)}, {"p": _rand(2, 2, 7, 7, 7, lo=-0.3, hi=1.0)}
    I = _bufs(A)
    return U.Live(I, A, D, {}, _on(lambda: {"tri": utils.grid_occupancy_tri_cls(I["p"], return_tri_cls_only=True)}), ["tri"])


# -------------------------------------------------------------------------------------------------------- the fused voxel update
def _updater_case(kind):
    """OccupancyGridUpdater.update on a workspace that is NOT self-cleaning (the memsets run), then the views of its state:
    kind "f32" gnbv_update_occ_grid on a non-binary GT, "packed" the bitmask variant, "coded" the byte-coded one."""
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.state_encoding import OccupancyGridUpdater
    n, g, h, w = 3, 16, 30, 37  # w % 4 != 0: the per-pixel loop; 1 110 pixels: more than one workgroup of the hit pass
    cfg, scene, fr = _frames(n, g, h, w)
    gt = scene.grid_gt.clone()
    if kind == "f32":
        gt = gt * 0.5  # not binary: the updater keeps the fp32 scanned grid
    up = OccupancyGridUpdater(n, g, h, w, S.inverse_intrinsics(h, w), scene.range_gt, scene.voxel_size, gt, DEV,
                              max_steps_between_resets=100 if kind == "coded" else None)
    assert up.coded == (kind == "coded") and up.packed == (kind != "f32")
    up.self_clean = False
    torch.cuda.synchronize()
    keys = ("depth", "seg", "c2w", "poses")
    A, D = ({k: f[k] for k in keys} for f in fr)
    state = {"scanned_bits": up.scanned_bits} if up.packed else {"scanned_f32": up._scanned_f32}
    state.update({"prob_code": up.prob_code, "overflow": up.code_overflow} if up.coded else {"prob": up._prob_f32})
    for k, t in state.items():  # in/out state: the same (empty map) in both sets, reloaded before every call
        A[k] = D[k] = torch.zeros_like(t)
    I = _bufs({k: A[k] for k in keys})
    I.update(state)
    tri = torch.empty(n, g ** 3, device=DEV)
    O = {"tri": tri, "coverage": up.coverage_count, "workspace": up.workspace}
    tri8 = None
    if up.coded:
        tri8 = O["tri8"] = torch.empty(n, g ** 3, dtype=torch.int8, device=DEV)

    def run():
        up.update(I["depth"], I["seg"], I["c2w"], I["poses"], tri_out=tri, tri_row_stride=g ** 3, tri_i8_out=tri8)
        hit, path = up.masks()
        return {"hit": hit, "path": path, "scanned": up.scanned_gt_grid}
    # (overflow is not compared: it stays 0 in both sets, no counter saturates in one step)
    cmp = ["tri", "coverage", "hit", "path", "scanned"] + [k for k in state if k != "overflow"] + (["tri8"] if up.coded else [])
    return U.Live(I, A, D, O, _on(run), cmp)


@case("update_occ_grid", "gnbv_update_occ_grid", "gnbv_unpack_masks")
def _c_update_f32():
    return _updater_case("f32")


@case("update_occ_grid_packed", "gnbv_update_occ_grid_packed", "gnbv_unpack_masks", "gnbv_unpack_grid_bits")
def _c_update_packed():
    return _updater_case("packed")


@case("update_occ_grid_coded", "gnbv_update_occ_grid_coded", "gnbv_unpack_masks", "gnbv_unpack_grid_bits")
def _c_update_coded():
    return _updater_case("coded")


@case("pack_grid_bits", "gnbv_pack_grid_bits", "gnbv_unpack_grid_bits")
def _c_pack_grid_bits():
    from gennbv_amd import _lib
    n, g = 3, 7
    lib = _lib.load()
    words = lib.gnbv_grid_bit_words(g)
    A = {"grid": (_rand(1, n, g ** 3) < 0.3).float()}
    D = {"grid": (_rand(2, n, g ** 3) < 0.3).float()}
    D["grid"][1, 5] = 0.25  # the decoy is not binary: the flag differs too
    I = _bufs(A)
    O = {"bits": torch.empty(n, words, dtype=torch.int32, device=DEV), "flag": torch.empty(1, dtype=torch.int32, device=DEV),
         "back": torch.empty(n, g ** 3, device=DEV)}

    def call(stream):
        s = stream.cuda_stream
        _lib.check(lib.gnbv_pack_grid_bits(I["grid"].data_ptr(), n, g, O["bits"].data_ptr(), O["flag"].data_ptr(), s), "gnbv_pack_grid_bits")
        _lib.check(lib.gnbv_unpack_grid_bits(O["bits"].data_ptr(), n, g, O["back"].data_ptr(), s), "gnbv_unpack_grid_bits")
    return U.Live(I, A, D, O, call, ["bits", "flag", "back"])


@case("decode_prob_grid", "gnbv_decode_prob_grid")
def _c_decode_prob_grid():
    from gennbv_amd import _lib
    lib = _lib.load()
    pl = (C.c_float * 256)()
    lib.gnbv_prob_code_tables(pl, None)
    lut = torch.tensor(list(pl), device=DEV)
    A, D = {"code": _randint(1, 0, 256, 5000, dtype=torch.uint8)}, {"code": _randint(2, 0, 256, 5000, dtype=torch.uint8)}
    I = _bufs(A)
    O = {"prob": torch.empty(5000, device=DEV)}

    def call(stream):
        _lib.check(lib.gnbv_decode_prob_grid(I["code"].data_ptr(), 5000, lut.data_ptr(), O["prob"].data_ptr(), stream.cuda_stream),
                   "gnbv_decode_prob_grid")
    return U.Live(I, A, D, O, call, ["prob"])


# ------------------------------------------------------------------------------------------------------------ mesh-scene kernels
@case("render_depth", "gnbv_render_depth")
def _c_render_depth():
    from gennbv_amd.env.render_feed import RenderFeed
    n, g, h, w = 2, 16, 30, 37
    cfg = _cfg(h, w, g)
    _, mesh = _mesh(n, g)
    feed = RenderFeed(mesh, cfg)
    A, D = {"poses": _look_poses(1, n, 1, cfg)[:, 0].contiguous()}, {"poses": _look_poses(2, n, 1, cfg)[:, 0].contiguous()}
    I = _bufs(A)
    O = {"depth": feed.depth_raw, "seg": feed.seg_raw, "rgba": feed.rgba, "c2w": feed.c2w}
    return U.Live(I, A, D, O, _on(lambda: feed.render(I["poses"])), ["depth", "seg", "rgba", "c2w"])


@case("voxelize_surface", "gnbv_voxelize_surface")
def _c_voxelize_surface():
    n, g = 2, 16
    scene, mesh = _mesh(n, g)
    # the triangles are fixed; the voxel frame is the device input that differs
    A = {"range": _dev(scene.range_gt), "voxel": _dev(scene.voxel_size)}
    D = {"range": _dev(scene.range_gt + 0.37), "voxel": _dev(scene.voxel_size * 1.25)}
    I = _bufs(A)
    O = {"grid": torch.empty(n, g, g, g, device=DEV)}
    return U.Live(I, A, D, O, _on(lambda: mesh.voxelize_into(O["grid"], I["range"], I["voxel"])), ["grid"])


@case("collide_cylinder", "gnbv_collide_cylinder", "gnbv_collide_cylinder_batch")
def _c_collide():
    from gennbv_amd.env.collision import CollisionBody
    n, k = 3, 16
    _, mesh = _mesh(n, 16)
    mesh.objects()
    torch.cuda.synchronize()
    body = CollisionBody(radius=0.4, half_length=0.2, ground=True)
    A, D = {"poses": _scene_poses(1, n, k)}, {"poses": _scene_poses(2, n, k)}
    I = _bufs(A)
    O = {"one": torch.empty(n, dtype=torch.uint8, device=DEV), "all": torch.empty(n, k, dtype=torch.uint8, device=DEV)}

    def run():
        mesh.collide(I["poses"][:, 0], body, out=O["one"])
        mesh.collide_candidates(I["poses"], body, out=O["all"])
    return U.Live(I, A, D, O, _on(run), ["all"])


@case("sweep_sphere", "gnbv_sweep_sphere")
def _c_sweep_sphere():
    from gennbv_amd.env.collision import CollisionBody
    n, k = 3, 16
    _, mesh = _mesh(n, 16)
    body = CollisionBody(radius=0.3, half_length=0.1, ground=True, sweep=True)
    A = {"from": _scene_poses(1, n, 1)[:, 0].contiguous(), "to": _scene_poses(2, n, k)}
    D = {"from": _scene_poses(3, n, 1)[:, 0].contiguous(), "to": _scene_poses(4, n, k)}
    I = _bufs(A)
    O = {"code": torch.empty(n, k, dtype=torch.uint8, device=DEV)}
    return U.Live(I, A, D, O, _on(lambda: mesh.sweep_candidates(I["from"], I["to"], body, out=O["code"])), ["code"])


# ------------------------------------------------------------------------------------------------------------- GAE and Chamfer
@case("gae", "gnbv_gae_sb3", "gnbv_gae_rsl")
def _c_gae():
    from gennbv_amd import gae
    t, n = 9, 5

    def mk(s):
        return {"r": _rand(s, t, n), "v": _rand(s + 1, t, n), "es": _randint(s + 2, 0, 2, t, n, dtype=torch.uint8),
                "lv": _rand(s + 3, n), "dn": _randint(s + 4, 0, 2, n, dtype=torch.uint8)}
    A, D = mk(10), mk(20)
    I = _bufs(A)

    def run():
        adv, ret = gae.compute_returns_and_advantage(I["r"], I["v"], I["es"], I["lv"], I["dn"], 0.99, 0.95)
        ret2, adv2 = gae.compute_returns_rsl(I["r"], I["v"], I["es"], I["lv"], 0.99, 0.95, normalize=False)
        return {"adv": adv, "ret": ret, "adv_rsl": adv2, "ret_rsl": ret2}
    return U.Live(I, A, D, {}, _on(run), ["adv", "ret", "adv_rsl", "ret_rsl"])


@case("chamfer_distance", "gnbv_chamfer_distance")
def _c_chamfer():
    from gennbv_amd import _lib
    lib = _lib.load()
    n, m = 700, 531
    A, D = {"x": _rand(1, n, 3), "y": _rand(2, m, 3)}, {"x": _rand(3, n, 3), "y": _rand(4, m, 3)}
    I = _bufs(A)
    need = lib.gnbv_chamfer_workspace_bytes(n, m)
    O = {"out": torch.empty(1, device=DEV), "ws": torch.empty(need + 256, dtype=torch.uint8, device=DEV)}

    def call(stream):  # (metrics.chamfer_distance owns its workspace; here it is the case's, so that it takes the fill)
        _lib.check(lib.gnbv_chamfer_distance(I["x"].data_ptr(), n, I["y"].data_ptr(), m, O["out"].data_ptr(), O["ws"].data_ptr(),
                                             O["ws"].numel(), stream.cuda_stream), "gnbv_chamfer_distance")
    return U.Live(I, A, D, O, call, ["out"])


@case("metrics_chamfer", "gnbv_chamfer_distance")
def _c_metrics_chamfer():
    from gennbv_amd.eval import metrics
    A, D = {"x": _rand(1, 300, 3), "y": _rand(2, 257, 3)}, {"x": _rand(3, 300, 3), "y": _rand(4, 257, 3)}
    I = _bufs(A)
    return U.Live(I, A, D, {}, _on(lambda: {"cd": metrics.chamfer_distance(I["x"], I["y"])}), ["cd"])


# ------------------------------------------------------------------------------------------------- candidate-view kernels
def _gt_bits(scene, g):
    from gennbv_amd import _lib
    lib = _lib.load()
    n = scene.grid_gt.shape[0]
    grid = _dev(scene.grid_gt.float())
    bits = torch.zeros(n, lib.gnbv_grid_bit_words(g), dtype=torch.int32, device=DEV)
    _lib.check(lib.gnbv_pack_grid_bits(grid.data_ptr(), n, g, bits.data_ptr(), None, None), "gnbv_pack_grid_bits")
    torch.cuda.synchronize()
    return bits


def _view_gain_case(g, slab):
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.ops.view_gain import ViewGain, ViewGainSlab
    n, k = 2, 5
    cfg = _cfg(30, 37, g)
    scene = S.make_scenes(n, g, seed=2)
    kw = dict(stride=1, range_m=50.0, device=DEV, with_c2w=True, chunk=2)
    vg = ViewGainSlab(n, k, cfg, scene.range_gt, scene.voxel_size, slab=slab, **kw) if slab else \
        ViewGain(n, k, cfg, scene.range_gt, scene.voxel_size, **kw)
    A = {"tri": _tri(1, n, g), "poses": _look_poses(1, n, k, cfg)}
    D = {"tri": _tri(2, n, g), "poses": _look_poses(2, n, k, cfg)}
    I = _bufs(A)
    O = {"gain": vg.gain, "c2w": vg.c2w}
    if slab:
        O["workspace"] = vg.workspace
    return U.Live(I, A, D, O, _on(lambda: vg(I["tri"], I["poses"])), ["gain", "c2w"])


@case("view_gain", "gnbv_view_gain")
def _c_view_gain():
    return _view_gain_case(16, 0)


@case("view_gain_slab", "gnbv_view_gain_slab")
def _c_view_gain_slab():
    return _view_gain_case(20, 8)  # three slabs


def _gain_masks_case(g, slab):
    """the masks, then both set covers over them with rounds > 1"""
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.ops.gain_masks import ViewGainMasks, ViewGainMasksSlab
    n, k = 2, 6
    cfg = _cfg(30, 37, g)
    scene = S.make_scenes(n, g, seed=2)
    kw = dict(stride=1, range_m=50.0, device=DEV, chunk=2)
    op = ViewGainMasksSlab(n, k, cfg, scene.range_gt, scene.voxel_size, slab=slab, **kw) if slab else \
        ViewGainMasks(n, k, cfg, scene.range_gt, scene.voxel_size, **kw)
    A = {"tri": _tri(1, n, g), "poses": _look_poses(1, n, k, cfg), "contact": _randint(5, 0, 2, n, k, dtype=torch.uint8)}
    D = {"tri": _tri(2, n, g), "poses": _look_poses(2, n, k, cfg), "contact": _randint(6, 0, 2, n, k, dtype=torch.uint8)}
    I = _bufs(A)
    O = {"gain": op.gain, "unknown_bits": op.unknown_bits, "hit_bits": op.hit_bits}
    if slab:
        O["workspace"] = op.workspace

    def run():
        op(I["tri"], I["poses"])
        c1, g1, cov1 = op.plan(3, "unknown", contact=I["contact"])
        out = {"choice": c1.clone(), "cgain": g1.clone(), "covered": cov1.clone(), "gains0": op.gains0.clone()}
        c2, g2, _ = op.plan_weighted(3, (1, 4), contact=I["contact"])
        out.update({"choice_w": c2, "gain_w": g2, "plane_gain": op.plane_gain, "gains0_w": op.gains0})
        return out
    return U.Live(I, A, D, O, _on(run), ["gain", "unknown_bits", "hit_bits", "choice", "cgain", "covered", "gains0", "choice_w", "gain_w",
                                         "plane_gain", "gains0_w"])


@case("view_gain_masks", "gnbv_view_gain_masks", "gnbv_cover_greedy", "gnbv_cover_greedy_w")
def _c_gain_masks():
    return _gain_masks_case(16, 0)


@case("view_gain_slab_masks", "gnbv_view_gain_slab_masks", "gnbv_cover_greedy", "gnbv_cover_greedy_w")
def _c_gain_masks_slab():
    return _gain_masks_case(20, 8)


@case("view_cover", "gnbv_view_cover")
def _c_view_cover():
    from gennbv_amd.ops.view_cover import ViewCover
    n, g, k = 2, 16, 5
    cfg = _cfg(30, 37, g)
    scene, mesh = _mesh(n, g)
    gt = _gt_bits(scene, g)
    vc = ViewCover(mesh, cfg, scene.range_gt, scene.voxel_size, k, stride=1)
    A = {"poses": _look_poses(1, n, k, cfg), "scanned": torch.zeros_like(gt)}
    D = {"poses": _look_poses(2, n, k, cfg), "scanned": gt & _randint(3, -2 ** 31, 2 ** 31 - 1, *gt.shape)}
    I = _bufs(A)
    O = {"cover": vc.cover}
    return U.Live(I, A, D, O, _on(lambda: vc(I["poses"], gt, I["scanned"])), ["cover"])


@case("view_pool", "gnbv_view_cover_masks", "gnbv_cover_greedy")
def _c_view_pool():
    """the pool's masks in two batches (the constructor is the launch site), then a three-round plan"""
    from gennbv_amd.ops.view_pool import ViewPool
    n, g, p = 2, 16, 6
    cfg = _cfg(30, 37, g)
    scene, mesh = _mesh(n, g)
    gt = _gt_bits(scene, g)
    A, D = {"poses": _look_poses(1, n, p, cfg)}, {"poses": _look_poses(2, n, p, cfg)}
    I = _bufs(A)

    def run():
        pool = ViewPool(mesh, cfg, scene.range_gt, scene.voxel_size, gt, I["poses"], stride=1, batch=4)
        choice, gain, covered = pool.plan(3)
        return {"masks": pool.masks, "union": pool.union_bits(), "choice": choice.clone(), "gain": gain.clone(), "covered": covered.clone()}
    return U.Live(I, A, D, {}, _on(run), ["masks", "union", "choice", "gain", "covered"])


# ----------------------------------------------------------------------------------------------------- flight, map and frontier
def _lattice(g=16):
    from gennbv_amd.env.flight import FlightLattice
    return FlightLattice(_cfg(30, 37, g), stride=10)  # 9 x 9 x 6 nodes, 2 m apart


def _flight_inputs(seed, n, k, g, free=0.4):
    """the map, a start high above the boxes (a free node) and targets in the upper half: routes exist and differ"""
    poses, targets = _scene_poses(seed + 10, n, 1)[:, 0].contiguous(), _scene_poses(seed + 20, n, k)[..., :3].contiguous()
    poses[:, :2] *= 1.4
    poses[:, 2] = 8.0 + poses[:, 2] * 0.3
    targets[..., :2] *= 1.4
    targets[..., 2] = 5.0 + targets[..., 2] * 0.7
    return {"tri": _tri(seed, n, g, occ=0.002, free=free), "poses": poses, "targets": targets}


@case("flight_field_mesh", "gnbv_flight_field", "gnbv_flight_query", "gnbv_flight_path")
def _c_flight_mesh():
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.ops.flight_field import FlightField
    n, k = 2, 7
    lat = _lattice()
    _, mesh = _mesh(n, 16)
    f = FlightField(mesh, lat, CollisionBody(radius=0.1, half_length=0.02, ground=True))
    torch.cuda.synchronize()
    A, D = ({k_: v for k_, v in _flight_inputs(s, n, k, 16).items() if k_ != "tri"} for s in (1, 2))
    I = _bufs(A)
    O = {"field": f.field, "status": f.status, "cost": torch.empty(n, k, dtype=torch.int32, device=DEV),
         "nodes": torch.empty(n, 32, dtype=torch.int32, device=DEV), "len": torch.empty(n, dtype=torch.int32, device=DEV)}

    def run():
        f.update(I["poses"])
        f.cost_mm(I["targets"], out=O["cost"])
        f.path_into(I["targets"][:, 0], O["nodes"], O["len"])
    return U.Live(I, A, D, O, _on(run), ["field", "cost", "nodes", "len"])  # (status is 0 in every settled field)


def _flight_map_case(unknown):
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.ops.flight_field import BeliefFlightField
    n, k, g = 2, 7, 16
    lat = _lattice(g)
    scene = S.make_scenes(n, g, seed=2)
    f = BeliefFlightField(n, lat, CollisionBody(radius=0.1, half_length=0.02, ground=True), scene.range_gt, scene.voxel_size, g,
                          unknown=unknown, outside="free", unknown_penalty_m=0.5 if unknown == "costly" else None, device=DEV)
    # (costly: unknown voxels stop a straight leg, so the map is mostly seen -- some legs pass, some do not)
    free = 0.97 if unknown == "costly" else 0.4
    A, D = _flight_inputs(1, n, k, g, free), _flight_inputs(2, n, k, g, free)
    I = _bufs(A)
    O = {"blocked_map": f.blocked_map, "field": f.field, "status": f.status, "cost": torch.empty(n, k, dtype=torch.int32, device=DEV),
         "nodes": torch.empty(n, 32, dtype=torch.int32, device=DEV), "len": torch.empty(n, dtype=torch.int32, device=DEV),
         "code": torch.empty(n, k, dtype=torch.uint8, device=DEV)}
    if unknown == "costly":
        O["costly_map"] = f.costly_map

    def run():
        f.refresh(I["tri"])
        f.update(I["poses"])
        f.cost_mm(I["targets"], out=O["cost"])
        f.path_into(I["targets"][:, 0], O["nodes"], O["len"])
        f.sweep(I["poses"], I["targets"], tri=I["tri"], out=O["code"])
    return U.Live(I, A, D, O, _on(run), [k_ for k_ in O if k_ != "status"])  # (status is 0 in every settled field)


@case("flight_map", "gnbv_flight_blocked_tri", "gnbv_flight_field", "gnbv_flight_query", "gnbv_flight_path", "gnbv_sweep_tri")
def _c_flight_map():
    return _flight_map_case("free")


@case("flight_map_costly", "gnbv_flight_classify_tri", "gnbv_flight_field_w", "gnbv_flight_query", "gnbv_flight_path_w", "gnbv_sweep_tri")
def _c_flight_map_costly():
    return _flight_map_case("costly")


@case("frontier", "gnbv_frontier_tri")
def _c_frontier():
    from gennbv_amd.ops.frontier import Frontier
    n, g = 3, 20
    fr = Frontier(n, g, block=4, device=DEV, keep_bits=True, slab=4)  # five slabs per env
    A, D = {"tri": _tri(1, n, g)}, {"tri": _tri(2, n, g)}
    I = _bufs(A)
    return U.Live(I, A, D, {"blocks": fr.blocks, "bits": fr.bits}, _on(lambda: fr(I["tri"])), ["blocks", "bits"])


@case("frontier_viewpoints", "gnbv_frontier_viewpoints")
def _c_frontier_viewpoints():
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.ops.frontier_view import FrontierViewpoints
    n, g, t = 2, 16, 5
    lat = _lattice(g)
    scene = S.make_scenes(n, g, seed=2)
    op = FrontierViewpoints(n, g, lat, scene.range_gt, scene.voxel_size, t, 0.5, 8.0, max_unknown=3 * g, device=DEV, chunk=2)

    def mk(s):
        return {"tri": _tri(s, n, g, occ=0.01), "field": _randint(s + 1, 0, 50000, n, lat.num_nodes),
                "targets": _randint(s + 2, 0, g, n, t, 3)}
    A, D = mk(1), mk(5)
    I = _bufs(A)
    O = {"node": op.node, "cost": op.cost_mm, "count": op.count}
    return U.Live(I, A, D, O, _on(lambda: op(I["tri"], I["field"], I["targets"])), ["node", "cost", "count"])


@case("tour_route", "gnbv_tour_route")
def _c_tour():
    from gennbv_amd.ops import tour
    n, p = 3, 9

    def mk(s):
        pts = _rand(s, n, p, 3, lo=-5.0, hi=5.0)
        d = ((pts[:, :, None] - pts[:, None]).double().norm(dim=-1) * 1000.0).round().to(torch.int32)
        return {"dist": d.contiguous(), "count": _randint(s + 1, 4, p + 1, n)}
    A, D = mk(1), mk(2)
    I = _bufs(A)

    def run():
        r = tour.route_tour(I["dist"], I["count"])
        return {"order": r.order, "routed": r.routed, "length": r.length_mm}
    return U.Live(I, A, D, {}, _on(run), ["order", "routed", "length"])


# --------------------------------------------------------------------------------------------------------------- losses and Adam
HEADS = [3, 4, 2]


@case("imitation_loss", "gnbv_imitation_loss")
def _c_imitation():
    import types
    from gennbv_amd.ops.imitation_ops import ImitationLossOp
    b, k, m = 5, 3, 11
    op = ImitationLossOp(b, HEADS, k, DEV, max_rows=4, label_smoothing=0.1, ent_coef=0.01, vf_coef=0.5)

    def mk(s):
        cand = torch.stack([_randint(s + i, 0, d, m, k, dtype=torch.int64) for i, d in enumerate(HEADS)], -1).contiguous()
        return {"logits": _rand(s + 10, b, sum(HEADS), lo=-2.0, hi=2.0), "values": _rand(s + 11, b), "cand": cand,
                "cand_w": _rand(s + 12, m, k), "sample_w": _rand(s + 13, m), "returns": _rand(s + 14, m),
                "rows": _randint(s + 15, 0, m, b, dtype=torch.int64)}
    A, D = mk(1), mk(50)
    I = _bufs(A)
    I["rows"] = op.rows
    for name in ("stats_row", "flags", "scratch"):  # in/out state the kernel expects zero-initialised once: reloaded, not filled
        I[name] = getattr(op, name)
        A[name] = D[name] = torch.zeros_like(I[name])
    op.bind(types.SimpleNamespace(cand=I["cand"], cand_w=I["cand_w"], sample_w=I["sample_w"], returns=I["returns"]))
    O = {"d_logits": op.d_logits, "d_values": op.d_values, "stats": op.stats}
    return U.Live(I, A, D, O, _on(lambda: op(I["logits"], I["values"])), ["d_logits", "d_values", "stats"])


@case("ppo_loss", "gnbv_gather_minibatch", "gnbv_ppo_loss", "gnbv_ppo_loss_finish")
def _c_ppo_loss():
    """the gather, the loss with deferred statistics, then their launch of its own"""
    import types
    from gennbv_amd.ops.ppo_ops import PpoLossOp
    b, rows = 5, 12
    op = PpoLossOp(b, HEADS, DEV, max_rows=4, clip_range=0.2, clip_range_vf=None, ent_coef=0.01, vf_coef=0.5, policy_scale=1.0,
                   target_kl=0.05)
    op.args.defer_stats = 1

    def mk(s):
        acts = torch.stack([_randint(s + i, 0, d, rows) for i, d in enumerate(HEADS)], -1).float().contiguous()
        return {"logits": _rand(s + 10, b, sum(HEADS), lo=-2.0, hi=2.0), "values": _rand(s + 11, b), "actions": acts,
                "buf_values": _rand(s + 12, rows), "log_probs": _rand(s + 13, rows, lo=-4.0, hi=-2.0), "advantages": _rand(s + 14, rows, lo=-1.0),
                "returns": _rand(s + 15, rows), "rows": _randint(s + 16, 0, rows, b, dtype=torch.int64)}
    A, D = mk(1), mk(50)
    I = _bufs(A)
    I["rows"] = op.rows
    for name in ("stats_row", "stop_flag", "scratch"):
        I[name] = getattr(op, name)
        A[name] = D[name] = torch.zeros_like(I[name])
    buf = types.SimpleNamespace(actions=I["actions"], values=I["buf_values"], log_probs=I["log_probs"], advantages=I["advantages"],
                                returns=I["returns"])
    O = {"d_logits": op.d_logits, "d_values": op.d_values, "stats": op.stats, "g_actions": op.actions, "g_values": op.old_values,
         "g_log_prob": op.old_log_prob, "g_adv": op.advantages, "g_ret": op.returns}

    def run():
        op.gather(buf)
        op(I["logits"], I["values"])
        op.finish_stats()
    return U.Live(I, A, D, O, _on(run), ["d_logits", "d_values", "stats", "g_actions", "g_adv"])


@case("flat_adam", "gnbv_clip_adam_step_ex", "gnbv_sq_partials", "gnbv_adam_shard_step")
def _c_flat_adam():
    from gennbv_amd.ops.ppo_ops import FlatAdam
    torch.manual_seed(3)
    mod = torch.nn.Linear(37, 29).to(DEV)
    opt = FlatAdam(mod, lr=1e-2)
    n = opt.n
    assert opt.enable_shard(0, 1000, 0, 2)
    I = {"params": opt.params, "grads": opt.grads, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "step": opt.step_count,
         "shard_grad": opt.shard["grad"]}

    def mk(s):
        return {"params": _rand(s, n, lo=-1.0), "grads": _rand(s + 1, n, lo=-3.0, hi=3.0), "exp_avg": _rand(s + 2, n, lo=-0.1, hi=0.1),
                "exp_avg_sq": _rand(s + 3, n, hi=0.1), "step": torch.full((1,), 2 + s, dtype=torch.int64, device=DEV),
                "shard_grad": _rand(s + 4, 500, lo=-3.0, hi=3.0)}
    A, D = mk(1), mk(50)
    O = {"norm_out": opt.norm_out, "ws": opt.ws, "sq": opt.shard["sq"]}

    def run():
        opt.step(0.5)
        opt.shard_sq()
        opt.shard_step()
    return U.Live(I, A, D, O, _on(run), ["params", "exp_avg", "exp_avg_sq", "step", "norm_out", "sq"])


@case("multicategorical_sample", "gnbv_multicategorical_sample")
def _c_sample():
    from gennbv_amd import _lib
    lib = _lib.load()
    b, h = 37, len(HEADS)
    dims = (C.c_int * h)(*HEADS)
    A = {"logits": _rand(1, b, sum(HEADS), lo=-2.0, hi=2.0), "u": _rand(2, b, h)}
    D = {"logits": _rand(3, b, sum(HEADS), lo=-2.0, hi=2.0), "u": _rand(4, b, h)}
    I = _bufs(A)
    O = {"actions": torch.empty(b, h, dtype=torch.int64, device=DEV), "log_prob": torch.empty(b, device=DEV)}

    def call(stream):  # (the wrapper draws its uniforms with torch.rand: not repeatable between the runs)
        _lib.check(lib.gnbv_multicategorical_sample(I["logits"].data_ptr(), b, sum(HEADS), h, dims, I["u"].data_ptr(), 0,
                                                    O["actions"].data_ptr(), O["log_prob"].data_ptr(), stream.cuda_stream),
                   "gnbv_multicategorical_sample")
    return U.Live(I, A, D, O, call, ["actions", "log_prob"])


@case("ppo_loss_rsl", "gnbv_ppo_loss_rsl")
def _c_ppo_loss_rsl():
    from gennbv_amd import _lib
    lib = _lib.load()
    b = 37
    names = ("lp", "olp", "adv", "v", "tv", "ret")

    def mk(s):
        d = {k: _rand(s + i, b, lo=-1.0) for i, k in enumerate(names)}
        d["sums"] = torch.zeros(2, device=DEV)  # accumulated over the minibatches of an update: in/out
        return d
    A, D = mk(1), mk(50)
    I = _bufs(A)
    O = {k: torch.empty(b, device=DEV) for k in ("d_lp", "d_v", "d_ent")}

    def call(stream):
        _lib.check(lib.gnbv_ppo_loss_rsl(b, *[I[k].data_ptr() for k in names], 0.2, 1.0, 0.01, 1, O["d_lp"].data_ptr(), O["d_v"].data_ptr(),
                                         O["d_ent"].data_ptr(), I["sums"].data_ptr(), stream.cuda_stream), "gnbv_ppo_loss_rsl")
    return U.Live(I, A, D, O, call, ["d_lp", "d_v", "sums"])


@case("rollout_add", "gnbv_rollout_add")
def _c_rollout_add():
    from gennbv_amd import _lib
    lib = _lib.load()
    n, ad = 5, 6

    def mk(s):
        return {"actions": _randint(s, 0, 50, n, ad, dtype=torch.int64), "rewards": _rand(s + 1, n), "time_outs": _randint(s + 2, 0, 2, n, dtype=torch.uint8),
                "tv": _rand(s + 3, n), "es": _randint(s + 4, 0, 2, n, dtype=torch.uint8), "values": _rand(s + 5, n), "lp": _rand(s + 6, n, lo=-3.0, hi=0.0)}
    A, D = mk(1), mk(50)
    I = _bufs(A)
    O = {"b_actions": torch.empty(n, ad, device=DEV), "b_rewards": torch.empty(n, device=DEV), "b_es": torch.empty(n, dtype=torch.uint8, device=DEV),
         "b_values": torch.empty(n, device=DEV), "b_lp": torch.empty(n, device=DEV)}

    def call(stream):
        _lib.check(lib.gnbv_rollout_add(n, ad, I["actions"].data_ptr(), I["rewards"].data_ptr(), I["time_outs"].data_ptr(), I["tv"].data_ptr(), 1,
                                        0.99, I["es"].data_ptr(), I["values"].data_ptr(), I["lp"].data_ptr(), O["b_actions"].data_ptr(),
                                        O["b_rewards"].data_ptr(), O["b_es"].data_ptr(), O["b_values"].data_ptr(), O["b_lp"].data_ptr(),
                                        stream.cuda_stream), "gnbv_rollout_add")
    return U.Live(I, A, D, O, call, list(O))


# ------------------------------------------------------------------------------------------------------------------- scan sets
@case("scan_accumulator", "gnbv_scan_add_frame", "gnbv_scan_score", "gnbv_scan_clear", "gnbv_scan_export")
def _c_scan():
    from gennbv_amd import _lib
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.eval.scan_accumulator import ScanAccumulator
    n, h, w = 3, 30, 37
    _, _, fr = _frames(n, 16, h, w)
    acc = ScanAccumulator(n, [_rand(7 + e, 300 + e, 3, lo=-4.0, hi=6.0) for e in range(n)], h, w, S.inverse_intrinsics(h, w), -50.0,
                          capacity_per_env=2048, device=DEV)
    keys = ("depth", "seg", "c2w")
    A, D = ({k: f[k] for k in keys} for f in fr)
    state = {"table": acc.table, "counts": acc.counts, "state": acc._state}
    for k, t in state.items():  # the empty sets, reloaded before every call
        A[k] = D[k] = t.clone()
    I = _bufs({k: A[k] for k in keys})
    I.update(state)
    every = torch.ones(n, dtype=torch.uint8, device=DEV)
    first = torch.tensor([1, 0, 0], dtype=torch.uint8, device=DEV)
    O = {"keys": acc.keys, "ws": acc._ws, "cloud": torch.empty(acc.capacity, 3, device=DEV), "counts_before": torch.empty_like(acc.counts)}
    lib = _lib.load()

    def run():
        acc.add_frame(I["depth"], I["seg"], I["c2w"])
        acc.score(every)
        O["counts_before"].copy_(acc.counts)
        # (ScanAccumulator.points reads the count back first; the export itself, into a buffer of the full capacity)
        _lib.check(lib.gnbv_scan_export(C.byref(acc._set), 1, O["cloud"].data_ptr(), acc._ws_ptr, acc._ws_bytes, _lib.stream_ptr(acc.device)),
                   "gnbv_scan_export")
        acc.clear(first)  # env 0 ends empty: a clear that ran early, before the frame, would leave its keys in place
    return U.Live(I, A, D, O, _on(run), ["state", "counts", "counts_before", "cloud"])


# ------------------------------------------------------------------------------------------------------------ env-step kernels
def _env_lattice(cfg):
    import numpy as np
    from gennbv_amd import _lib
    lat = _lib.GnbvLattice()
    for i in range(6):
        lat.clip_low[i], lat.clip_up[i], lat.init_action[i] = cfg.clip_pose_idx_low[i], cfg.clip_pose_idx_up[i], cfg.init_action[i]
        lat.action_unit[i] = float(np.float32(cfg.action_unit[i]))
        lat.pose_low[i] = float(np.float32(cfg.clip_pose_low[i]))
        lat.init_pose[i] = float(np.float32(cfg.init_pose_buf[i]))
    return lat


def _observe_case(fused):
    from gennbv_amd import _lib
    lib = _lib.load()
    n, stack, h, w, oh, ow = 3, 4, 30, 37, 8, 8
    cfg = _cfg(h, w, 16)
    lat = _env_lattice(cfg)
    row = stack * 6 + 2 * oh * ow

    def mk(s):
        return {"actions": _randint(s, -5, 90, n, 6, dtype=torch.int64), "elb": _randint(s + 1, 0, 3, n, dtype=torch.int64),
                "hist": _rand(s + 2, n, stack, 6), "reset": _randint(s + 3, 0, 2, n, dtype=torch.uint8),
                "rgba": _randint(s + 4, 0, 256, n, h, w, 4, dtype=torch.uint8), "gray_prev": _rand(s + 5, n, oh * ow)}
    A, D = mk(1), mk(50)
    I = _bufs(A)
    O = {"actions_out": torch.empty(n, 6, dtype=torch.int64, device=DEV), "poses": torch.empty(n, 6, device=DEV), "obs": torch.empty(n, row, device=DEV)}
    p = {k: v.data_ptr() for k, v in {**I, **O}.items()}
    rgb = p["obs"] + stack * 6 * 4

    def call(stream):
        s = stream.cuda_stream
        if fused:
            _lib.check(lib.gnbv_env_observe(p["actions"], C.byref(lat), p["elb"], n, p["actions_out"], p["poses"], p["hist"], p["reset"], stack,
                                            p["obs"], row, p["rgba"], p["gray_prev"], h, w, oh, ow, rgb, s), "gnbv_env_observe")
            return
        _lib.check(lib.gnbv_env_pre_step(p["actions"], C.byref(lat), p["elb"], n, p["actions_out"], p["poses"], s), "gnbv_env_pre_step")
        _lib.check(lib.gnbv_env_obs_state(p["hist"], p["poses"], p["reset"], C.byref(lat), n, stack, p["obs"], row, s), "gnbv_env_obs_state")
        _lib.check(lib.gnbv_env_obs_rgb(p["rgba"], p["gray_prev"], p["reset"], n, h, w, oh, ow, rgb, row, s), "gnbv_env_obs_rgb")
    return U.Live(I, A, D, O, call, ["actions_out", "poses", "obs", "elb", "hist", "gray_prev"])


@case("env_observe", "gnbv_env_observe")
def _c_env_observe():
    return _observe_case(True)


@case("env_observe_three", "gnbv_env_pre_step", "gnbv_env_obs_state", "gnbv_env_obs_rgb")
def _c_env_observe_three():
    return _observe_case(False)


@case("env_post_step", "gnbv_env_post_step", "gnbv_env_post_step_contacts")
def _c_env_post_step():
    from gennbv_amd import _lib
    from tests.envstep_util import PostState
    lib = _lib.load()
    n = 37
    cfg = _cfg(30, 37, 16)

    def mk(seed):
        st = PostState(n, cfg, 6, seed)
        g = torch.Generator().manual_seed(seed + 1)
        st.prev_ratio.copy_(torch.rand(n, generator=g) * 0.2)
        st.advance(g)
        d = {k: getattr(st, k) for k in PostState.NAMES}
        d["contact"] = _randint(seed + 2, 0, 2, n, dtype=torch.uint8)
        return st, d
    live_state, _ = mk(0)
    _, A = mk(1)
    _, D = mk(2)
    I = {k: getattr(live_state, k) for k in PostState.NAMES}
    I["contact"] = torch.empty(n, dtype=torch.uint8, device=DEV)
    post = live_state.struct()
    O = {"first_rewards": torch.empty(n, device=DEV)}

    def call(stream):
        s = stream.cuda_stream
        _lib.check(lib.gnbv_env_post_step(C.byref(post), s), "gnbv_env_post_step")
        with torch.cuda.stream(stream):
            O["first_rewards"].copy_(I["rewards"])
        _lib.check(lib.gnbv_env_post_step_contacts(C.byref(post), I["contact"].data_ptr(), s), "gnbv_env_post_step_contacts")
    return U.Live(I, A, D, O, call, ["first_rewards", "rewards", "dones", "reset_mask", "coverage_ratio", "episode_length_buf", "episode_info",
                                     "episode_sums"])


# ---------------------------------------------------------------------------------------------- encoder, fc layers, policy head
def _policy(g):
    from tests import policy_util as pu
    pol, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    return pol, pu


def _obs(seed, b, g, pu, compact=False):
    """observation rows [state | tri-class grid | rgb] (compact: [state | rgb] and the int8 grid rows)"""
    state = _rand(seed, b, pu.STACK * 6, lo=-3.0, hi=3.0)
    grid = _tri(seed + 1, b, g, occ=0.1)
    rgb = _rand(seed + 2, b, 8192)
    if compact:
        return torch.cat((state, rgb), 1).contiguous(), grid
    return torch.cat((state, grid.float(), rgb), 1).contiguous()


def _bn_state(pol):
    """BatchNorm running statistics: in/out state of a training forward"""
    return {k: v for k, v in pol.state_dict(keep_vars=True).items() if "running_" in k or "num_batches" in k}


def _policy_train_case(g, b):
    """a training forward and backward of the whole policy: conv stack, fc layers, pose branch (the wrapper forks it onto a second stream
    and joins it: FORKS), BatchNorm statistics"""
    pol, pu = _policy(g)
    pol.set_training_mode(True)
    acts = lambda s: torch.stack([_randint(s + i, 0, n, b) for i, n in enumerate(pu.NVEC)], -1).float().contiguous()  # noqa: E731
    A, D = {"obs": _obs(1, b, g, pu), "actions": acts(5)}, {"obs": _obs(20, b, g, pu), "actions": acts(25)}
    I = _bufs(A)
    for k, v in _bn_state(pol).items():
        I[k] = v
        A[k] = D[k] = v.detach().clone()
    w = torch.linspace(0.5, 1.5, b, device=DEV)
    names = [n for n, _ in pol.named_parameters()]
    pick = [names[0], names[len(names) // 2], names[-2]] + [n for n in names if "output_layer_grid" in n or "naive_encoder_action" in n]

    def run():
        pol.zero_grad()
        values, log_prob, entropy = pol.evaluate_actions(I["obs"], I["actions"])
        loss = (values.flatten() * w).sum() + (log_prob * w.flip(0)).sum() + 0.3 * (entropy * w).sum()
        loss.backward()
        out = {"values": values.detach(), "log_prob": log_prob.detach()}
        out.update({"grad:" + n: p.grad for n, p in pol.named_parameters() if n in pick})
        return out
    bn = [k for k in I if "running_" in k]
    return U.Live(I, A, D, {}, _on(run), ["values", "log_prob"] + ["grad:" + n for n in dict.fromkeys(pick)] + bn)


@case("encoder_train", "gnbv_encoder_grid_forward", "gnbv_encoder_grid_backward", "gnbv_linear_forward", "gnbv_linear_bwd_prep",
      "gnbv_linear_bwd_dx", "gnbv_linear_bwd_dw", "gnbv_pose_encode")
def _c_encoder_train():
    return _policy_train_case(20, 16)


@case("encoder_train_g64", "gnbv_encoder_grid_forward", "gnbv_encoder_grid_backward", "gnbv_linear_forward_fold", "gnbv_pose_encode")
def _c_encoder_train_g64():
    return _policy_train_case(64, 2)


FORKS.add("encoder_train_g64")


def _rollout_plan_case(g, n, compact):
    """ops/rollout_plan.RolloutForward: the prepared inference forward (its pose branch runs on the plan's own second stream: FORKS)"""
    from gennbv_amd.ops import encoder_ops
    from gennbv_amd.ops.rollout_plan import RolloutForward
    pol, pu = _policy(g)
    pol.set_training_mode(False)
    pol._fused_rollout = True
    plan = RolloutForward.build(pol, n)
    assert plan is not None and plan.fold == compact
    if compact:
        (a0, a1), (d0, d1) = _obs(1, n, g, pu, True), _obs(20, n, g, pu, True)
        A, D = {"obs": a0, "grid": a1}, {"obs": d0, "grid": d1}
    else:
        A, D = {"obs": _obs(1, n, g, pu)}, {"obs": _obs(20, n, g, pu)}
    I = _bufs(A)
    obs = encoder_ops.DenseObs(I["obs"], I["grid"], pu.STACK * 6) if compact else I["obs"]
    O = {"fg": plan.fg, "fa": plan.fa, "feat": plan.feat, "y2": plan.y2}

    def run():
        with torch.no_grad():
            assert plan.prepare() and plan.applies_to(obs)
            logits, values = plan(obs)
        return {"logits": logits, "values": values}
    return U.Live(I, A, D, O, _on(run), ["logits", "values", "fg", "fa", "feat"])


@case("rollout_plan", "gnbv_encoder_grid_forward", "gnbv_linear_forward", "gnbv_pose_encode", "gnbv_policy_head_forward")
def _c_rollout_plan():
    return _rollout_plan_case(20, 3, False)


@case("rollout_plan_g64", "gnbv_encoder_eval_prepare", "gnbv_encoder_grid_forward", "gnbv_linear_forward_fold", "gnbv_pose_encode",
      "gnbv_policy_head_forward")
def _c_rollout_plan_g64():
    return _rollout_plan_case(64, 2, True)


FORKS.add("rollout_plan_g64")


@case("input_autocorr", "gnbv_input_autocorr")
def _c_input_autocorr():
    from gennbv_amd import _lib
    from gennbv_amd.ops import encoder_ops
    n, g = 3, 16
    A, D = {"grid": _tri(1, n, g, occ=0.1)}, {"grid": _tri(2, n, g, occ=0.1)}
    I = _bufs(A)
    O = {"ac": torch.empty(n, _lib.load().gnbv_input_autocorr_row_ints(), dtype=torch.int32, device=DEV)}
    return U.Live(I, A, D, O, _on(lambda: encoder_ops.input_autocorr(I["grid"], g, out=O["ac"])), ["ac"])


@case("linear_bwd_dw_variants", "gnbv_linear_forward", "gnbv_linear_bwd_prep", "gnbv_linear_bwd_dw_sq", "gnbv_linear_forward_fold",
      "gnbv_linear_bwd_dw_fold")
def _c_linear_variants():
    """the fc layer's variants the training case above does not take: dW with its squared sum, and BatchNorm-2 folded into the operand
    load (forward and dW), at M = 16, N = 64, K = 16 channels x 512 (the smallest P the fold takes)"""
    from gennbv_amd import _lib
    lib = _lib.load()
    m, n, c, p_ = 16, 64, 16, 512
    k = c * p_
    assert lib.gnbv_linear_fold_ok(m, n, k, p_)

    def mk(s):
        return {"x": _rand(s, m, k, lo=-1.0), "w": _rand(s + 1, n, k, lo=-0.1, hi=0.1), "b": _rand(s + 2, n, lo=-0.1, hi=0.1),
                "d_out": _rand(s + 3, m, n, lo=-1.0), "scale": _rand(s + 4, c, lo=0.5, hi=1.5), "shift": _rand(s + 5, c, lo=-0.2, hi=0.2)}
    A, D = mk(1), mk(30)
    I = _bufs(A)
    f32 = dict(dtype=torch.float32, device=DEV)
    O = {"out": torch.empty(m, n, **f32), "out_fold": torch.empty(m, n, **f32), "db": torch.empty(n, **f32), "dw": torch.empty(n, k, **f32),
         "dw_fold": torch.empty(n, k, **f32), "sq": torch.empty(lib.gnbv_linear_bwd_dw_sq_parts(k), dtype=torch.float64, device=DEV),
         "sq_fold": torch.empty(lib.gnbv_linear_bwd_dw_sq_parts(k), dtype=torch.float64, device=DEV),
         "ws": torch.empty(lib.gnbv_linear_workspace_bytes(m, n, k), dtype=torch.uint8, device=DEV),
         "ws_bwd": torch.empty(lib.gnbv_linear_bwd_workspace_bytes(m, n, k), dtype=torch.uint8, device=DEV)}
    p = {k_: v.data_ptr() for k_, v in {**I, **O}.items()}

    def call(stream):
        s = stream.cuda_stream
        _lib.check(lib.gnbv_linear_forward(p["x"], p["w"], p["b"], m, n, k, 1, p["out"], p["ws"], O["ws"].numel(), s), "gnbv_linear_forward")
        _lib.check(lib.gnbv_linear_bwd_prep(p["d_out"], p["out"], m, n, p["db"], p["ws_bwd"], O["ws_bwd"].numel(), s), "gnbv_linear_bwd_prep")
        _lib.check(lib.gnbv_linear_bwd_dw_sq(p["ws_bwd"], p["x"], m, n, k, p["dw"], p["sq"], s), "gnbv_linear_bwd_dw_sq")
        _lib.check(lib.gnbv_linear_forward_fold(p["x"], p["scale"], p["shift"], p_, None, p["w"], p["b"], m, n, k, 1, p["out_fold"], p["ws"],
                                                O["ws"].numel(), s), "gnbv_linear_forward_fold")
        _lib.check(lib.gnbv_linear_bwd_prep(p["d_out"], p["out_fold"], m, n, p["db"], p["ws_bwd"], O["ws_bwd"].numel(), s), "gnbv_linear_bwd_prep")
        _lib.check(lib.gnbv_linear_bwd_dw_fold(p["ws_bwd"], p["x"], p["scale"], p["shift"], p_, m, n, k, p["dw_fold"], p["sq_fold"], s),
                   "gnbv_linear_bwd_dw_fold")
    return U.Live(I, A, D, O, call, ["out", "out_fold", "db", "dw", "dw_fold", "sq", "sq_fold"])


@case("policy_head", "gnbv_policy_head_forward", "gnbv_policy_head_backward")
def _c_policy_head():
    from gennbv_amd import _lib
    lib = _lib.load()
    m, k1, k2, f, a = 5, 32, 48, 64, 9
    shapes = {"fa": (m, k1), "fg": (m, k2), "w_out": (f, k1 + k2), "b_out": (f,), "w_act": (a, f), "b_act": (a,), "w_val": (1, f), "b_val": (1,),
              "d_logits": (m, a), "d_values": (m,)}

    def mk(s):
        return {k_: _rand(s + i, *shp, lo=-0.5, hi=0.5) for i, (k_, shp) in enumerate(shapes.items())}
    A, D = mk(1), mk(40)
    I = _bufs(A)
    outs = {"feat": (m, f), "logits": (m, a), "values": (m,), "dh": (m, f), "d_fa": (m, k1), "d_fg": (m, k2), "g_w_out": (f, k1 + k2), "g_b_out": (f,),
            "g_w_act": (a, f), "g_b_act": (a,), "g_w_val": (1, f), "g_b_val": (1,)}
    O = {k_: torch.empty(*shp, device=DEV) for k_, shp in outs.items()}
    p = {k_: v.data_ptr() for k_, v in {**I, **O}.items()}

    def call(stream):
        s = stream.cuda_stream
        _lib.check(lib.gnbv_policy_head_forward(p["fa"], p["fg"], m, k1, k2, p["w_out"], p["b_out"], f, p["w_act"], p["b_act"], a, p["w_val"], p["b_val"],
                                                p["feat"], p["logits"], p["values"], s), "gnbv_policy_head_forward")
        _lib.check(lib.gnbv_policy_head_backward(p["fa"], p["fg"], m, k1, k2, p["feat"], p["d_logits"], p["d_values"], p["w_out"], f, p["w_act"], a,
                                                 p["w_val"], p["dh"], p["d_fa"], p["d_fg"], p["g_w_out"], p["g_b_out"], p["g_w_act"], p["g_b_act"],
                                                 p["g_w_val"], p["g_b_val"], s), "gnbv_policy_head_backward")
    return U.Live(I, A, D, O, call, [k_ for k_ in O if k_ != "dh"])


@case("clip_adam_step", "gnbv_clip_adam_step", "gnbv_clip_adam_step_rotate")
def _c_clip_adam_step():
    """the two plain-argument forms of the optimizer step, one after the other on the same buffers; the second rotates the row table"""
    from gennbv_amd import _lib
    lib = _lib.load()
    n, rows, rl = 5000, 3, 4

    def mk(s):
        return {"params": _rand(s, n, lo=-1.0), "grads": _rand(s + 1, n, lo=-3.0, hi=3.0), "m": _rand(s + 2, n, lo=-0.1, hi=0.1), "v": _rand(s + 3, n, hi=0.1),
                "step": torch.full((1,), 2 + s, dtype=torch.int64, device=DEV), "stop": torch.zeros(1, dtype=torch.int32, device=DEV),
                "kl": _rand(s + 4, 1, hi=0.01), "table": _randint(s + 5, 0, 1000, rows, rl, dtype=torch.int64),
                "counter": torch.full((1,), s % rows, dtype=torch.int32, device=DEV)}
    A, D = mk(1), mk(41)
    I = _bufs(A)
    O = {"norm": torch.empty(2, device=DEV), "norm2": torch.empty(2, device=DEV), "row": torch.empty(rl, dtype=torch.int64, device=DEV),
         "ws": torch.empty(lib.gnbv_adam_workspace_bytes(), dtype=torch.uint8, device=DEV)}
    p = {k_: v.data_ptr() for k_, v in {**I, **O}.items()}

    def call(stream):
        s = stream.cuda_stream
        head = (p["params"], p["grads"], p["m"], p["v"], n, 0.5, 1e-2, 0.9, 0.999, 1e-5, p["step"], p["stop"], 1.0, p["kl"], 0.05)
        _lib.check(lib.gnbv_clip_adam_step(*head, p["norm"], p["ws"], O["ws"].numel(), s), "gnbv_clip_adam_step")
        _lib.check(lib.gnbv_clip_adam_step_rotate(*head, p["norm2"], p["ws"], O["ws"].numel(), p["table"], rows, rl, p["row"], p["counter"], s),
                   "gnbv_clip_adam_step_rotate")
    return U.Live(I, A, D, O, call, ["params", "m", "v", "step", "norm", "norm2", "row", "counter"])


# ------------------------------------------------------------------------------------------------------- rollout containers
@case("rollout_buffer_add", "gnbv_rollout_add")
def _c_rollout_buffer_add():
    import numpy as np
    from gennbv_amd.sb3.buffers import TensorRolloutBuffer_Grid_Obs
    from gennbv_amd.spaces import Box, MultiDiscrete
    n = 5
    buf = TensorRolloutBuffer_Grid_Obs(2, Box(-np.inf, np.inf, shape=(10,), dtype=np.float32), MultiDiscrete([81, 81, 51, 1, 13, 13]), DEV,
                                       gae_lambda=0.95, gamma=0.99, n_envs=n)

    def mk(s):
        return {"actions": _randint(s, 0, 50, n, 6, dtype=torch.int64), "rewards": _rand(s + 1, n), "time_outs": _randint(s + 2, 0, 2, n, dtype=torch.uint8),
                "tv": _rand(s + 3, n, 1), "es": _randint(s + 4, 0, 2, n, dtype=torch.uint8), "values": _rand(s + 5, n, 1), "lp": _rand(s + 6, n, lo=-3.0, hi=0.0)}
    A, D = mk(1), mk(50)
    I = _bufs(A)
    O = {"b_actions": buf.actions, "b_rewards": buf.rewards, "b_es": buf.episode_starts, "b_values": buf.values, "b_lp": buf.log_probs}

    def run():
        buf.step = buf.pos = 1
        buf.add_bootstrapped(buf.observations[1], I["actions"], I["rewards"], I["time_outs"], I["tv"], 0.99, I["es"], I["values"], I["lp"])
    return U.Live(I, A, D, O, _on(run), list(O))


@case("rollout_storage_rsl", "gnbv_gae_rsl")
def _c_rollout_storage_rsl():
    from gennbv_amd.rsl_rl.storage import RolloutStorage
    t, n = 9, 5
    st = RolloutStorage(n, t, (4,), (None,), (2,), DEV)
    I = {"rewards": st.rewards, "values": st.values, "dones": st.dones, "lv": torch.empty(n, 1, device=DEV)}

    def mk(s):
        return {"rewards": _rand(s, t, n, 1), "values": _rand(s + 1, t, n, 1), "dones": _randint(s + 2, 0, 2, t, n, 1, dtype=torch.uint8),
                "lv": _rand(s + 3, n, 1)}
    A, D = mk(1), mk(50)
    O = {"returns": st.returns}

    def run():
        st.compute_returns(I["lv"], 0.99, 0.95)
        return {"advantages": st.advantages}
    return U.Live(I, A, D, O, _on(run), ["returns", "advantages"])


# wrappers that read a result back on the host by design (a boolean index, a count): no delayed protocol for them -- the stream would
# drain --, the handle and the result are checked (test_host_reading_wrappers_pass_the_callers_stream)
def _w_back_projection_fg():
    from gennbv_amd import utils
    from gennbv_amd.env import synthetic as S
    _, _, fr = _frames(2, 16, 30, 37)
    f = fr[0]
    ki = S.inverse_intrinsics(30, 37)
    return lambda: list(utils.back_projection_fg(f["depth"].clamp_min(-50.0), f["seg"], f["c2w"], ki))


def _w_bresenham3d():
    from gennbv_amd import utils
    s, t = _randint(1, 0, 16, 1, 3), _randint(2, -3, 19, 70, 3)
    return lambda: [utils.bresenham3D_hip(s, t, 16)]


def _w_scanned_pts_to_idx():
    from gennbv_amd import utils
    scene, _ = _mesh(2, 16)
    rg, vs = _dev(scene.range_gt), _dev(scene.voxel_size)
    pts = [_rand(1, 400, 3, lo=-6.0, hi=9.0), _rand(2, 300, 3, lo=-6.0, hi=9.0)]
    return lambda: [x for x in utils.scanned_pts_to_idx_3D(pts, rg, vs, 16) if isinstance(x, torch.Tensor)]


def _w_mesh_sweep_and_blocked():
    from gennbv_amd.env.collision import CollisionBody
    _, mesh = _mesh(2, 16)
    mesh.objects()
    body = CollisionBody(radius=0.3, half_length=0.1, ground=True, sweep=True)
    a, b = _scene_poses(1, 2, 1)[:, 0].contiguous(), _scene_poses(2, 2, 1)[:, 0].contiguous()
    lat = _lattice()
    return lambda: [mesh.sweep(a, b, body), mesh.flight_blocked(lat, body)]


def _w_scan_points():
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.eval.scan_accumulator import ScanAccumulator
    n, h, w = 2, 30, 37
    _, _, fr = _frames(n, 16, h, w)
    acc = ScanAccumulator(n, [_rand(7 + e, 300, 3, lo=-4.0, hi=6.0) for e in range(n)], h, w, S.inverse_intrinsics(h, w), -50.0,
                          capacity_per_env=2048, device=DEV)

    def run():
        acc.reset()
        acc.add_frame(fr[0]["depth"], fr[0]["seg"], fr[0]["c2w"])
        return [acc.points(0), acc.points(1)]
    return run


def _w_sample_and_log_prob():
    from gennbv_amd.sb3.distributions import MultiCategoricalDistribution
    dist = MultiCategoricalDistribution(HEADS)
    logits = _rand(1, 37, sum(HEADS), lo=-2.0, hi=2.0)
    return lambda: list(dist.sample_and_log_prob(logits, deterministic=True))


def _w_ground_truth():
    _, mesh = _mesh(2, 16)
    return lambda: [mesh.ground_truth(16).grid_gt]


HOST_READING = {"back_projection_fg": _w_back_projection_fg, "bresenham3D_hip": _w_bresenham3d, "scanned_pts_to_idx_3D": _w_scanned_pts_to_idx,
                "MeshScene.sweep/flight_blocked": _w_mesh_sweep_and_blocked, "ScanAccumulator.points": _w_scan_points,
                "sample_and_log_prob": _w_sample_and_log_prob, "MeshScene.ground_truth": _w_ground_truth}


# ================================================================================================================== the tests
class _Built:
    def __init__(self):
        self.live, self.error, self.vacuous, self.default_calls = {}, {}, {}, {}


@pytest.fixture(scope="module")
def built():
    """Every case built and run twice on the default stream (steps 1 and 2 of the protocol), with the recording proxy in place
    before any operator object exists; the delay comes from the slowest case's host time."""
    from gennbv_amd import _lib
    mp = pytest.MonkeyPatch()
    proxy = U.RecordingProxy(_lib.load())
    mp.setattr(_lib, "_lib", proxy)
    b = _Built()
    b.proxy = proxy
    U.side_stream()
    for name, (_, make) in CASES.items():
        try:
            live = make()
            torch.cuda.synchronize()
            proxy.clear()
            b.vacuous[name] = U.reference_runs(live)
            b.default_calls[name] = proxy.streams()
            print(f"[stream-order calls] {name}: {sorted({n for n, _ in b.default_calls[name]})}")
            b.live[name] = live
        except Exception as e:  # the case's own tests report it
            torch.cuda.synchronize()
            b.error[name] = e
    b.cal = U.delay_for([l.host_ms for l in b.live.values()] or [0.0])
    slow = max(b.live, key=lambda k: b.live[k].host_ms) if b.live else None
    print(f"[stream-order calibration] {b.cal} slowest case: {slow}")
    for k, l in b.live.items():
        print(f"[stream-order host ms] {k}: {l.host_ms:.3f}")
    yield b
    mp.undo()


def _self_test():
    side = U.side_stream()
    good, bad = U.fake_entry_point(False), U.fake_entry_point(True)
    assert U.reference_runs(good) == [] and U.reference_runs(bad) == []
    cal = U.delay_for([good.host_ms, bad.host_ms])
    print("[stream-order self-test]", cal, "pool streams passed over:", U._side["skipped"])
    assert U.run_protocol(good, side, cal["cycles"]) == []
    problems = U.run_protocol(bad, side, cal["cycles"])
    assert any("differs" in p for p in problems), problems
    assert not any("drained" in p for p in problems), problems


def test_harness_flags_a_launch_on_the_default_stream():
    """The harness's own test, on this machine: a fake entry point that issues one stage on stream 0 is flagged, the correct one
    passes -- the side stream is not ordered with stream 0 here, implicitly or through a shared hardware queue
    (stream_order_util.side_stream), and the delay is long enough."""
    _self_test()


def _live(built, name):
    if name in built.error:
        raise built.error[name]
    return built.live[name]


@pytest.mark.parametrize("name", list(CASES))
def test_c_layer_keeps_to_the_stream(built, name):
    live = _live(built, name)
    assert built.vacuous[name] == [], built.vacuous[name]
    built.proxy.clear()
    problems = U.run_protocol(live, U.side_stream(), built.cal["cycles"])
    live.side_calls = built.proxy.streams()
    assert problems == [], problems


@pytest.mark.parametrize("name", list(CASES))
def test_python_layer_passes_the_callers_stream(built, name):
    live = _live(built, name)
    side = U.side_stream()
    if not hasattr(live, "side_calls"):  # run alone: no delay needed for the handles
        built.proxy.clear()
        U.run_protocol(live, side, 1000)
        live.side_calls = built.proxy.streams()
    want, null = side.cuda_stream, torch.cuda.default_stream().cuda_stream
    assert want != null
    seen = {n for n, _ in live.side_calls}
    missing = set(CASES[name][0]) - seen
    assert not missing, f"the case did not call {sorted(missing)}"
    if name in FORKS:
        assert all(s != 0 for _, s in live.side_calls), live.side_calls
    else:
        assert all(s == want for _, s in live.side_calls), (hex(want), live.side_calls)
        assert all(s == null for _, s in built.default_calls[name]), built.default_calls[name]
    # a second call under the default stream AFTER the side-stream one: the default stream's handle again, the same result
    built.proxy.clear()
    got = U._enqueue(live, live.A, torch.cuda.default_stream())
    torch.cuda.synchronize()
    again = built.proxy.streams()
    assert again and (name in FORKS or all(s == null for _, s in again)), again
    for k in live.compare:
        assert U._same(live, got[k], live.R_A[k]), k


@pytest.mark.parametrize("name", list(HOST_READING))
def test_host_reading_wrappers_pass_the_callers_stream(monkeypatch, name):
    """The wrappers that synchronise by design: every library call they make carries the caller's stream, on a side stream and on the
    default stream afterwards, and the results agree."""
    proxy = U.install_proxy(monkeypatch)
    run = HOST_READING[name]()
    side, null = U.side_stream(), torch.cuda.default_stream()
    torch.cuda.synchronize()
    out = {}
    for stream in (side, null):
        proxy.clear()
        with torch.cuda.stream(stream):
            got = run()
        stream.synchronize()
        calls = proxy.streams()
        assert calls and all(h == stream.cuda_stream for _, h in calls), (hex(stream.cuda_stream), calls)
        out[stream] = [t.clone() for t in got]
    torch.cuda.synchronize()
    assert len(out[side]) == len(out[null]) > 0
    for a, b in zip(out[side], out[null]):
        assert torch.equal(a, b)


def test_harness_still_flags_a_launch_on_the_default_stream_at_the_end():
    """The same after every case has run: the side stream has not come to share a queue with stream 0 along the way."""
    _self_test()

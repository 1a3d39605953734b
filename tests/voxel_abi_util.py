"""Shared by tests/test_voxel_abi_gpu.py and tests/test_voxel_abi_regimes_cpu.py: frames whose geometry differs per env, the
launch geometry of csrc/voxel.hip and csrc/voxel_plan.h restated from their comments and constants, the CPU oracle run over a case, and device buffers the
test places itself (base, byte offset and row stride chosen by the test, the bytes around the rows filled with a sentinel).

Nothing here touches the GPU at import; only `Rows` and `VoxelCall` do."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from gennbv_amd.env import synthetic as S
from oracle import oracle as orc

DEV = "cuda:0"
f32 = np.float32
CLEAN = 1    # GNBV_VOXEL_WS_CLEAN
INVALID = 1  # hipErrorInvalidValue

# ---------------------------------------------------------------------------
# csrc/voxel.hip: constants and launch geometry (launch_masks and the kernels' own block -> work maps)
# ---------------------------------------------------------------------------
K_QUEUE_CAP = 4096          # kQueueCap: targets per k_raycast round
K_RAY_CHUNK_WORDS = 8192    # kRayChunkWords: mask words per k_raycast super-chunk
K_LIST_THREADS = 384        # kListThreads: rays per k_ray_list item
K_LIST_GRID_SLICES = 5      # kListGridSlices: k_ray_list workgroups per env on average
K_QUEUE_CAP_PX = 2048       # kQueueCapPx
K_LIST_SLICES = 16          # kListSlices: k_ray_slab slices per env and slab at most
K_WAVE = 64
LDS_MAX = 160 * 1024
GRID_STRIDE_THREADS = 2048 * 256  # grid_for(): at most 2048 blocks of 256 threads, grid-stride beyond


def mask_words(g):
    """mask_words_padded: words of one env's bitmask, a multiple of 64."""
    return (((g ** 3 + 31) // 32) + 63) & ~63


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def chunk_ranges(hw, chunks):
    """[px0, px1) of every image chunk, as k_hit_list / k_hit_atomic / k_hit_mask cut it (px1 < px0: an empty trailing chunk)."""
    ppc = (-(-hw // chunks) + 3) & ~3
    return [(c * ppc, min(hw, c * ppc + ppc)) for c in range(chunks)]


def slab_geometry(g, planes=0):
    """k_ray_slab: a slab is a run of whole x-planes of the path mask that starts on a word boundary and, where the grid allows it,
    holds at most 32 KiB of mask.  planes: GENNBV_VOXEL_SLAB_PLANES (0: by size), rounded up to the alignment."""
    gg = g * g
    align = 32 // math.gcd(gg, 32)                         # fewest planes whose bits fill whole words
    per = align * max(1, (32 * 1024 * 8) // (gg * align))  # aligned groups in 32 KiB, at least one
    if planes > 0:
        per = -(-planes // align) * align
    per = min(per, -(-g // align) * align)                 # (never more than the grid, rounded up to the alignment)
    slabs = -(-g // per)
    return SimpleNamespace(align=align, planes=per, slabs=slabs, lds=-(-per * gg // 32) * 4,
                           slices=_clamp(32 // slabs, 2, K_LIST_SLICES))  # ~32 workgroups per env, at least two per slab


def dispatch(n, g, h, w, full_ws, large=None, slab_planes=0):
    """Which kernels a call launches and with which geometry.  full_ws: the workspace has the h*w-sized ray lists;
    large: GENNBV_VOXEL_LARGE ("0", "1" or None); slab_planes: GENNBV_VOXEL_SLAB_PLANES."""
    words = mask_words(g)
    d = SimpleNamespace(n=n, g=g, words=words, env_groups=(n + 7) // 8)
    list_lds = words * 4 + 64 * 4 + ((words + 1) & ~1) * 2 + K_QUEUE_CAP_PX * 4
    if full_ws and list_lds <= LDS_MAX and words <= 65536 and large != "1":
        d.path = "list"       # k_hit_list + k_ray_list
    elif full_ws and large != "0" and slab_geometry(g, slab_planes).lds <= LDS_MAX:
        d.path = "large"      # k_hit_atomic + k_ray_slab
    else:
        d.path = "round1"     # k_hit_mask + k_raycast (also where no slab fits a workgroup's LDS)
    d.fchunks = _clamp(-(-512 // n), 1, 16)      # k_hit_list / k_hit_atomic workgroups per env
    d.chunks = _clamp(-(-2048 // n), 1, 16)      # k_hit_mask workgroups per env
    d.splits = _clamp(-(-1024 // n), 1, 8)       # k_raycast workgroups per env
    d.hit_windowed = words * 4 > LDS_MAX         # k_hit_mask<*, true>
    d.path_windowed = words * 4 + (K_QUEUE_CAP + 32) * 4 > LDS_MAX  # k_raycast<true, true>
    d.windowed = d.hit_windowed or d.path_windowed
    d.scan_passes = -(-d.env_groups // K_WAVE)   # k_ray_list: passes of the wave scan over one XCD's ray counts
    d.word_chunks = -(-words // K_RAY_CHUNK_WORDS)
    d.list_wgs_per_xcd = d.env_groups * K_LIST_GRID_SLICES
    d.hit_ranges = chunk_ranges(h * w, d.chunks if d.path == "round1" else d.fchunks)
    d.predictor = w % 4 == 0 and h * w < (1 << 23)  # (with a pinhole inv_intri; 16-byte requests)
    return d


def list_items_per_xcd(ray_counts):
    """k_ray_list work items per XCD: env e belongs to XCD e % 8 and has ceil(rays / 384) items."""
    items = -(-np.asarray(ray_counts, np.int64) // K_LIST_THREADS)
    return [int(items[x::8].sum()) for x in range(8)]


def raycast_rounds(hit_count, splits):
    """k_raycast queue rounds of the busiest split of an env with `hit_count` hit voxels in one word chunk."""
    return -(-(-(-hit_count // splits)) // K_QUEUE_CAP)


def grid_vec4(g3, tri_stride, *ptrs):
    """The fp32 / packed grid update takes its float4 kernel."""
    return g3 % 4 == 0 and tri_stride % 4 == 0 and all(p % 16 == 0 for p in ptrs)


def coded_vpl(g3, code_ptr, tri_ptr, tri_stride, tri8_ptr, tri8_stride):
    """Voxels per lane of k_grid_update_coded (0 for a NULL pointer)."""
    vec4 = (g3 % 4 == 0 and (tri_ptr == 0 or (tri_stride % 4 == 0 and tri_ptr % 16 == 0)) and code_ptr % 4 == 0
            and (tri8_ptr == 0 or (tri8_ptr | tri8_stride) % 4 == 0))
    vec16 = tri_ptr == 0 and g3 % 16 == 0 and code_ptr % 16 == 0 and (tri8_ptr | tri8_stride) % 16 == 0
    return 16 if vec16 else 4 if vec4 else 1


# ---------------------------------------------------------------------------
# inputs: every env has its own range, offset and anisotropy
# ---------------------------------------------------------------------------
def make_scene(n, g, seed, binary=True):
    rs = np.random.RandomState(seed)
    ext = rs.uniform(4.0, 12.0, (n, 3)).astype(f32)
    lo = (rs.uniform(-3.0, 3.0, (n, 3)).astype(f32) - ext * f32(0.5)).astype(f32)
    hi = (lo + ext).astype(f32)
    range_gt = np.stack([hi[:, 0], lo[:, 0], hi[:, 1], lo[:, 1], hi[:, 2], lo[:, 2]], -1).astype(f32)
    # voxel = extent / (g - 1) per axis in fp32, as the reference (env_train_gennbv.py:67-80)
    voxel = ((hi - lo) / f32(g - 1)).astype(f32)
    gt = rs.randint(0, 2, (n, g, g, g), dtype=np.uint8).astype(f32)
    if not binary:
        gt *= np.asarray([0.25, 0.4, 1.0, 0.75], f32)[rs.randint(0, 4, (n, g, g, g))]
    return SimpleNamespace(n=n, g=g, lo=lo, hi=hi, range_gt=range_gt, voxel_size=voxel, grid_gt=gt)


def make_frame(scene, h, w, seed, fg_share=0.7, outside_share=0.125, corner_envs=()):
    """Random depth per pixel, a seg mask with `fg_share` foreground (a scalar or one share per env), a camera somewhere in
    (an eighth: around) the env's grid looking at a point inside it.  corner_envs: the camera sits in a corner of the grid and
    looks at its centre, with depths that keep most points inside (as many distinct hit voxels as the pixels allow)."""
    n, rs = scene.n, np.random.RandomState(seed)
    ext = (scene.hi - scene.lo).astype(np.float64)
    cam = scene.lo + ext * rs.uniform(0.05, 0.95, (n, 3))
    out = rs.rand(n) < outside_share
    cam[out] = (scene.lo + ext * rs.uniform(-0.3, 1.3, (n, 3)))[out]
    tgt = scene.lo + ext * rs.uniform(0.2, 0.8, (n, 3))
    depth_scale = rs.uniform(0.05, 1.0, (n, h, w))
    for e in corner_envs:
        cam[e], tgt[e] = scene.lo[e] + 0.04 * ext[e], scene.lo[e] + 0.5 * ext[e]
        depth_scale[e] = rs.uniform(0.05, 0.5, (h, w))
    d = tgt - cam
    poses = np.zeros((n, 6), f32)
    poses[:, :3] = cam
    poses[:, 4] = np.arctan2(-d[:, 2], np.hypot(d[:, 0], d[:, 1]))
    poses[:, 5] = np.arctan2(d[:, 1], d[:, 0])
    c2w = S.camera_to_world(torch.from_numpy(poses)).float().numpy()
    diag = np.linalg.norm(ext, axis=1)
    depth = (-(depth_scale * diag[:, None, None])).astype(f32)  # raw depth: negative metres
    share = np.broadcast_to(np.asarray(fg_share, np.float64).reshape(-1, 1, 1), (n, 1, 1))
    seg = np.where(rs.rand(n, h, w) < share, f32(255.0), f32(0.0)).astype(f32)
    return SimpleNamespace(depth=depth, seg=seg, c2w=np.ascontiguousarray(c2w), poses=np.ascontiguousarray(poses[:, :3]))


def intrinsics(h, w, pinhole=True):
    kinv = S.inverse_intrinsics(h, w).numpy().astype(f32).copy()
    if not pinhole:  # skew terms: the generic chain (k_hit_list<false> / k_hit_mask<false> / k_hit_atomic<false>)
        kinv[0, 1] = 3e-4; kinv[1, 0] = -2e-4; kinv[2, 0] = 1e-6; kinv[2, 2] = 1.0009765625
    return kinv


def pack_bits(grid, g):
    """[N, G^3] != 0 -> [N, mask_words(G)] u32, bit v = voxel v."""
    n = grid.shape[0]
    bits = np.packbits(grid.reshape(n, -1) != 0, axis=1, bitorder="little")
    out = np.zeros((n, mask_words(g) * 4), np.uint8)
    out[:, :bits.shape[1]] = bits
    return out.view(np.uint32)


def pixel_voxels(scene, frame, kinv):
    """Linear voxel index of every pixel by the oracle's canonical chain, -1 for a pixel that hits nothing: [N, h*w]."""
    dp, sp = orc.post_process_depth(frame.depth, frame.seg)
    world, fg = orc.back_projection(dp, sp, frame.c2w, kinv)
    idx = orc.points_to_idx(world, fg, scene.range_gt, scene.voxel_size, scene.g).astype(np.int64)
    lin = (idx[..., 0] * scene.g + idx[..., 1]) * scene.g + idx[..., 2]
    return np.where(idx[..., 0] >= 0, lin, -1)


def list_ray_counts(lin, ranges):
    """Entries of every env's ray list: one per distinct voxel and image chunk."""
    cnt = np.zeros(lin.shape[0], np.int64)
    for p0, p1 in ranges:
        if p1 > p0:
            for e in range(lin.shape[0]):
                v = lin[e, p0:p1]
                cnt[e] += np.unique(v[v >= 0]).size
    return cnt


# ---------------------------------------------------------------------------
# a case = scene + frames + reset masks; its reference = the oracle's outputs after every call
# ---------------------------------------------------------------------------
def make_case(n, g, h, w, steps=3, seed=0, fg_share=0.7, binary=True, pinhole=True, reset_at=(1,), outside_share=0.125, twins=False, corner_envs=()):
    scene = make_scene(n, g, 1000 + seed, binary)
    frames = [make_frame(scene, h, w, 2000 + 17 * seed + s, fg_share, outside_share, corner_envs) for s in range(steps)]
    if twins:  # envs 0 and 1: the same images, camera matrix and pose in every frame -- only range_gt / voxel_size differ
        scene.lo[1] = scene.lo[0] + np.asarray([0.37, -0.21, 0.55], f32)
        scene.hi[1] = scene.hi[0] + np.asarray([1.9, 0.8, -0.7], f32)
        lo, hi = scene.lo, scene.hi
        scene.range_gt = np.stack([hi[:, 0], lo[:, 0], hi[:, 1], lo[:, 1], hi[:, 2], lo[:, 2]], -1).astype(f32)
        scene.voxel_size = ((hi - lo) / f32(g - 1)).astype(f32)
        for f in frames:
            f.depth[1], f.seg[1], f.c2w[1], f.poses[1] = f.depth[0], f.seg[0], f.c2w[0], f.poses[0]
    rs = np.random.RandomState(3000 + seed)
    resets = []
    for s in range(steps):
        r = None
        if s in reset_at:
            r = (rs.rand(n) < 0.5).astype(np.uint8)
            r[0] = 1
            r[-1] = 0 if n > 1 else 1
        resets.append(r)
    return SimpleNamespace(n=n, g=g, h=h, w=w, scene=scene, frames=frames, resets=resets, kinv=intrinsics(h, w, pinhole), pinhole=pinhole)


def run_oracle(case):
    """The oracle's state after every call: prob / scan / tri [N, G^3] f32, coverage, hit / path [N, G^3] bool."""
    n, g, sc = case.n, case.g, case.scene
    prob = np.zeros((n, g, g, g), f32)
    scan = np.zeros_like(prob)
    out = []
    for f, r in zip(case.frames, case.resets):
        dp, sp = orc.post_process_depth(f.depth, f.seg)
        tri, cov, hit, path = orc.update_occ_grid(dp, sp, f.c2w, case.kinv, f.poses, sc.range_gt, sc.voxel_size, sc.grid_gt, prob, scan,
                                                  reset_mask=r, return_masks=True)
        # (kept compactly -- a case has up to 2048 envs: the tri classes are -1 / 0 / 1, the scanned set of a binary GT 0 / 1)
        binary = bool(np.isin(scan, (0.0, 1.0)).all())
        out.append(SimpleNamespace(prob=prob.reshape(n, -1).copy(), scan=scan.reshape(n, -1).astype(np.uint8 if binary else f32),
                                   tri=tri.reshape(n, -1).astype(np.int8), cov=cov, hit=hit.reshape(n, -1), path=path.reshape(n, -1)))
    return out


def assert_masks_not_vacuous(ref):
    """Every call of the case sets hit voxels and strictly more path voxels."""
    for s, o in enumerate(ref):
        assert o.hit.sum() > 0 and o.path.sum() > o.hit.sum(), s


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
FILL = 0x5B  # sentinel byte around every buffer the test places (0x5B5B5B5B is 6.2e16 as fp32, 91 as int8: no kernel output)


class Rows:
    """rows x cols elements of `dtype` inside a sentinel-filled device arena: row r starts `offset` bytes + r * stride elements behind
    a 256-byte aligned base."""

    def __init__(self, rows, cols, dtype, stride=None, offset=0, init=None):
        self.rows, self.cols, self.dtype = rows, cols, np.dtype(dtype)
        self.stride = cols if stride is None else stride
        self.offset = offset
        self.span = ((rows - 1) * self.stride + cols) * self.dtype.itemsize
        self.arena = torch.full((offset + self.span + 256 + 64,), FILL, dtype=torch.uint8, device=DEV)
        self.base = (-self.arena.data_ptr()) % 256
        self.ptr = self.arena.data_ptr() + self.base + offset
        self.row_bytes = self.stride * self.dtype.itemsize
        self.write(np.zeros((rows, cols), self.dtype) if init is None else init)

    def _rows_of(self, buf):
        lo = self.base + self.offset
        flat = np.zeros(self.rows * self.row_bytes, np.uint8)
        flat[:self.span] = buf[lo:lo + self.span]
        return flat.view(self.dtype).reshape(self.rows, self.stride)[:, :self.cols]

    def write(self, a):
        a = np.ascontiguousarray(a, self.dtype).reshape(self.rows, self.cols)
        buf = self.arena.cpu().numpy()
        lo = self.base + self.offset
        flat = np.full(self.rows * self.row_bytes, FILL, np.uint8)
        flat[:self.span] = buf[lo:lo + self.span]
        flat.view(self.dtype).reshape(self.rows, self.stride)[:, :self.cols] = a
        buf[lo:lo + self.span] = flat[:self.span]
        self.arena.copy_(torch.from_numpy(buf))

    def read(self):
        return np.ascontiguousarray(self._rows_of(self.arena.cpu().numpy()))

    def padding_intact(self):
        """The bytes in front of, between and behind the rows still hold the sentinel."""
        buf = self.arena.cpu().numpy()
        lo = self.base + self.offset
        flat = np.full(self.rows * self.row_bytes, FILL, np.uint8)
        flat[:self.span] = buf[lo:lo + self.span]
        flat.view(self.dtype).reshape(self.rows, self.stride)[:, :self.cols] = np.frombuffer(bytes([FILL]) * self.dtype.itemsize, self.dtype)[0]
        buf[lo:lo + self.span] = flat[:self.span]
        return bool((buf == FILL).all())

    def snapshot(self):
        return self.arena.cpu().numpy().tobytes()


def libs():
    from gennbv_amd import _lib as L
    return L, L.load()


F32_ARGS = ("depth_raw", "seg_raw", "c2w", "inv_intri", "poses_xyz", "poses_row_stride", "range_gt", "voxel_size", "grid_gt", "reset_mask",
            "n", "h", "w", "g", "depth_sense_dist", "prob_grid", "scanned_gt_grid", "tri_out", "tri_row_stride", "coverage_count",
            "workspace", "workspace_bytes", "stream")
PACKED_ARGS = tuple({"grid_gt": "gt_bits", "scanned_gt_grid": "scanned_bits"}.get(a, a) for a in F32_ARGS)
CODED_ARGS = ("depth_raw", "seg_raw", "c2w", "inv_intri", "poses_xyz", "poses_row_stride", "range_gt", "voxel_size", "gt_bits", "reset_mask",
              "n", "h", "w", "g", "depth_sense_dist", "prob_code", "tri_lut", "scanned_bits", "tri_out", "tri_row_stride", "tri_i8",
              "tri_i8_row_stride", "coverage_count", "overflow", "workspace", "workspace_bytes", "workspace_flags", "stream")
ENTRY = {"f32": ("gnbv_update_occ_grid", F32_ARGS), "packed": ("gnbv_update_occ_grid_packed", PACKED_ARGS),
         "coded": ("gnbv_update_occ_grid_coded", CODED_ARGS)}


class VoxelCall:
    """One entry point with buffers the test owns.  `kind`: f32 / packed / coded.  Layout keywords (bytes unless noted):
    tri_off, prob_off (prob_grid / prob_code), scan_off, gt_off, tri8_off, ws_off, depth_off (depth_raw and seg_raw),
    tri_stride / tri8_stride / pose_stride (elements), use_tri / use_tri8 / use_overflow (coded), tri_lut (a replacement table),
    full_ws (False: the mask-only workspace)."""

    def __init__(self, kind, case, full_ws=True, tri_off=0, prob_off=0, scan_off=0, gt_off=0, tri8_off=0, ws_off=0, depth_off=0,
                 tri_stride=None, tri8_stride=None, pose_stride=3, use_tri=None, use_tri8=None, use_overflow=True, tri_lut=None):
        self.L, self.lib = libs()
        self.kind, self.case = kind, case
        n, g, h, w, sc = case.n, case.g, case.h, case.w, case.scene
        self.g3 = g3 = g ** 3
        words = mask_words(g)
        coded = kind == "coded"
        self.use_tri = (not coded) if use_tri is None else use_tri
        self.use_tri8 = coded if use_tri8 is None else use_tri8
        self.pose_stride = pose_stride
        self.depth = Rows(n, h * w, f32, offset=depth_off)
        self.seg = Rows(n, h * w, f32, offset=depth_off)
        self.c2w = Rows(n, 16, f32)
        self.poses = Rows(n, 3, f32, stride=pose_stride)
        self.range_gt = Rows(n, 6, f32, init=sc.range_gt)
        self.voxel = Rows(n, 3, f32, init=sc.voxel_size)
        self.kinv = (C.c_float * 9)(*case.kinv.reshape(-1).tolist())
        self.reset = Rows(1, n, np.uint8)
        self.cov = Rows(1, n, np.int32, init=np.full(n, -77, np.int32))
        self.tri = Rows(n, g3, f32, stride=tri_stride or g3, offset=tri_off, init=np.full((n, g3), 7.0, f32)) if self.use_tri else None
        if kind == "f32":
            self.gt = Rows(n, g3, f32, offset=gt_off, init=sc.grid_gt)
            self.scan = Rows(n, g3, f32, offset=scan_off)
            self.prob = Rows(n, g3, f32, offset=prob_off)
        else:
            self.gt = Rows(n, words, np.uint32, offset=gt_off, init=pack_bits(sc.grid_gt, g))
            self.scan = Rows(n, words, np.uint32, offset=scan_off)
            self.prob = Rows(n, g3, np.uint8 if coded else f32, offset=prob_off)
        if coded:
            pl, tl = (C.c_float * 256)(), (C.c_float * 256)()
            self.lib.gnbv_prob_code_tables(pl, tl)
            self.prob_lut = np.asarray(pl[:], f32)
            self.tri_lut_host = np.asarray(tl[:], f32) if tri_lut is None else np.asarray(tri_lut, f32)
            self.prob_lut_dev = Rows(1, 256, f32, init=self.prob_lut)
            self.tri_lut = Rows(1, 256, f32, init=self.tri_lut_host)
            self.tri8 = Rows(n, g3, np.int8, stride=tri8_stride or g3, offset=tri8_off, init=np.full((n, g3), 99, np.int8)) if self.use_tri8 else None
            self.overflow = Rows(1, 1, np.int32) if use_overflow else None
        self.ws_bytes = int(self.lib.gnbv_voxel_workspace_bytes_hw(n, g, h, w) if full_ws else self.lib.gnbv_voxel_workspace_bytes(n, g))
        assert self.ws_bytes >= 2 * n * words * 4 and (full_ws or self.ws_bytes == 2 * n * words * 4)
        self.ws = Rows(1, self.ws_bytes, np.uint8, offset=ws_off)

    def load(self, frame, reset):
        self.depth.write(frame.depth)
        self.seg.write(frame.seg)
        self.c2w.write(frame.c2w)
        self.poses.write(frame.poses)
        if reset is not None:
            self.reset.write(reset)

    def args(self, reset=None, flags=0):
        c, p = self.case, (lambda r: None if r is None else r.ptr)
        a = dict(depth_raw=self.depth.ptr, seg_raw=self.seg.ptr, c2w=self.c2w.ptr, inv_intri=C.addressof(self.kinv), poses_xyz=self.poses.ptr,
                 poses_row_stride=self.pose_stride, range_gt=self.range_gt.ptr, voxel_size=self.voxel.ptr,
                 reset_mask=None if reset is None else self.reset.ptr, n=c.n, h=c.h, w=c.w, g=c.g, depth_sense_dist=-50.0,
                 tri_out=p(self.tri), tri_row_stride=self.tri.stride if self.tri else 0, coverage_count=self.cov.ptr,
                 workspace=self.ws.ptr, workspace_bytes=self.ws_bytes, stream=None)
        if self.kind == "f32":
            a.update(grid_gt=self.gt.ptr, prob_grid=self.prob.ptr, scanned_gt_grid=self.scan.ptr)
        elif self.kind == "packed":
            a.update(gt_bits=self.gt.ptr, prob_grid=self.prob.ptr, scanned_bits=self.scan.ptr)
        else:
            a.update(gt_bits=self.gt.ptr, prob_code=self.prob.ptr, scanned_bits=self.scan.ptr, tri_lut=self.tri_lut.ptr, tri_i8=p(self.tri8),
                     tri_i8_row_stride=self.tri8.stride if self.tri8 else 0, overflow=p(self.overflow), workspace_flags=flags)
        return a

    def call(self, a):
        name, order = ENTRY[self.kind]
        err = getattr(self.lib, name)(*[a[k] for k in order])
        torch.cuda.synchronize()
        return err

    def step(self, s, flags=0):
        """Call number s of the case; returns the error code."""
        self.load(self.case.frames[s], self.case.resets[s])
        return self.call(self.args(self.case.resets[s], flags))

    # ---- outputs, in the oracle's terms ----
    def outputs(self, masks=True):
        n, g, lib, chk = self.case.n, self.case.g, self.lib, self.L.check
        o = SimpleNamespace(cov=self.cov.read().reshape(-1), tri=None, tri8=None, hit=None, path=None)
        if self.kind == "coded":
            o.code = self.prob.read()
            dec = torch.empty(n * self.g3, dtype=torch.float32, device=DEV)
            chk(lib.gnbv_decode_prob_grid(self.prob.ptr, n * self.g3, self.prob_lut_dev.ptr, dec.data_ptr(), None), "decode")
            o.prob = dec.cpu().numpy().reshape(n, -1)
            o.tri8 = None if self.tri8 is None else self.tri8.read()
            o.overflow = None if self.overflow is None else int(self.overflow.read()[0, 0])
        else:
            o.prob = self.prob.read()
        if self.kind == "f32":
            o.scan = self.scan.read()
        else:
            bits = torch.from_numpy(self.scan.read().view(np.int32)).to(DEV)  # (a dense copy: gnbv_unpack_grid_bits has no offset)
            sc = torch.empty(n * self.g3, dtype=torch.float32, device=DEV)
            chk(lib.gnbv_unpack_grid_bits(bits.data_ptr(), n, g, sc.data_ptr(), None), "unpack_grid_bits")
            o.scan = sc.cpu().numpy().reshape(n, -1)
        if self.tri is not None:
            o.tri = self.tri.read()
        if masks:
            hm = torch.empty(n * self.g3, dtype=torch.uint8, device=DEV)
            pm = torch.empty_like(hm)
            chk(lib.gnbv_unpack_masks(self.ws.ptr, n, g, hm.data_ptr(), pm.data_ptr(), None), "unpack_masks")
            o.hit, o.path = hm.cpu().numpy().reshape(n, -1).astype(bool), pm.cpu().numpy().reshape(n, -1).astype(bool)
        return o

    def padding_intact(self):
        bufs = [self.prob, self.scan, self.gt, self.cov, self.tri, self.ws, self.depth, self.seg, self.poses]
        if self.kind == "coded":
            bufs += [self.tri8, self.overflow, self.tri_lut]
        return all(b.padding_intact() for b in bufs if b is not None)

    def snapshot(self):
        """Every buffer a call may write, as bytes."""
        bufs = [self.prob, self.scan, self.cov, self.tri, self.ws]
        if self.kind == "coded":
            bufs += [self.tri8, self.overflow]
        return [b.snapshot() for b in bufs if b is not None]


def _same(name, got, want, where):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (where, name, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
        raise AssertionError(f"{where}: {name} differs at {bad.size} places, first {bad[:6].tolist()}: got {got.reshape(-1)[bad[:6]].tolist()} "
                             f"want {want.reshape(-1)[bad[:6]].tolist()}")


def compare(call, o, ref, where, masks=True):
    """Every output of one call against the oracle's state `ref`, as bytes."""
    ref = SimpleNamespace(prob=ref.prob, scan=ref.scan.astype(f32), tri=ref.tri.astype(f32), cov=ref.cov, hit=ref.hit, path=ref.path)
    _same("prob", o.prob, ref.prob, where)
    _same("scanned", o.scan, ref.scan, where)
    _same("coverage", o.cov, ref.cov, where)
    if call.kind == "coded":
        _same("prob_lut[code]", call.prob_lut[o.code], ref.prob, where)
        default_lut = call.tri_lut_host.tobytes() == ((call.prob_lut > 0.5).astype(f32) - (call.prob_lut < 0).astype(f32)).tobytes()
        tri_ref = ref.tri if default_lut else call.tri_lut_host[o.code]
        if default_lut:
            _same("tri_lut[code]", call.tri_lut_host[o.code], ref.tri, where)
        if o.tri8 is not None:
            _same("tri_i8", o.tri8, tri_ref.astype(np.int8), where)
    else:
        tri_ref = ref.tri
    if o.tri is not None:
        _same("tri", o.tri, tri_ref, where)
    if masks:
        _same("hit mask", o.hit, ref.hit, where)
        _same("path mask", o.path, ref.path, where)
    assert call.padding_intact(), f"{where}: bytes outside the rows were written"


def same_outputs(a, b, where):
    for k in ("prob", "scan", "cov", "tri", "tri8", "hit", "path"):
        x, y = getattr(a, k, None), getattr(b, k, None)
        if x is not None and y is not None:
            _same(k, x, y, where)


cached = functools.lru_cache(maxsize=None)


# ---------------------------------------------------------------------------
# launch-regime cases: id -> (entry point, make_case arguments, workspaces to run, GENNBV_VOXEL_LARGE, regime check)
# G = 16 and tiny images (8x12: the predictor stream, w % 4 == 0; 7x9: the per-pixel canonical loop) unless the regime needs more.
# ---------------------------------------------------------------------------
def _every_third_blank(n):
    return np.where(np.arange(n) % 3 == 0, 0.0, 0.8)


def _one_loaded_env(n, e=5):
    s = np.full(n, 0.01)
    s[e] = 1.0
    return s


LAUNCH_CASES = {
    # ---- list path: k_hit_list + k_ray_list (full workspace, G <= 104) ----
    "list-n1-16chunks": ("f32", dict(n=1, g=16, h=24, w=32, binary=False), "list_n1"),
    "list-n100-fchunks6": ("packed", dict(n=100, g=16, h=7, w=9), "list_fchunks_not_pow2"),
    "list-n512-one-scan-pass": ("coded", dict(n=512, g=16, h=8, w=12, steps=4), "list_n512"),
    "list-n513-two-scan-passes": ("coded", dict(n=513, g=16, h=8, w=12, steps=4), "list_n513"),
    "list-n1027-three-scan-passes": ("coded", dict(n=1027, g=16, h=7, w=9, steps=4), "list_n1027"),
    "list-n2-8x12-empty-trailing-chunks": ("coded", dict(n=2, g=16, h=8, w=12, steps=4), "list_empty_chunks"),
    "list-n2-several-items-per-workgroup": ("packed", dict(n=2, g=24, h=128, w=160, fg_share=1.0, outside_share=0.0), "list_several_items"),
    "list-n600-empty-ray-lists-interleaved": ("coded", dict(n=600, g=16, h=8, w=12, steps=4, fg_share=_every_third_blank(600)), "list_empty_lists"),
    # ---- round-1 kernels: k_hit_mask + k_raycast (mask-only workspace); every one also runs on the full workspace ----
    "round1-g16-n3-splits8": ("f32", dict(n=3, g=16, h=8, w=12, binary=False), "r1_splits8"),
    "round1-g33-n180-splits6-generic-chain": ("coded", dict(n=180, g=33, h=7, w=9, pinhole=False), "r1_splits_not_pow2"),
    "round1-g72-n2-second-word-chunk": ("packed", dict(n=2, g=72, h=24, w=32, fg_share=1.0, outside_share=0.0), "r1_two_word_chunks"),
    "round1-g16-n1024-splits1": ("coded", dict(n=1024, g=16, h=8, w=12), "r1_splits1"),
    "round1-g16-n2048-hit-chunks1": ("coded", dict(n=2048, g=16, h=7, w=9), "r1_chunks1"),
    "round1-g32-n1024-two-queue-rounds": ("coded", dict(n=1024, g=32, h=80, w=120, steps=2, fg_share=_one_loaded_env(1024), outside_share=0.0, corner_envs=(5,)),
                                          "r1_queue_rounds"),
    # ---- large-grid kernels forced at G = 16: k_hit_atomic + k_ray_slab ----
    "large-g16-n520-own-env": ("coded", dict(n=520, g=16, h=8, w=12, steps=4), "large_own_env"),
    "large-g16-n3": ("coded", dict(n=3, g=16, h=8, w=12, steps=4), "large_small_n"),
}


@cached
def launch_case(cid):
    """(case, oracle outputs per call) of a launch-regime case, computed once."""
    case = make_case(seed=sorted(LAUNCH_CASES).index(cid), **LAUNCH_CASES[cid][1])
    return case, run_oracle(case)


def workspaces_of(cid):
    """(full_ws, GENNBV_VOXEL_LARGE) of every run of the case."""
    if cid.startswith("list-"):
        return [(True, None)]
    if cid.startswith("large-"):
        return [(True, "1")]
    return [(False, None), (True, None)]


def check_regime(cid):
    """The case reaches the branch its id names -- from n, the shapes and the ORACLE's masks; returns the figures it used."""
    kind, kw, regime = LAUNCH_CASES[cid]
    case, ref = launch_case(cid)
    n, g, h, w, hw = case.n, case.g, case.h, case.w, case.h * case.w
    assert_masks_not_vacuous(ref)
    full_ws, large = workspaces_of(cid)[0]
    d = dispatch(n, g, h, w, full_ws, large)
    hits = np.stack([o.hit.sum(1) for o in ref])  # [steps, n] distinct hit voxels
    info = dict(path=d.path, fchunks=d.fchunks, chunks=d.chunks, splits=d.splits, env_groups=d.env_groups, words=d.words, max_hits=int(hits.max()))
    empty = [r for r in d.hit_ranges if r[0] >= hw]
    if regime.startswith("list_"):
        assert d.path == "list" and dispatch(n, g, h, w, False).path == "round1"
        lin = [pixel_voxels(case.scene, f, case.kinv) for f in case.frames]
        rays = np.stack([list_ray_counts(l, d.hit_ranges) for l in lin])  # [steps, n] ray-list entries
        for s, l in enumerate(lin):  # (the per-pixel chain and the oracle's update agree on the hit set)
            for e in range(min(n, 4)):
                assert np.array_equal(np.unique(l[e][l[e] >= 0]), np.nonzero(ref[s].hit[e])[0])
        info.update(max_rays=int(rays.max()), mean_rays=float(rays.mean()))
    if regime == "list_n1":
        assert n == 1 and d.fchunks == 16 and not empty and d.predictor
    elif regime == "list_fchunks_not_pow2":
        assert d.fchunks > 1 and d.fchunks & (d.fchunks - 1) and not d.predictor  # (7x9: the canonical per-pixel loop)
    elif regime == "list_n512":
        assert n == 512 and d.fchunks == 1 and d.env_groups == 64 and d.scan_passes == 1
    elif regime == "list_n513":
        assert d.fchunks == 1 and d.env_groups == 65 and d.scan_passes == 2
        assert (rays[:, 512] > 0).all()  # the env of the second pass has rays
    elif regime == "list_n1027":
        assert d.fchunks == 1 and n % 8 and d.scan_passes == 3 and (rays[:, 1024:] > 0).any()
    elif regime == "list_empty_chunks":
        assert d.fchunks == 16 and d.predictor and len(empty) >= 2 and any(p1 < p0 for p0, p1 in d.hit_ranges)
    elif regime == "list_several_items":
        items = [list_items_per_xcd(r) for r in rays]
        info.update(items_per_xcd=items, workgroups_per_xcd=d.list_wgs_per_xcd)
        assert all(max(i) > d.list_wgs_per_xcd for i in items) and (rays.mean(1) > K_LIST_GRID_SLICES * K_LIST_THREADS).all()
    elif regime == "list_empty_lists":
        assert n > 512 and d.scan_passes == 2
        for r in rays:  # an env without rays between two envs of the same XCD that have some, in both scan passes
            mid = [e for e in range(8, n - 8) if r[e] == 0 and r[e - 8] > 0 and r[e + 8] > 0]
            assert any(e < 512 for e in mid) and any(e >= 512 for e in mid)
    if regime.startswith("r1_"):
        assert d.path == "round1" and not d.windowed and dispatch(n, g, h, w, True).path == "list"
    if regime == "r1_splits8":
        assert d.splits == 8 and d.chunks == 16 and d.predictor and empty
    elif regime == "r1_splits_not_pow2":
        assert d.splits & (d.splits - 1) and d.splits > 1 and not case.pinhole and g ** 3 % 4
    elif regime == "r1_two_word_chunks":
        assert 65 <= g <= 104 and d.word_chunks == 2
        lo_hi = [(int(o.hit[:, :K_RAY_CHUNK_WORDS * 32].sum()), int(o.hit[:, K_RAY_CHUNK_WORDS * 32:].sum())) for o in ref]
        info.update(hits_per_word_chunk=lo_hi)
        assert all(a > 0 and b > 0 for a, b in lo_hi)
    elif regime == "r1_splits1":
        assert n == 1024 and d.splits == 1 and d.chunks == 2
    elif regime == "r1_chunks1":
        assert n == 2048 and d.chunks == 1 and d.splits == 1
    elif regime == "r1_queue_rounds":
        assert n == 1024 and d.splits == 1 and d.word_chunks == 1
        assert (hits.max(1) > K_QUEUE_CAP).all() and all(raycast_rounds(int(m), 1) >= 2 for m in hits.max(1))
        info.update(hits_of_loaded_env=hits.max(1).tolist(), median_hits=float(np.median(hits)))
    if regime.startswith("large_"):
        assert d.path == "large"
        assert (d.fchunks == 1 and n > 512) if regime == "large_own_env" else d.fchunks == 16
    return info

"""Shared by tests/test_voxel_ops_cpu.py and tests/test_voxel_ops_abi_gpu.py: references of the function-granular voxel operators and
bit packers of include/gennbv_hip.h, written from the header's contract in plain numpy (oracle/oracle.c mirrors the kernels' arithmetic,
so the two could share a mistake), and the inputs of every case of the two files.

numpy fp32 rounds every elementwise operation once: the clamp, the voxel frame, the quotient, floor and the strict bounds below are the
kernels' _rn chains.  The bits are integer numpy, the line walk is plain Python.  NaN, inf and |q| >= 1e9 are masked before any
astype(int): nothing here rests on how the host converts them.  Nothing here touches the GPU."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import voxel_abi_util as U

f32 = np.float32
FLT_MAX = np.finfo(f32).max
DENORMAL = f32(1e-40)
EPS = 2.0 ** -24  # unit round-off of fp32
cached = functools.lru_cache(maxsize=None)


def bits_of(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def bitset(a):
    return set(bits_of(a).reshape(-1).tolist())


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def nan_to_num_neginf0(x):
    """torch.nan_to_num(x, neginf=0): NaN -> 0, +inf -> FLT_MAX, -inf -> 0, every other bit pattern kept."""
    x = np.asarray(x, f32)
    out = x.copy()
    out[np.isnan(x)] = f32(0.0)
    out[x == np.inf] = FLT_MAX
    out[x == -np.inf] = f32(0.0)
    return out


def post_process_depth(depth_raw, seg_raw, sense):
    """depth = |max(nan_to_num(depth_raw), sense)|, seg = nan_to_num(seg_raw)."""
    return np.abs(np.maximum(nan_to_num_neginf0(depth_raw), f32(sense))), nan_to_num_neginf0(seg_raw)


def voxel_frame(range_gt, voxel_size):
    """(vmin, vmax) [N, 3]: range_min - 0.5 v and range_max + 0.5 v in fp32."""
    r, v = np.asarray(range_gt, f32), np.asarray(voxel_size, f32)
    half = f32(0.5) * v
    return r[:, 1::2] - half, r[:, 0::2] + half


def _floor_to_int(fl):
    """floor values -> int64; NaN, inf and |fl| >= 1e9 give 0 (the caller clamps or has excluded them)."""
    ok = np.isfinite(fl) & (np.abs(np.where(np.isfinite(fl), fl, 0)) < 1e9)
    out = np.zeros(fl.shape, np.int64)
    out[ok] = fl[ok].astype(np.int64)
    return out


def points_to_idx(world, fg, range_gt, voxel_size, g):
    """[N, P, 3] int32: floor((p - vmin) / v) clamped to [0, g - 1] for a foreground point strictly inside (vmin, vmax) on every axis,
    (-1, -1, -1) otherwise."""
    world = np.asarray(world, f32)
    vmin, vmax = voxel_frame(range_gt, voxel_size)
    v = np.asarray(voxel_size, f32)[:, None, :]
    with np.errstate(all="ignore"):
        fl = np.floor((world - vmin[:, None, :]) / v)
        keep = ((vmax[:, None, :] > world) & (world > vmin[:, None, :])).all(-1) & (np.asarray(fg) != 0)
    i = np.clip(_floor_to_int(fl), 0, g - 1)
    return np.where(keep[..., None], i, -1).astype(np.int32)


def pose_quotient(poses, range_gt, voxel_size):
    vmin, _ = voxel_frame(range_gt, voxel_size)
    return (np.asarray(poses, f32) - vmin) / np.asarray(voxel_size, f32)


def pose_to_idx(poses, range_gt, voxel_size):
    """[N, 3] int64: floor((p - vmin) / v), no clamp, no bounds (poses are finite and |q| < 2^31)."""
    fl = np.floor(pose_quotient(poses, range_gt, voxel_size))
    assert np.isfinite(fl).all() and (np.abs(fl) < 2.0 ** 31).all()
    return fl.astype(np.int64)


def bresenham_ray(src, tgt, g):
    """The classic driving-axis integer 3-D Bresenham from src to tgt, both ends included; the driving axis is the first of x, y, z
    with the largest |delta|; only voxels inside [0, g)^3 are emitted."""
    x, y, z = (int(c) for c in src)
    x1, y1, z1 = (int(c) for c in tgt)
    dx, dy, dz = abs(x1 - x), abs(y1 - y), abs(z1 - z)
    xs, ys, zs = (1 if x1 > x else -1), (1 if y1 > y else -1), (1 if z1 > z else -1)
    pts = []

    def emit():
        if 0 <= x < g and 0 <= y < g and 0 <= z < g:
            pts.append((x, y, z))
    emit()
    if dx >= dy and dx >= dz:
        p1, p2 = 2 * dy - dx, 2 * dz - dx
        while x != x1:
            x += xs
            if p1 >= 0:
                y += ys
                p1 -= 2 * dx
            if p2 >= 0:
                z += zs
                p2 -= 2 * dx
            p1 += 2 * dy
            p2 += 2 * dz
            emit()
    elif dy >= dz:
        p1, p2 = 2 * dx - dy, 2 * dz - dy
        while y != y1:
            y += ys
            if p1 >= 0:
                x += xs
                p1 -= 2 * dy
            if p2 >= 0:
                z += zs
                p2 -= 2 * dy
            p1 += 2 * dx
            p2 += 2 * dz
            emit()
    else:
        p1, p2 = 2 * dx - dz, 2 * dy - dz
        while z != z1:
            z += zs
            if p1 >= 0:
                x += xs
                p1 -= 2 * dz
            if p2 >= 0:
                y += ys
                p2 -= 2 * dz
            p1 += 2 * dx
            p2 += 2 * dy
            emit()
    return pts


def bresenham3d(src, targets, g, fill):
    """(trajectory_pts [R, 3g, 3], trajectory_lengths [R]) int32 as gnbv_bresenham3d leaves buffers prefilled with `fill`."""
    targets = np.asarray(targets, np.int64).reshape(-1, 3)
    traj = np.full((targets.shape[0], 3 * g, 3), fill, np.int32)
    lens = np.zeros(targets.shape[0], np.int32)
    for r, t in enumerate(targets):
        pts = bresenham_ray(src, t, g)
        lens[r] = len(pts)
        if pts:
            traj[r, :len(pts)] = pts
    return traj, lens


def pack_bits(grid, g):
    """[N, g^3] floats -> [N, mask_words(g)] u32: bit v & 31 of word v >> 5 is (x != 0); every other bit zero."""
    n, words = grid.shape[0], U.mask_words(g)
    b = np.zeros((n, words * 32), np.uint32)
    b[:, :g ** 3] = np.asarray(grid, f32).reshape(n, -1) != 0
    return (b.reshape(n, words, 32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint64).astype(np.uint32)


def not_binary(grid):
    x = np.asarray(grid, f32)
    return int(((x != 0) & (x != 1)).any())


def unpack_bits(words, g, dtype=f32):
    """[N, words] u32 -> [N, g^3] of 0 / 1."""
    v = np.arange(g ** 3)
    return ((np.asarray(words, np.uint32)[:, v >> 5] >> (v & 31).astype(np.uint32)) & np.uint32(1)).astype(dtype)


def prob_code_tables():
    """prob_lut[base << 7 | k] = base after k fp32 steps x <- x - 0.05f; tri_lut = (prob > 0.5) - (prob < 0)."""
    prob = np.zeros(256, f32)
    for base in (0, 1):
        x = f32(base)
        for k in range(128):
            prob[base * 128 + k] = x
            x = f32(x - f32(0.05))
    return prob, (prob > f32(0.5)).astype(f32) - (prob < f32(0.0)).astype(f32)


def back_projection_f64(depth, seg, c2w, kinv):
    """(world [N, HW, 3] in fp64, the elementwise bound 8 * 2^-24 * (|M| |Kinv| |p| + |t|), fg [N, HW] bool):
    c2w[:3, :4] @ [Kinv @ (d u, d v, d); 1] with d = 0 for a background pixel (not seg > 50)."""
    n, h, w = depth.shape
    with np.errstate(invalid="ignore"):
        fg = (np.asarray(seg, f32) > f32(50.0)).reshape(n, -1)
    d = np.where(fg, depth.reshape(n, -1).astype(np.float64), 0.0)
    yy, xx = np.divmod(np.arange(h * w), w)
    p = np.stack([d * xx, d * yy, d], -1)                             # [N, HW, 3]
    K = np.asarray(kinv, np.float64).reshape(3, 3)
    M = np.asarray(c2w, np.float64)[:, :3, :3]
    t = np.asarray(c2w, np.float64)[:, :3, 3]
    world = np.einsum("nij,npj->npi", M, p @ K.T) + t[:, None, :]
    mag = np.einsum("nij,npj->npi", np.abs(M), np.abs(p) @ np.abs(K).T) + np.abs(t)[:, None, :]
    return world, 8 * EPS * mag, fg


def err_over_bound(world, want, bound):
    return float((np.abs(world.astype(np.float64) - want) / bound).max())


# ---------------------------------------------------------------------------
# case inputs.  Every builder is deterministic and cached: the two test files see the same arrays, and nobody writes to them.
# ---------------------------------------------------------------------------
def _frames(n, g, rs):
    """range_gt off the origin and an anisotropic voxel_size of its own per env: (range_gt [N, 6], voxel_size [N, 3])."""
    v = rs.uniform(0.05, 0.6, (n, 3)).astype(f32)
    lo = rs.uniform(-7.0, 5.0, (n, 3)).astype(f32)
    hi = (lo + f32(g - 1) * v).astype(f32)
    return np.stack([hi[:, 0], lo[:, 0], hi[:, 1], lo[:, 1], hi[:, 2], lo[:, 2]], -1).astype(f32), v


# ---- 1. gnbv_post_process_depth ----
DEPTH_COUNTS = (0, 1, U.GRID_STRIDE_THREADS + 37)
DEPTH_SENSE = (-50.0, -3.5)


def depth_specials(sense):
    s = f32(sense)
    return np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, s, np.nextafter(s, f32(np.inf)), np.nextafter(s, f32(-np.inf)), FLT_MAX, -FLT_MAX,
                       DENORMAL, -DENORMAL, -1.25, 3.0, 255.0, -1000.0], f32)


@cached
def depth_case(count, sense):
    rs = np.random.RandomState(count % 997 + int(-sense * 2))
    sp = depth_specials(sense)
    m = max(count, 1)
    d = rs.uniform(2 * sense, 1.0, m).astype(f32)
    s = rs.choice(np.asarray([0.0, 50.0, 255.0, 17.5], f32), m)
    if count == 1:
        d[0], s[0] = -0.0, -0.0  # depth must come out +0.0, seg must stay -0.0
    elif count > 1:
        for a in (d, s):
            a[rs.choice(count, 20 * sp.size, replace=False)] = np.tile(sp, 20)
            a[:sp.size] = sp
            a[-sp.size:] = sp[::-1]
    return SimpleNamespace(count=count, sense=sense, depth=d, seg=s, specials=sp)


# ---- 2. gnbv_back_projection ----
BACKPROJ_SHAPES = ((1, 1, 1), (3, 7, 9), (2, 48, 64), (7, 240, 320))
SEG_BG = np.asarray([0.0, 50.0, np.nan], f32)                                      # not > 50
SEG_FG = np.asarray([np.nextafter(f32(50.0), f32(np.inf)), 255.0, 100.0], f32)


def generic_intrinsics(h, w):
    """Inverse intrinsics with skew and a perspective row: nine non-zero entries."""
    k = U.intrinsics(h, w, pinhole=True)
    k[0, 1] = 3e-4; k[1, 0] = -2e-4; k[2, 0] = 1e-6; k[2, 1] = -2e-6; k[2, 2] = 1.0009765625
    return k


@cached
def backproj_case(n, h, w, pinhole):
    rs = np.random.RandomState(n * 1000 + h + 7 * pinhole)
    kinv = U.intrinsics(h, w, True) if pinhole else generic_intrinsics(h, w)
    c2w = np.zeros((n, 4, 4), f32)
    for e in range(n):
        q, r = np.linalg.qr(rs.randn(3, 3))
        c2w[e, :3, :3] = q * np.sign(np.diag(r))
        c2w[e, :3, 3] = rs.uniform(-5.0, 5.0, 3)
    c2w[:, 3, :] = np.nan  # the kernel reads 12 of the 16 floats
    is_fg = rs.rand(n, h, w) < 0.5
    seg = np.where(is_fg, rs.choice(SEG_FG, (n, h, w)), rs.choice(SEG_BG, (n, h, w))).astype(f32)
    depth = rs.uniform(0.1, 50.0, (n, h, w)).astype(f32)
    if h * w == 1:  # one pixel: the foreground threshold from above (pinhole) or exactly on it with a NaN depth (generic)
        seg[:] = SEG_FG[0] if pinhole else f32(50.0)
        is_fg[:] = pinhole
    else:
        flat_s, flat_f = seg.reshape(n, -1), is_fg.reshape(n, -1)
        k = min(3, h * w // 8)
        flat_s[:, :k], flat_f[:, :k] = SEG_FG[:k], True
        flat_s[:, -k:], flat_f[:, -k:] = SEG_BG[:k], False
        dd = depth.reshape(n, -1)
        dd[:, 0], dd[:, 1] = 0.0, 50.0  # foreground pixels at both ends of the processed depth's range
    bg = ~is_fg
    depth[bg] = np.where(rs.rand(int(bg.sum())) < 0.5, f32(np.nan), f32(np.inf))  # a background pixel's depth is never used
    return SimpleNamespace(n=n, h=h, w=w, pinhole=pinhole, kinv=kinv, c2w=c2w, seg=seg, depth=depth, is_fg=is_fg.reshape(n, -1))


# ---- 3. gnbv_points_to_idx ----
POINTS_CASES = tuple((3, hw, g) for g in (1, 7, 16, 33, 128) for hw in (1, 37)) + ((3, 174800, 33),)
FG_BYTES = np.asarray([0, 1, 2, 255], np.uint8)
POINT_CLASSES_DROPPED = ("on_vmin", "on_vmax", "nan", "+inf", "-inf", "+1e30", "-1e30", "background")
POINT_CLASSES_KEPT = ("ulp_inside_vmin", "ulp_inside_vmax", "interior_face")


@cached
def points_case(n, hw, g):
    """Points uniform over 1.3x the frame, and planted ones whose other two coordinates lie well inside: `classes` maps a class to the
    (env, point, axis) triples that hold it."""
    rs = np.random.RandomState(g * 100 + hw % 1000)
    range_gt, v = _frames(n, g, rs)
    vmin, vmax = voxel_frame(range_gt, v)
    ctr, ext = (vmin.astype(np.float64) + vmax) / 2, (vmax.astype(np.float64) - vmin)
    world = (ctr[:, None] + ext[:, None] * rs.uniform(-0.65, 0.65, (n, hw, 3))).astype(f32)
    fg = rs.choice(FG_BYTES, (n, hw), p=[0.1, 0.4, 0.25, 0.25]).astype(np.uint8)
    classes = {c: [] for c in POINT_CLASSES_DROPPED + POINT_CLASSES_KEPT}
    names = list(classes)
    if hw == 1:  # one point per env: a kept edge, a dropped edge, an interior point behind the byte 255
        plan = [(0, 0, "ulp_inside_vmax"), (1, 0, "on_vmin"), (2, 0, None)]
    else:
        slots = np.concatenate([np.arange(3), hw - 1 - np.arange(3), 3 + rs.permutation(hw - 6)])
        reps = max(1, min(40, hw // (4 * len(names))))
        plan = [(e, int(slots[i]), c) for e in range(n) for i, c in enumerate(names * reps + ["interior_face"] * 2 * reps)]
    for j, (e, p, c) in enumerate(plan):
        a = j % 3
        world[e, p] = (ctr[e] + ext[e] * rs.uniform(-0.3, 0.3, 3)).astype(f32)
        fg[e, p] = FG_BYTES[1 + j % 3]
        if c is None:
            fg[e, p] = 255
            continue
        classes[c].append((e, p, a))
        if c == "background":
            fg[e, p] = 0
        else:
            world[e, p, a] = {"on_vmin": vmin[e, a], "on_vmax": vmax[e, a], "nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "+1e30": 1e30,
                              "-1e30": -1e30, "ulp_inside_vmin": np.nextafter(vmin[e, a], f32(np.inf)),
                              "ulp_inside_vmax": np.nextafter(vmax[e, a], f32(-np.inf)),
                              "interior_face": vmin[e, a] + f32(rs.randint(1, g) if g > 1 else 0) * v[e, a]}[c]
    if g == 1:  # (vmin + 0 v is vmin itself: no interior face in a grid of one voxel)
        for e, p, a in classes.pop("interior_face"):
            world[e, p, a] = f32(ctr[e, a])
    return SimpleNamespace(n=n, hw=hw, g=g, range_gt=range_gt, voxel_size=v, world=world, fg=fg, classes=classes, vmin=vmin, vmax=vmax)


# ---- 4. gnbv_pose_to_idx ----
POSE_NS = (1, 3, 300)


@cached
def pose_case(n):
    """Poses inside the frame, outside on both sides up to 1e6 voxels away, exactly on faces, and 0.3 voxels below vmin (a quotient
    in (-1, 0): floor gives -1, truncation 0)."""
    rs = np.random.RandomState(40 + n)
    range_gt, v = _frames(n, 16, rs)
    vmin, vmax = voxel_frame(range_gt, v)
    kind = rs.randint(0, 5, (n, 3))
    kind.reshape(-1)[:5] = [3, 0, 1, 2, 4][:min(5, 3 * n)]
    far = 10.0 ** rs.uniform(0, 6, (n, 3))
    q = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [rs.uniform(0, 16, (n, 3)), -far, 16 + far, np.full((n, 3), -0.3)],
                  rs.randint(-3, 20, (n, 3)).astype(np.float64))  # (kind 4: on a face)
    poses = (vmin + q.astype(f32) * v).astype(f32)
    return SimpleNamespace(n=n, range_gt=range_gt, voxel_size=v, poses=poses)


# ---- 5. gnbv_bresenham3d ----
BRESENHAM_CASES = ((0, 7), (1, 1), (1, 7), (255, 7), (256, 7), (257, 1), (257, 2), (257, 7), (257, 33), (257, 128), (5000, 2), (5000, 33))
BRESENHAM_PY_RAYS = 300  # rays of a case that the plain-Python reference walks (the planted ones come first)


def bresenham_sources(g):
    """Inside the grid, on two corners, outside on the negative side, outside beyond g, and up to 10 g away on both sides."""
    s = [(g // 2, g // 3, g - 1 - g // 4), (0, 0, 0), (g - 1, 0, g - 1), (-2, g // 2, -1 - g), (g, g + 3, g // 2), (10 * g, -10 * g, 4 * g)]
    return [np.asarray(x, np.int32) for x in dict.fromkeys(s)]


def bresenham_targets(src, rays, g, seed):
    sx, k = np.asarray(src, np.int64), max(1, g // 2)
    j = k // 2
    rel = [(k, k, j), (0, 0, 0), (k, j, k), (j, k, k), (-k, k, -j), (k, 0, 0), (0, -k, 0), (0, 0, k), (k, k, k), (k, -k, k), (-k, -k, -k),
           (k, j, j), (j, k, j), (j, j, -k), (2 * g, j, 1), (1, -3 * g, j)]
    planted = [sx + r for r in rel] + [np.asarray(t, np.int64) for t in ((-3, g + 2, 5 * g), (g - 1, g - 1, g - 1), (0, 0, 0), (g, 0, 0), (-1, -1, -1))]
    rs = np.random.RandomState(seed)
    rnd = rs.randint(-(g // 2) - 1, g + g // 2 + 2, (max(rays, 1), 3))
    return np.concatenate([np.asarray(planted, np.int64), rnd])[:rays].astype(np.int32).reshape(rays, 3)


@cached
def bresenham_case(rays, g):
    srcs = bresenham_sources(g)
    return SimpleNamespace(rays=rays, g=g, runs=[(s, bresenham_targets(s, rays, g, 7 * g + i)) for i, s in enumerate(srcs)])


def ray_classes(src, targets):
    """How many targets of a run are: the source itself, axis-aligned, full ties, two-way ties of the two largest deltas (xy, xz, yz)."""
    d = np.abs(np.asarray(targets, np.int64) - np.asarray(src, np.int64))
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return dict(same=int((d.sum(1) == 0).sum()), axis=int((((d > 0).sum(1)) == 1).sum()), tie3=int(((dx == dy) & (dy == dz) & (dx > 0)).sum()),
                tie_xy=int(((dx == dy) & (dx > dz)).sum()), tie_xz=int(((dx == dz) & (dx > dy)).sum()), tie_yz=int(((dy == dz) & (dy > dx)).sum()))


def check_ray_properties(src, targets, traj, lens, g, fill):
    """What holds for every ray, whatever the reference: points in grid, steps of at most one voxel per axis, both ends where they are in
    grid, the caller's fill behind the points."""
    src, targets = np.asarray(src, np.int64), np.asarray(targets, np.int64)
    k = np.arange(traj.shape[1])[None, :]
    valid = k < lens[:, None]
    assert (lens >= 0).all() and (lens <= g).all()
    assert (traj[~valid] == fill).all(), "entries behind a ray's points were written"
    pts = traj[valid]
    assert ((pts >= 0) & (pts < g)).all()
    step = np.abs(np.diff(traj.astype(np.int64), axis=1))
    assert (step[valid[:, 1:]] <= 1).all()
    inb = lambda p: ((p >= 0) & (p < g)).all(-1)
    if inb(src):
        assert (lens >= 1).all() and (traj[:, 0] == src).all()
    t_in = inb(targets)
    assert (lens[t_in] >= 1).all()
    last = traj[np.arange(len(lens)), np.maximum(lens - 1, 0)]
    assert (last[t_in] == targets[t_in]).all()


# ---- 6. gnbv_pack_grid_bits / gnbv_unpack_grid_bits ----
PACK_GS = (1, 3, 7, 20, 33, 64, 65)
PACK_NS = (1, 3)
BINARY_VALUES = np.asarray([0.0, 1.0, -0.0], f32)
OTHER_VALUES = np.asarray([0.5, -1.0, np.nan, np.inf, DENORMAL], f32)


@cached
def pack_case(n, g):
    """binary: values of {0, 1, -0.0} only; mixed: every planted value, at both ends of every row too."""
    rs = np.random.RandomState(g * 10 + n)
    g3 = g ** 3
    binary = rs.choice(BINARY_VALUES, (n, g3))
    mixed = rs.choice(np.concatenate([BINARY_VALUES, OTHER_VALUES]), (n, g3))
    if g3 >= 16:
        allv = np.concatenate([BINARY_VALUES, OTHER_VALUES])
        mixed[:, :allv.size], mixed[:, -allv.size:] = allv, allv[::-1]
        binary[:, :3], binary[:, -3:] = BINARY_VALUES, BINARY_VALUES
    else:
        mixed[-1, -1], binary[-1, -1] = DENORMAL, -0.0
    words = rs.randint(0, 2 ** 32, (n, U.mask_words(g)), dtype=np.uint64).astype(np.uint32)  # (garbage in the pad bits and words)
    return SimpleNamespace(n=n, g=g, binary=binary.astype(f32), mixed=mixed.astype(f32), words=words)


# ---- 7. gnbv_decode_prob_grid ----
DECODE_COUNTS = (0, 1, U.GRID_STRIDE_THREADS + 37)


@cached
def decode_case(count):
    rs = np.random.RandomState(count % 991)
    code = rs.randint(0, 256, max(count, 1)).astype(np.uint8)
    if count >= 512:
        code[:256], code[-256:] = np.arange(256), np.arange(256)[::-1]
    elif count == 1:
        code[0] = 200
    odd = rs.randint(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32)  # a table of arbitrary bit patterns
    odd[:4] = [0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800001]           # NaN payloads, -0.0, a signalling NaN
    odd[200] = 0xFF800000
    return SimpleNamespace(count=count, code=code, odd_lut=odd.view(f32))


# ---- 8. gnbv_unpack_masks ----
UNPACK_MASK_CASES = ((3, 7), (2, 33), (2, 65))


@cached
def unpack_masks_case(n, g):
    """The words of a workspace: hit rows first, path rows from word n * words on."""
    words = U.mask_words(g)
    rs = np.random.RandomState(n * 7 + g)
    return SimpleNamespace(n=n, g=g, words=words, mask=rs.randint(0, 2 ** 32, (2, n, words), dtype=np.uint64).astype(np.uint32))


# ---- 9. the fused update against the operator chain ----
FUSED_CASES = {"n3-30x37-g16": dict(n=3, g=16, h=30, w=37, seed=1, fg_share=(0.0, 0.7, 0.7), outside_share=0.5),
               "n2-48x64-g33": dict(n=2, g=33, h=48, w=64, seed=0, fg_share=0.7, outside_share=0.5)}


@cached
def fused_case(cid):
    kw = dict(FUSED_CASES[cid])
    kw["fg_share"] = np.asarray(kw["fg_share"], np.float64)
    return U.make_case(steps=1, reset_at=(), **kw)


def chain_masks(idx, src, g, walk):
    """hit and path [N, g^3] bool of the operator chain: idx [N, HW, 3] of points_to_idx, src [N, 3] of pose_to_idx, walk(source,
    targets, g) -> (trajectory_pts, trajectory_lengths).  Returns also the distinct hit voxels per env (the targets)."""
    n = idx.shape[0]
    hit, path, targets = np.zeros((n, g ** 3), bool), np.zeros((n, g ** 3), bool), []
    for e in range(n):
        kept = idx[e][idx[e, :, 0] >= 0].astype(np.int64)
        t = np.unique(kept, axis=0).reshape(-1, 3) if len(kept) else kept
        targets.append(t.astype(np.int32))
        hit[e, (t[:, 0] * g + t[:, 1]) * g + t[:, 2]] = True
        if len(t):
            traj, lens = walk(np.asarray(src[e], np.int64).astype(np.int32), t.astype(np.int32), g)
            pts = traj[np.arange(traj.shape[1])[None, :] < lens[:, None]].astype(np.int64)
            path[e, (pts[:, 0] * g + pts[:, 1]) * g + pts[:, 2]] = True
    return hit, path, targets

"""Cell-grid variants of one set of triangles, for the kernels that read a GnbvMeshScene (tests/test_mesh_grids_*.py).

include/gennbv_hip.h promises one thing about a scene's cell grid: every cell's list is a conservative superset of the
triangles that touch it.  So no kernel's answer may depend on WHICH conservative grid it gets.  `variants` builds, from one
list of per-env triangles (the same triangle order in every variant, so MeshScene.objects() and the fp64 oracles are
shared):

  default     MeshScene.from_triangles as is
  one         max_cells_per_axis = 1: one cell per env that lists everything
  fine        many cells per triangle (hundreds to thousands of cells under a body, long DDA walks)
  loose       hand-built: a box several metres larger than the scene on every side (it holds the cameras and reaches below
              z = 0), unequal resolutions with strongly anisotropic cells, one env with res == 1 on two axes; a triangle is
              listed by the builder's rule (AABB padded by EPS_REL * the grid's largest extent + EPS_ABS) applied to this box
  overlisted  default's geometry, every triangle's cell range widened by one cell on each side; in one env every triangle is
              listed in every cell
  shuffled    default's geometry and cells, every cell's entries in random order, about one entry in ten listed twice
  scattered   default's lists, laid out differently: the env blocks in reverse env order in cell_start (cell_base decreasing)
              with runs of unused empty cells between them

Everything here is host side, numpy / torch on the CPU; `to_device` moves a finished scene.  The `*_stats` functions count, with
the kernels' own formulas, the regimes the GPU tests claim to reach.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from gennbv_amd.env.mesh_scene import EPS_ABS, EPS_REL, MeshScene, box_triangles, random_rotation, sphere_triangles

f32 = np.float32
VARIANTS = ("default", "one", "fine", "loose", "overlisted", "shuffled", "scattered")
K_WAVE = 64  # csrc/common.h kWave: cells per batch and entries per step of wave_any_listed_tri
K_BLOCK, K_CAP = 512, 1024  # csrc/voxelize.hip kBlock, kCap
FINE_CELLS_PER_TRIANGLE = 50.0
LOOSE_RES = [(3, 17, 40), (40, 5, 11), (7, 23, 4), (1, 1, 23)]  # per env, cycled; the last: res == 1 on two axes
LOOSE_MARGIN = ((3.0, 5.5, 4.0), (6.0, 2.5, 7.0))  # metres added below / above the triangle bounds, per axis
CAMERA_REGION = ((-8.5, -8.5, -0.5), (8.5, 8.5, 10.6))  # holds every lattice pose of TaskConfig; the loose box holds it
GAP = 37  # unused cells between the env blocks of `scattered`


# ---------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------
def _rotated_boxes(gen, k, first_id=1):
    t, i = [], []
    for b in range(k):
        half = 0.5 + torch.rand(3, generator=gen, dtype=torch.float64) * 2.0
        tri = box_triangles(-half[None], half[None]).double() @ random_rotation(gen).T
        centre = torch.cat([(torch.rand(2, generator=gen, dtype=torch.float64) - 0.5) * 9.0,
                            2.0 + torch.rand(1, generator=gen, dtype=torch.float64) * 4.0])
        t.append((tri + centre).float())
        i.append(torch.full((12,), first_id + b, dtype=torch.int32))
    return t, i


def scene_triangles(seed: int = 12):
    """(tris, ids) of four envs, in the style of tests/test_render_gpu.py::_rotated_mesh: rotated boxes and a small sphere; a
    UV sphere of 2 208 triangles beside a rotated box (so `one` gives a list longer than kBlock and kCap); no triangles; three
    rotated boxes."""
    gen = torch.Generator().manual_seed(seed)
    tris, ids = [], []
    t, i = _rotated_boxes(gen, 3)
    s = sphere_triangles((2.5, -3.0, 3.0), 1.4, 10, 20)
    tris.append(torch.cat(t + [s]))
    ids.append(torch.cat(i + [torch.full((s.shape[0],), 7, dtype=torch.int32)]))
    big = sphere_triangles((0.5, -0.3, 3.0), 1.6, 24, 48)
    half = torch.tensor([[0.8, 1.2, 0.6]], dtype=torch.float64)
    box = (box_triangles(-half, half).double() @ random_rotation(gen).T + torch.tensor([-3.5, 3.0, 2.5], dtype=torch.float64)).float()
    tris.append(torch.cat([big, box]))
    ids.append(torch.cat([torch.full((big.shape[0],), 1, dtype=torch.int32), torch.full((12,), 2, dtype=torch.int32)]))
    tris.append(torch.zeros(0, 3, 3))
    ids.append(torch.zeros(0, dtype=torch.int32))
    t, i = _rotated_boxes(gen, 3)
    tris.append(torch.cat(t))
    ids.append(torch.cat(i))
    return tris, ids


THIN_FOV = 3.0  # degrees: the camera of the long thin scene looks down the tube


def thin_scene_triangles():
    """(tris, ids) of one env 19 m long and 0.4 m across: small spheres and a rotated box along the floor of a tube along x, a sphere
    closing its far end.  Binned finely it has hundreds of cells along x and a handful across."""
    gen = torch.Generator().manual_seed(5)
    end = sphere_triangles((9.3, 0.0, 2.2), 0.19, 8, 12)
    half = torch.tensor([[0.05, 0.07, 0.04]], dtype=torch.float64)
    mid = (box_triangles(-half, half).double() @ random_rotation(gen).T + torch.tensor([1.0, 0.08, 2.1], dtype=torch.float64)).float()
    parts, pid = [end, mid], [torch.full((end.shape[0],), 1, dtype=torch.int32), torch.full((12,), 2, dtype=torch.int32)]
    for k, x in enumerate((-9.4, -5.0, -1.0, 3.5, 7.0)):
        s = sphere_triangles((x, -0.12 + 0.05 * (k % 2), 2.08), 0.06, 6, 10)
        parts.append(s)
        pid.append(torch.full((s.shape[0],), 3 + k, dtype=torch.int32))
    return [torch.cat(parts)], [torch.cat(pid)]


def thin_poses():
    """[3,6] camera poses of the thin scene (three copies of the env, one pose each): level down the tube from inside the grid box,
    from behind its end a little obliquely, and level across it from the side."""
    return torch.tensor([[-9.0, 0.04, 2.36, 0.0, 0.0, 0.0],
                         [-12.0, 0.1, 2.4, 0.0, 0.004, -0.004],
                         [-9.45, -0.2, 2.3, 0.0, 0.0, 0.02]], dtype=torch.float32)


def thin_variants(device="cpu"):
    """{"one", "fine"} of three copies of the thin env; fine has res >= 256 along x and <= 8 across."""
    t, i = thin_scene_triangles()
    t, i = t * 3, i * 3
    return {"one": MeshScene.from_triangles(t, i, device=device, max_cells_per_axis=1),
            "fine": MeshScene.from_triangles(t, i, device=device, cells_per_triangle=24.0, max_cells_per_axis=1024)}


def walk_scene_triangles():
    """(tris, ids, small) of the one-env scene of the hand cases of the cell walk: the 2 208-triangle sphere, and one small
    horizontal triangle stored LAST, far from the sphere; small = its centre."""
    big = sphere_triangles((0.0, 0.0, 3.0), 1.5, 24, 48)
    c = np.array([5.0, 5.0, 2.0], np.float64)
    d = 0.02
    small = torch.tensor([[[c[0] - d, c[1] - d, c[2]], [c[0] + d, c[1] - d, c[2]], [c[0], c[1] + d, c[2]]]], dtype=torch.float32)
    tris = torch.cat([big, small])
    return [tris], [torch.cat([torch.full((big.shape[0],), 1, dtype=torch.int32), torch.full((1,), 2, dtype=torch.int32)])], c


def walk_hand_poses(c, half_length, clear: bool):
    """The upright body (roll = pitch = 0: axis z) whose top cap's centre lies 0.5 mm above the small triangle at c (the triangle
    is inside the body by 0.5 mm), or, `clear`, 1 mm below it."""
    top = c[2] + (-1e-3 if clear else 5e-4)
    return np.array([[c[0], c[1], top - float(f32(half_length)), 0.0, 0.0, 0.0]], f32)


# ---------------------------------------------------------------------------------------------------------------
# cell lists as COO, and their layout
# ---------------------------------------------------------------------------------------------------------------
def to_device(m: MeshScene, device) -> MeshScene:
    return MeshScene(*[t.to(device) for t in (m.tris, m.tri_obj, m.tri_env)], m.tri_count,
                     *[t.to(device) for t in (m.cell_lo, m.cell_size, m.cell_res, m.cell_base, m.cell_start, m.cell_tris)])


def env_entries(m: MeshScene, e: int):
    """(cell [E] local cell index, ascending; tri [E] global triangle index) of env e's lists, in stored order."""
    r = m.cell_res[e].tolist()
    ncell, base = r[0] * r[1] * r[2], int(m.cell_base[e])
    start = m.cell_start[base:base + ncell + 1].cpu().numpy().astype(np.int64)
    if ncell == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    cell = np.repeat(np.arange(ncell, dtype=np.int64), np.diff(start))
    return cell, m.cell_tris[int(start[0]):int(start[-1])].cpu().numpy().astype(np.int64)


def _assemble(ref: MeshScene, lo, size, res, entries, order=None, gap=0) -> MeshScene:
    """A MeshScene over ref's triangles with the grid (lo, size, res [N,3]) and per-env COO entries (cell ascending).  `order`: the
    envs' cell blocks in this order in cell_start, `gap` unused cells before each block and after the last."""
    n = ref.num_envs
    res = np.asarray(res, np.int64)
    ncell = res.prod(-1)
    order = list(range(n)) if order is None else list(order)
    base = np.zeros(n, np.int64)
    counts, tris, at = [], [], 0
    for e in order:
        counts.append(np.zeros(gap, np.int64))
        at += gap
        base[e] = at if ncell[e] else max(at - gap // 2, 0)  # an env without cells: its base is never read; here it points into the gap
        cell, tri = entries[e]
        assert cell.size == 0 or (np.diff(cell) >= 0).all() and cell[-1] < ncell[e]
        counts.append(np.bincount(cell, minlength=int(ncell[e])).astype(np.int64))
        tris.append(tri)
        at += int(ncell[e])
    counts.append(np.zeros(gap, np.int64))
    counts = np.concatenate(counts)
    start = np.zeros(counts.size + 1, np.int64)
    start[1:] = np.cumsum(counts)
    tris = np.concatenate(tris) if tris else np.zeros(0, np.int64)
    assert start[-1] == tris.size < 2 ** 31
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).contiguous()
    return MeshScene(ref.tris, ref.tri_obj, ref.tri_env, ref.tri_count, t(np.asarray(lo, f32), torch.float32), t(np.asarray(size, f32), torch.float32),
                     t(res, torch.int32), t(base, torch.int32), t(start, torch.int32), t(tris, torch.int32))


def _entries_of_ranges(i0, i1, res, first):
    """COO entries (cell ascending, triangles ascending inside a cell) of triangles first .. first + T - 1 listed in the cells
    i0 .. i1 [T,3] of a grid of `res`."""
    span = i1 - i0 + 1
    per = span.prod(-1)
    tri_of = np.repeat(np.arange(i0.shape[0], dtype=np.int64), per)
    k = np.arange(tri_of.size, dtype=np.int64) - (np.cumsum(per) - per)[tri_of]
    sp = span[tri_of]
    cx = i0[tri_of, 0] + k % sp[:, 0]
    cy = i0[tri_of, 1] + (k // sp[:, 0]) % sp[:, 1]
    cz = i0[tri_of, 2] + k // (sp[:, 0] * sp[:, 1])
    cell = cx + res[0] * (cy + res[1] * cz)
    order = np.lexsort((tri_of, cell))
    return cell[order], tri_of[order] + first


def _ranges_of_entries(cell, tri, res, first, count):
    """The box of cells (i0, i1 [T,3]) each triangle is listed in (the builder lists a triangle in a box of cells)."""
    ijk = np.stack([cell % res[0], (cell // res[0]) % res[1], cell // (res[0] * res[1])], -1)
    i0 = np.full((count, 3), np.iinfo(np.int64).max, np.int64)
    i1 = np.full((count, 3), -1, np.int64)
    np.minimum.at(i0, tri - first, ijk)
    np.maximum.at(i1, tri - first, ijk)
    return i0, i1


def _loose(ref: MeshScene) -> MeshScene:
    n = ref.num_envs
    lo, size, res, entries = np.zeros((n, 3), f32), np.ones((n, 3), f32), np.zeros((n, 3), np.int64), []
    first = 0
    for e in range(n):
        t = ref.env_triangles(e)[0].numpy()
        cnt = t.shape[0]
        if cnt == 0:
            entries.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))
            continue
        v = t.reshape(-1, 3)
        blo = (np.minimum(v.min(0), np.array(CAMERA_REGION[0])) - np.array(LOOSE_MARGIN[0])).astype(f32)
        bhi = (np.maximum(v.max(0), np.array(CAMERA_REGION[1])) + np.array(LOOSE_MARGIN[1])).astype(f32)
        r = np.array(LOOSE_RES[e % len(LOOSE_RES)], np.int64)
        sz = ((bhi - blo) / r.astype(f32)).astype(f32)
        eps = f32((bhi - blo).max() * f32(EPS_REL) + f32(EPS_ABS))
        # the builder's rule (MeshScene._bin), in its own fp32 arithmetic, on this box
        i0 = np.clip(np.floor((t.min(1) - eps - blo) / sz).astype(np.int64), 0, None)
        i1 = np.minimum(np.floor((t.max(1) + eps - blo) / sz).astype(np.int64), r - 1)
        i0 = np.minimum(i0, i1)
        lo[e], size[e], res[e] = blo, sz, r
        entries.append(_entries_of_ranges(i0, i1, r, first))
        first += cnt
    return _assemble(ref, lo, size, res, entries)


def _derived(ref: MeshScene, default: MeshScene, seed: int, names):
    """overlisted, shuffled, scattered (those in `names`) from default's lists."""
    n = ref.num_envs
    rs = np.random.RandomState(seed)
    res = default.cell_res.numpy().astype(np.int64)
    lo, size = default.cell_lo.numpy(), default.cell_size.numpy()
    with_tris = [e for e in range(n) if int(ref.tri_count[e])]
    everywhere = with_tris[-1]  # the env whose every cell lists every triangle
    plain, over, shuf = [], [], []
    first = 0
    for e in range(n):
        cell, tri = env_entries(default, e)
        cnt = int(ref.tri_count[e])
        plain.append((cell, tri))
        if cnt == 0:
            over.append((cell, tri))
            shuf.append((cell, tri))
            continue
        if "overlisted" in names:
            i0, i1 = _ranges_of_entries(cell, tri, res[e], first, cnt)
            if e == everywhere:
                i0, i1 = np.zeros_like(i0), np.broadcast_to(res[e] - 1, i1.shape).copy()
            else:
                i0, i1 = np.maximum(i0 - 1, 0), np.minimum(i1 + 1, res[e] - 1)
            over.append(_entries_of_ranges(i0, i1, res[e], first))
        twice = rs.rand(cell.size) < 0.1
        c2, t2 = np.concatenate([cell, cell[twice]]), np.concatenate([tri, tri[twice]])
        p = rs.permutation(c2.size)
        c2, t2 = c2[p], t2[p]
        o = np.argsort(c2, kind="stable")
        shuf.append((c2[o], t2[o]))
        first += cnt
    out = {"shuffled": _assemble(ref, lo, size, res, shuf),
           "scattered": _assemble(ref, lo, size, res, plain, order=list(range(n))[::-1], gap=GAP)}
    if "overlisted" in names:
        out["overlisted"] = _assemble(ref, lo, size, res, over)
    return out


def variants(tris, ids, device="cpu", seed: int = 0, names=VARIANTS):
    """{name: MeshScene on `device`} over the same triangles in the same order."""
    cpu = lambda **kw: MeshScene.from_triangles(tris, ids, device="cpu", **kw)
    default = cpu()
    out = {"default": default}
    if "one" in names:
        out["one"] = cpu(max_cells_per_axis=1)
    if "fine" in names:
        out["fine"] = cpu(cells_per_triangle=FINE_CELLS_PER_TRIANGLE)
    if "loose" in names:
        out["loose"] = _loose(default)
    if set(names) & {"overlisted", "shuffled", "scattered"}:
        out.update(_derived(default, default, seed, names))
    return {k: to_device(out[k], device) for k in names}


# ---------------------------------------------------------------------------------------------------------------
# superset / consistency (CPU tests)
# ---------------------------------------------------------------------------------------------------------------
def brute_force_cells(m: MeshScene, e: int):
    """Cells of env e whose box intersects each triangle (separating-axis test, fp64), as a set of (cell, tri)."""
    t, _ = m.env_triangles(e)
    first = int(m.tri_count[:e].sum())
    r = m.cell_res[e].tolist()
    ncell = r[0] * r[1] * r[2]
    c = torch.arange(ncell)
    ijk = torch.stack([c % r[0], (c // r[0]) % r[1], c // (r[0] * r[1])], -1).to(torch.float32)
    lo32 = m.cell_lo[e] + ijk * m.cell_size[e]  # MeshScene.cell_box of every cell
    lo, hi = lo32.double(), (lo32 + m.cell_size[e]).double()
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    out = set()
    axes_e = torch.eye(3, dtype=torch.float64)
    for i in range(t.shape[0]):
        v = t[i].double()[None] - ctr[:, None, :]  # [C,3,3]
        edges = [v[0, 1] - v[0, 0], v[0, 2] - v[0, 1], v[0, 0] - v[0, 2]]
        axes = [axes_e[a] for a in range(3)] + [torch.cross(edges[0], edges[1], dim=0)]
        axes += [torch.cross(axes_e[a], ed, dim=0) for a in range(3) for ed in edges]
        sep = torch.zeros(ncell, dtype=torch.bool)
        for ax in axes:
            if ax.norm() < 1e-12:
                continue
            p = v @ ax  # [C,3]
            rad = (half * ax.abs()).sum(-1)
            sep |= (p.amin(-1) > rad) | (p.amax(-1) < -rad)
        out |= {(int(c), first + i) for c in torch.nonzero(~sep).flatten()}
    return out


def listed(m: MeshScene, e: int):
    """The (cell, tri) pairs of env e's lists, as a set."""
    cell, tri = env_entries(m, e)
    return set(zip(cell.tolist(), tri.tolist()))


# ---------------------------------------------------------------------------------------------------------------
# the regimes, counted with the kernels' formulas
# ---------------------------------------------------------------------------------------------------------------
def cell_range(m: MeshScene, e: int, lo, hi):
    """csrc/scene_cells.h cell_range in fp64: (c0, c1 [3]) or None."""
    res = m.cell_res[e].cpu().numpy().astype(np.int64)
    if res[0] <= 0:
        return None
    clo, csz = m.cell_lo[e].cpu().numpy().astype(np.float64), m.cell_size[e].cpu().numpy().astype(np.float64)
    f0 = np.floor((np.asarray(lo, np.float64) - clo) / csz - 1e-6)
    f1 = np.floor((np.asarray(hi, np.float64) - clo) / csz + 1e-6)
    top = (res - 1).astype(np.float64)
    if not ((f1 >= 0) & (f0 <= top)).all():
        return None
    return np.minimum(np.maximum(f0, 0), top).astype(np.int64), np.maximum(np.minimum(f1, top), 0).astype(np.int64)


def body_box(pose, r, h):
    """csrc/collide.hip collide_code's AABB [blo, bhi] of the cylinder (radius r, half length h) at pose [6]."""
    from tests.collision_oracle import axes
    p = np.asarray(pose, f32)
    c = p[:3].astype(np.float64)
    a = axes(p[None])[0]
    r, h = float(f32(r)), float(f32(h))
    ext = r * np.sqrt(np.maximum(0.0, 1.0 - a * a)) + h * np.abs(a)
    grow = 1e-12 * (np.abs(c).max() + r + h)
    return c - ext - grow, c + ext + grow


def walk_stats(m: MeshScene, e: int, lo, hi):
    """wave_any_listed_tri over the cells of box [lo, hi] with no previous range: (cells, most flat entries of one 64-cell batch,
    batches, the global cell index of every flat cell j in walk order)."""
    rng = cell_range(m, e, lo, hi)
    if rng is None:
        return 0, 0, 0, np.zeros(0, np.int64)
    c0, c1 = rng
    res = m.cell_res[e].cpu().numpy().astype(np.int64)
    nx, ny, nz = (c1 - c0 + 1).tolist()
    j = np.arange(nx * ny * nz, dtype=np.int64)
    kx, ky, kz = c0[0] + j % nx, c0[1] + (j // nx) % ny, c0[2] + j // (nx * ny)
    cell = int(m.cell_base[e]) + kx + res[0] * (ky + res[1] * kz)
    start = m.cell_start.cpu().numpy().astype(np.int64)
    cnt = start[cell + 1] - start[cell]
    per_batch = np.add.reduceat(cnt, np.arange(0, j.size, K_WAVE))
    return int(j.size), int(per_batch.max()), int(per_batch.size), cell


def brick_candidates(m: MeshScene, e: int, range_row, vox_row, g: int):
    """Per 8^3 brick of env e's voxel grid: the number of the env's triangles whose AABB meets the brick's box (every such triangle
    is a candidate of k_voxelize_surface at least once, whatever the grid).  [nb, nb, nb]."""
    from tests.voxelize_oracle import voxel_bounds
    face = voxel_bounds(np.asarray(range_row), np.asarray(vox_row), g)[2]
    t = m.env_triangles(e)[0].cpu().numpy().astype(np.float64)
    nb = (g + 7) // 8
    out = np.zeros((nb, nb, nb), np.int64)
    if t.shape[0] == 0:
        return out
    tmin, tmax = t.min(1), t.max(1)
    meets = []
    for a in range(3):
        blo = face[a][np.arange(nb) * 8]
        bhi = face[a][np.minimum(np.arange(nb) * 8 + 8, g)]
        meets.append((tmax[:, a][None] >= blo[:, None]) & (tmin[:, a][None] <= bhi[:, None]))  # [nb, T]
    return np.einsum("xt,yt,zt->xyz", *[x.astype(np.int64) for x in meets])


def dda_steps(m: MeshScene, e: int, origin, dirs, t_hit):
    """Cells the renderer's walk crosses per ray before it stops, in fp64: from the grid box's entry (at least 1e-3) to the closest
    hit `t_hit` or the box's exit, one step per cell boundary crossed.  dirs [R,3], t_hit [R] (inf: none) -> [R] (0: the ray misses
    the box)."""
    res = m.cell_res[e].cpu().numpy().astype(np.int64)
    lo, sz = m.cell_lo[e].cpu().numpy().astype(np.float64), m.cell_size[e].cpu().numpy().astype(np.float64)
    o, d = np.asarray(origin, np.float64), np.asarray(dirs, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a0, a1 = (lo - o) / d, (lo + res * sz - o) / d
    t_in = np.maximum(np.nanmax(np.minimum(a0, a1), -1), 1e-3)
    t_out = np.nanmin(np.maximum(a0, a1), -1)
    t_end = np.minimum(t_out, np.asarray(t_hit, np.float64))
    ok = (t_in <= t_out) & (t_end > t_in)
    idx = lambda t: np.clip(np.floor((o + d * t[:, None] - lo) / sz), 0, res - 1)
    steps = np.abs(idx(np.where(ok, t_end, 0.0)) - idx(np.where(ok, t_in, 0.0))).sum(-1)
    return np.where(ok, steps, 0).astype(np.int64)


def lattice_poses(n: int, k: int, seed: int, cfg=None):
    """[n,k,6] f32 random poses of the task's lattice."""
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.config import TaskConfig
    cfg = cfg or TaskConfig()
    a = S.sample_actions(n * k, cfg, torch.Generator().manual_seed(seed))
    return S.poses_from_actions(a, cfg).float().reshape(n, k, 6)


def render_poses(seed: int):
    """[4,6]: env 0 a lattice pose, env 1 straight down from above the big sphere, env 2 (no triangles) a lattice pose, env 3 level
    (pitch 0: a row of rays with dz == 0).  Every camera lies inside the loose box."""
    p = lattice_poses(4, 1, seed)[:, 0].clone()
    p[1] = torch.tensor([0.4, -0.2, 9.9, 0.0, math.pi / 2, 0.0])
    p[3, 2], p[3, 4] = 3.0, 0.0
    return p


# ---------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests and the regimes they must reach (asserted on the CPU and again on the GPU machine)
# ---------------------------------------------------------------------------------------------------------------
DRONE = (0.1, 0.02)  # tests/test_collision_gpu.py R, H
LARGE = (1.0, 0.5)  # spans hundreds of `fine` cells
VOXEL_RANGE = [8.0, -8.0, 8.0, -8.0, 8.0, 0.0]  # the explicit voxel frame (xmax, xmin, ymax, ymin, zmax, zmin)
CAMERAS = ((37, 53), (48, 64))
POSES_PER_ENV = 256


def collide_poses(tris, seed: int = 3):
    """[n, 256, 6] f32: per env 128 poses near the surface (any attitude) and 128 on the task's lattice."""
    from tests.test_collision_gpu import _near_surface_poses
    n, half = len(tris), POSES_PER_ENV // 2
    gen = torch.Generator().manual_seed(seed)
    near = np.stack([_near_surface_poses(np.asarray(tris[e]), half, gen, False) for e in range(n)])
    return np.concatenate([near, lattice_poses(n, half, seed + 1).numpy()], 1).astype(f32)


def sweep_flights(tris, k: int = 48, seed: int = 8):
    """(a, b) [n, k, 3] f32: the flights of tests/test_sweep_gpu.py's one-vs-fine test on this scene -- grazing flights, lattice
    to lattice, and the long diagonal across every env."""
    from gennbv_amd.env.config import TaskConfig
    from tests.test_sweep_gpu import _grazing_flights, _lattice_poses
    n, cfg, rs = len(tris), TaskConfig(), np.random.RandomState(seed)
    ab = [_grazing_flights(np.asarray(tris[e]), k // 2, rs) for e in range(n)]
    a = np.concatenate([np.stack([x[0] for x in ab]), _lattice_poses(cfg, n, k // 2, rs)[..., :3]], 1)
    b = np.concatenate([np.stack([x[1] for x in ab]), _lattice_poses(cfg, n, k // 2, rs)[..., :3]], 1)
    a[:, -1], b[:, -1] = [-9.5, -9.0, 0.3], [9.5, 9.0, 9.7]
    return a.astype(f32), b.astype(f32)


def check_walk_regimes(vs, poses):
    """The regimes of wave_any_listed_tri the collide cases claim, over every 16th pose: under the large body more than 128 cells
    of `fine` and more than 64 of `overlisted` (second and later batches); more than 64 flat entries in one batch on `one`,
    `overlisted` and `fine` (the i0 loop); ranges with empty cells between full ones (the search across lanes with equal incl).
    -> {variant: (most cells, most entries of a batch, ranges with such holes)}."""
    n = poses.shape[0]
    most = {}
    for name in ("one", "fine", "overlisted", "shuffled"):
        m = vs[name]
        cells, entries, holes = [], [], 0
        for e in range(n):
            for p in poses[e, ::16]:
                nc, mb, _, cell = walk_stats(m, e, *body_box(p, *LARGE))
                cells.append(nc)
                entries.append(mb)
                if nc:
                    start = m.cell_start.cpu().numpy()
                    cnt = start[cell + 1] - start[cell]
                    holes += int(((cnt[1:-1] == 0) & (cnt[:-2] > 0)).any() and (cnt > 0).sum() > 1)
        most[name] = (max(cells), max(entries), holes)
    assert most["fine"][0] > 128 and most["overlisted"][0] > 64, most
    assert most["one"][1] > K_WAVE and most["fine"][1] > K_WAVE and most["overlisted"][1] > K_WAVE, most
    assert most["fine"][2] > 0 and most["shuffled"][2] > 0, most
    return most


def check_walk_hand_cases(one: MeshScene, fine: MeshScene, centre):
    """On `one` the small triangle is the last of more than 2 048 entries; on `fine` it is listed only in the top layer of the
    large body's range, that layer has more than 64 cells, and its cell falls into the last batch."""
    last = one.num_triangles - 1
    cell, tri = env_entries(one, 0)
    assert tri.size > 2048 and int(tri[-1]) == last and int((tri == last).sum()) == 1
    cell, tri = env_entries(fine, 0)
    mine = cell[tri == last] + int(fine.cell_base[0])
    for clear in (False, True):
        lo, hi = body_box(walk_hand_poses(centre, LARGE[1], clear)[0], *LARGE)
        c0, c1 = cell_range(fine, 0, lo, hi)
        ncell, _, batches, walk = walk_stats(fine, 0, lo, hi)
        nx, ny = int(c1[0] - c0[0] + 1), int(c1[1] - c0[1] + 1)
        assert nx * ny > K_WAVE and batches > 2
        j = np.nonzero(np.isin(walk, mine))[0]
        assert j.size >= 1 and (j >= ncell - nx * ny).all(), "the small triangle is listed below the top layer"
        assert (j // K_WAVE == batches - 1).all(), (j, ncell)


def check_brick_regime(m: MeshScene, rng, vox, g: int):
    """k_voxelize_surface's flush runs when a brick gathers more than kCap - kBlock candidates: here one brick's box meets the AABBs
    of more triangles than that (each is a candidate at least once on every grid), and `one` lists them in one cell longer than
    kBlock (the k0 loop)."""
    most = max(int(brick_candidates(m, e, rng[e], vox[e], g).max()) for e in range(m.num_envs))
    assert most > K_CAP - K_BLOCK, most
    return most


def check_render_inputs(vs, poses):
    """Every camera lies inside its env's `loose` box, which reaches below z = 0 and is far larger than the scene."""
    m, d = vs["loose"], vs["default"]
    for e in range(m.num_envs):
        if int(m.cell_res[e, 0]) == 0:
            continue
        lo = m.cell_lo[e].cpu()
        hi = lo + m.cell_size[e].cpu() * m.cell_res[e].cpu().float()
        p = poses[e, :3].cpu()
        assert bool((p > lo).all() and (p < hi).all()) and float(lo[2]) < -1.0
        tight = d.cell_size[e].cpu() * d.cell_res[e].cpu().float()
        assert bool(((hi - lo) > tight + 6.0).all())


def walk_side_poses(c, clear: bool):
    """[144, 6] upright large bodies whose SIDE meets the small triangle at c, all around it and at nine heights from its bottom rim to
    its top rim (the triangle's centre 0.5 mm inside the radius), or, `clear`, passes it more than 1 mm away.  Over these placements
    the triangle's cell falls into the first, the second and many later 64-cell batches of the body's range."""
    r, h = float(f32(LARGE[0])), float(f32(LARGE[1]))
    dist = r + (0.03 if clear else -5e-4)  # the triangle reaches 0.0283 m from its centre
    phi, dz = np.meshgrid(np.arange(16) * (2 * math.pi / 16), np.linspace(-0.49, 0.49, 9) * (h / 0.5), indexing="ij")
    p = np.zeros((phi.size, 6), f32)
    p[:, 0], p[:, 1], p[:, 2] = c[0] - dist * np.cos(phi.ravel()), c[1] - dist * np.sin(phi.ravel()), c[2] - dz.ravel()
    return p


def check_walk_batches(fine: MeshScene, poses):
    """The 64-cell batches of the large body's range that hold the last triangle's cell, over `poses`: the first three and at least
    a dozen different ones occur.  -> the sorted batch indices."""
    last = fine.num_triangles - 1
    cell, tri = env_entries(fine, 0)
    mine = cell[tri == last] + int(fine.cell_base[0])
    seen = set()
    for p in poses:
        walk = walk_stats(fine, 0, *body_box(p, *LARGE))[3]
        j = np.nonzero(np.isin(walk, mine))[0]
        assert j.size >= 1
        seen.add(int(j.min()) // K_WAVE)  # the first batch that lists it; the walk must not lose it before
    assert {0, 1, 2} <= seen and len(seen) >= 12, sorted(seen)
    return sorted(seen)

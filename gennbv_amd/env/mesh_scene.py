"""MeshScene: per-env triangle geometry for the closed-loop renderer (csrc/render.hip).

Each env holds a triangle soup in env-local coordinates (the frame of the poses and of `range_gt`); every triangle
carries an int object id > 0.  Over each env's triangle bounds lies a uniform grid of cells whose triangle lists are
stored as CSR (cell -> triangle indices).  A triangle is listed in every cell its axis-aligned bounding box, padded
by `eps`, overlaps: the lists are a conservative superset, so a ray that crosses a triangle always visits a cell that
lists it, also where the renderer's fp32 cell walk rounds a boundary crossing by a few ulps.

The lists are built once with torch on the scene's device: set-up work, not hot path.

Cell resolution: with T triangles over a padded box of volume V, the grid aims at CELLS_PER_TRIANGLE * T cells of
equal edge (edge = (V / (CELLS_PER_TRIANGLE * T)) ** (1/3)), so each axis gets ceil(extent / edge) cells, at least 1
and at most MAX_CELLS_PER_AXIS.  A box scene (<= 96 triangles) gets a few hundred cells; a 50 k-triangle mesh about
100 k.

Ground truth comes from the same triangles: `ground_truth` voxelizes the surface with gnbv_voxelize_surface
(csrc/voxelize.hip) under the updater's own voxel bounds; `observable_ground_truth` restricts it to the voxels a camera
can see (gnbv_view_cover, csrc/viewcover.hip), so the coverage reward can reach 1; `surface_points` samples
the GT point cloud of the evaluation env.  env/mesh_io.py reads Wavefront OBJ files.

Collision termination uses the same triangles as closed solids: `objects` indexes them per (env, object id) -- the
objects of each env, each object's AABB and triangle list, CSR, built once with torch -- and `collide` runs
gnbv_collide_cylinder (csrc/collide.hip) for a CollisionBody (env/collision.py) at given poses.  `sweep` /
`sweep_candidates` ask the same of the straight flight between two poses (gnbv_sweep_sphere, csrc/sweep.hip), through
the cell lists alone.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

import torch

from .. import _lib
from . import synthetic as S

CELLS_PER_TRIANGLE = 2.0
MAX_CELLS_PER_AXIS = 64
EPS_REL = 1e-4  # AABB padding, relative to the env's largest extent
EPS_ABS = 1e-5  # metres, for tiny or flat scenes

# the 12 triangles of a box as corner indices (corner bit 0 = x max, bit 1 = y max, bit 2 = z max), wound
# counter-clockwise seen from outside (normal = (v1 - v0) x (v2 - v0) points out)
_BOX_TRIS = torch.tensor([
    [0, 4, 6], [0, 6, 2],  # x min
    [1, 3, 7], [1, 7, 5],  # x max
    [0, 1, 5], [0, 5, 4],  # y min
    [2, 6, 7], [2, 7, 3],  # y max
    [0, 2, 3], [0, 3, 1],  # z min
    [4, 5, 7], [4, 7, 6],  # z max
])


def box_triangles(lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """[B,3] corners -> [B*12,3,3] outward-wound triangles."""
    bits = torch.tensor([[(c >> a) & 1 for a in range(3)] for c in range(8)], dtype=torch.bool, device=lo.device)
    corners = torch.where(bits[None], hi[:, None, :], lo[:, None, :])  # [B,8,3]
    return corners[:, _BOX_TRIS.to(lo.device)].reshape(-1, 3, 3)


class MeshScene:
    """Triangles + cell lists of N envs, resident on one device (see the module docstring)."""

    def __init__(self, tris: torch.Tensor, tri_obj: torch.Tensor, tri_env: torch.Tensor, tri_count: torch.Tensor,
                 cell_lo: torch.Tensor, cell_size: torch.Tensor, cell_res: torch.Tensor, cell_base: torch.Tensor,
                 cell_start: torch.Tensor, cell_tris: torch.Tensor):
        self.tris, self.tri_obj, self.tri_env, self.tri_count = tris, tri_obj, tri_env, tri_count
        self.cell_lo, self.cell_size, self.cell_res, self.cell_base = cell_lo, cell_size, cell_res, cell_base
        self.cell_start, self.cell_tris = cell_start, cell_tris
        self.num_envs = int(cell_res.shape[0])
        self.device = tris.device
        self._objects = None

    @property
    def num_triangles(self) -> int:
        return int(self.tris.shape[0])

    def env_triangles(self, e: int):
        """(triangles [T_e,3,3], object ids [T_e]) of env e."""
        s = int(self.tri_count[:e].sum())
        k = int(self.tri_count[e])
        return self.tris[s:s + k], self.tri_obj[s:s + k]

    def c_struct(self) -> "_lib.GnbvMeshScene":
        """include/gennbv_hip.h GnbvMeshScene over this scene's tensors (they must outlive the call)."""
        s = _lib.GnbvMeshScene()
        s.n = self.num_envs
        s.tris = self.tris.data_ptr() if self.tris.numel() else None
        s.tri_obj = self.tri_obj.data_ptr() if self.tri_obj.numel() else None
        s.cell_lo, s.cell_size = self.cell_lo.data_ptr(), self.cell_size.data_ptr()
        s.cell_res, s.cell_base = self.cell_res.data_ptr(), self.cell_base.data_ptr()
        s.cell_start = self.cell_start.data_ptr()
        s.cell_tris = self.cell_tris.data_ptr() if self.cell_tris.numel() else None
        return s

    def objects(self) -> dict:
        """The per-object index of gnbv_collide_cylinder (built on the first call, then kept), tensors on the scene's device:
        env_obj_start [N+1] i32 (CSR: env e's objects), obj_id [K] i32 (ascending within an env), obj_aabb [K,6] f32
        (xmin, ymin, zmin, xmax, ymax, zmax of the object's vertices), obj_tri_start [K+1] i32 and obj_tris i32 (CSR: the
        object's triangle indices, ascending)."""
        if self._objects is None:
            dev, n, t = self.device, self.num_envs, self.num_triangles
            key = self.tri_env.to(torch.int64) * 2 ** 31 + self.tri_obj.to(torch.int64)  # (env, id) in env order, then id order
            order = torch.sort(key, stable=True).indices
            uniq, inv, counts = torch.unique_consecutive(key[order], return_inverse=True, return_counts=True)
            k = int(uniq.shape[0])
            env_of = torch.div(uniq, 2 ** 31, rounding_mode="floor")
            env_obj_start = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            env_obj_start[1:] = torch.cumsum(torch.bincount(env_of, minlength=n), 0)
            obj_tri_start = torch.zeros(k + 1, dtype=torch.int64, device=dev)
            obj_tri_start[1:] = torch.cumsum(counts, 0)
            v = self.tris[order]  # [T,3,3] in object order
            idx = inv[:, None].expand(-1, 3)
            lo = torch.full((k, 3), float("inf"), device=dev).scatter_reduce(0, idx, v.amin(1), "amin")
            hi = torch.full((k, 3), float("-inf"), device=dev).scatter_reduce(0, idx, v.amax(1), "amax")
            if t >= 2 ** 31:
                raise ValueError("MeshScene.objects: too many triangles")
            self._objects = {"env_obj_start": env_obj_start.to(torch.int32).contiguous(),
                             "obj_id": (uniq - env_of * 2 ** 31).to(torch.int32).contiguous(),
                             "obj_aabb": torch.cat([lo, hi], 1).to(torch.float32).contiguous(),
                             "obj_tri_start": obj_tri_start.to(torch.int32).contiguous(),
                             "obj_tris": order.to(torch.int32).contiguous()}
        return self._objects

    def objects_c_struct(self) -> "_lib.GnbvMeshObjects":
        """include/gennbv_hip.h GnbvMeshObjects over `objects()` (the tensors live as long as the scene)."""
        o = self.objects()
        s = _lib.GnbvMeshObjects()
        s.n, s.num_objects = self.num_envs, int(o["obj_id"].shape[0])
        s.env_obj_start, s.obj_tri_start = o["env_obj_start"].data_ptr(), o["obj_tri_start"].data_ptr()
        s.obj_aabb = o["obj_aabb"].data_ptr() if o["obj_aabb"].numel() else None
        s.obj_tris = o["obj_tris"].data_ptr() if o["obj_tris"].numel() else None
        return s

    def collide(self, poses: torch.Tensor, body, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gnbv_collide_cylinder on the current stream: contact code [N] u8 of the CollisionBody `body` (env/collision.py) at
        poses [N, >= 6] f32 (x, y, z, roll, pitch, yaw; env-local, unit row stride): bit 0 a triangle meets the body, bit 1
        none does and the centre is inside an object, bit 2 the body reaches z <= 0 (body.ground); 0 = free.  On the GPU only."""
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("MeshScene.collide runs on the GPU only (no CPU fallback): build the MeshScene on a cuda device")
        n = self.num_envs
        _lib.require_cuda(poses, out)
        assert poses.dtype == torch.float32 and poses.dim() == 2 and poses.shape[0] == n and poses.shape[1] >= 6 and poses.stride(1) == 1
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.shape == (n,) and out.is_contiguous()
        sc, ob = self.c_struct(), self.objects_c_struct()
        _lib.check(_lib.load().gnbv_collide_cylinder(C.byref(sc), C.byref(ob), poses.data_ptr(), poses.stride(0), float(body.radius),
                                                     float(body.half_length), int(bool(body.ground)), out.data_ptr(),
                                                     _lib.stream_ptr(self.device)), "gnbv_collide_cylinder")
        return out

    def collide_candidates(self, poses: torch.Tensor, body, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gnbv_collide_cylinder_batch on the current stream: contact code [N,K] u8 of `body` at poses [N, K, >= 6] f32 (unit
        element stride, rows (e, j) evenly spaced), one launch; out[e, j] == collide(poses[:, j])[e], bit for bit."""
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("MeshScene.collide_candidates runs on the GPU only (no CPU fallback): build the MeshScene on a "
                                      "cuda device")
        n = self.num_envs
        _lib.require_cuda(poses, out)
        assert poses.dtype == torch.float32 and poses.dim() == 3 and poses.shape[0] == n and poses.shape[2] >= 6 and poses.stride(2) == 1
        k = int(poses.shape[1])
        if k > 1 and n > 1 and poses.stride(0) != k * poses.stride(1):
            poses = poses.contiguous()
        row = int(poses.stride(1)) if k > 1 else int(poses.stride(0))
        if row < 6:  # a dimension of size 1 may carry any stride
            poses, row = poses.contiguous(), int(poses.shape[2])
        if out is None:
            out = torch.empty(n, k, dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.shape == (n, k) and out.is_contiguous()
        sc, ob = self.c_struct(), self.objects_c_struct()
        _lib.check(_lib.load().gnbv_collide_cylinder_batch(C.byref(sc), C.byref(ob), poses.data_ptr(), k, row, float(body.radius),
                                                           float(body.half_length), int(bool(body.ground)), out.data_ptr(),
                                                           _lib.stream_ptr(self.device)), "gnbv_collide_cylinder_batch")
        return out

    def sweep(self, from_poses: torch.Tensor, to_poses: torch.Tensor, body, episode_length: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gnbv_sweep_sphere on the current stream: path code [N] u8 of the straight flight from from_poses [N, >= 3] to
        to_poses [N, >= 3] f32 (x, y, z first; unit element stride) for the sphere of radius body.path_radius: bit 3 (8) a
        triangle comes within the radius of the segment, bit 4 (16) the swept sphere reaches z <= 0 (body.ground); 0 = free.
        episode_length [N] int64: envs with episode_length <= 1 get 0 (their pose was set, not flown to).  Equal to
        sweep_candidates(...)[:, 0], bit for bit.  On the GPU only."""
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("MeshScene.sweep runs on the GPU only (no CPU fallback): build the MeshScene on a cuda device")
        n = self.num_envs
        _lib.require_cuda(from_poses, to_poses, episode_length, out)
        assert to_poses.dtype == torch.float32 and to_poses.dim() == 2 and to_poses.shape[0] == n and to_poses.shape[1] >= 3 and to_poses.stride(1) == 1
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.shape == (n,) and out.is_contiguous()
        self.sweep_candidates(from_poses, to_poses.unsqueeze(1), body, episode_length, out.unsqueeze(1))
        return out

    def sweep_candidates(self, from_poses: torch.Tensor, to_poses: torch.Tensor, body, episode_length: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
        """gnbv_sweep_sphere on the current stream: path code [N,K] u8 of the flights to to_poses [N, K, >= 3] f32 (unit element
        stride, rows (e, j) evenly spaced) from from_poses [N, >= 3] (one start per env, broadcast over K) or [N, K, >= 3], one
        launch.  `accumulate`: OR the codes into `out` (e.g. what collide_candidates has just stored there) instead of
        storing them.  See `sweep` for the code, the radius and episode_length."""
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("MeshScene.sweep_candidates runs on the GPU only (no CPU fallback): build the MeshScene on a "
                                      "cuda device")
        n = self.num_envs
        _lib.require_cuda(from_poses, to_poses, episode_length, out)
        assert to_poses.dtype == torch.float32 and to_poses.dim() == 3 and to_poses.shape[0] == n and to_poses.shape[2] >= 3 and to_poses.stride(2) == 1
        k = int(to_poses.shape[1])
        assert from_poses.dtype == torch.float32 and from_poses.dim() in (2, 3) and from_poses.shape[0] == n and from_poses.shape[-1] >= 3
        assert from_poses.stride(-1) == 1 and (from_poses.dim() == 2 or from_poses.shape[1] == k)

        def rows(t, broadcast):  # (tensor, its strides of dim 0 and 1 in floats); a dimension of size 1 may carry any stride
            def bad(t):
                return (t.shape[0] > 1 and t.stride(0) < 3) or (t.dim() == 3 and t.shape[1] > 1 and t.stride(1) < 3 and
                                                               not (broadcast and t.stride(1) == 0))
            if bad(t):
                t = t.contiguous()
            s1 = int(t.stride(1)) if t.dim() == 3 and t.shape[1] > 1 else 0
            return t, max(int(t.stride(0)), 3), s1
        if k > 1 and n > 1 and to_poses.stride(0) != k * to_poses.stride(1):
            to_poses = to_poses.contiguous()
        to_poses, t0, t1 = rows(to_poses, False)
        row = t1 if k > 1 else t0
        from_poses, f0, f1 = rows(from_poses, True)
        if episode_length is not None:
            assert episode_length.dtype == torch.int64 and episode_length.shape == (n,) and episode_length.is_contiguous()
        if out is None:
            assert not accumulate, "accumulate needs the buffer to OR into"
            out = torch.empty(n, k, dtype=torch.uint8, device=self.device)
        assert out.dtype == torch.uint8 and out.shape == (n, k) and out.is_contiguous()
        sc = self.c_struct()
        _lib.check(_lib.load().gnbv_sweep_sphere(C.byref(sc), from_poses.data_ptr(), f0, f1, to_poses.data_ptr(), k, row,
                                                 float(body.path_radius), int(bool(body.ground)), _lib.ptr(episode_length),
                                                 int(bool(accumulate)), out.data_ptr(), _lib.stream_ptr(self.device)),
                   "gnbv_sweep_sphere")
        return out

    def flight_blocked(self, lattice, body, chunk: int = 1 << 18) -> torch.Tensor:
        """The free set of the flight search (env/flight.py FlightLattice, csrc/flight.hip): int32 [N, ceil(M / 32)], bit c of
        env e set iff the sphere of radius rho = (body.path_radius + |h| / 2) (1 + 2^-20) at node c is NOT free -- some closed
        triangle of env e lies within rho of the node, or the node lies inside a closed object, or (body.ground) z - rho <= 0.
        Padding bits are set.

        The inflation by |h| / 2 (h = the node spacing per axis) is the whole soundness argument of a lattice route: every point
        of an edge between two 26-adjacent nodes is within |h| / 2 of one of them, and every lattice pose is within |h| / 2 of its
        nearest node, so the sphere of radius path_radius flown pose -> nearest node -> free neighbours -> nearest node -> pose
        never leaves the inflated spheres of free nodes.  Conservative: gaps narrower than 2 rho are closed; no route passes that
        the swept sphere could not fly.  (1 + 2^-20 covers the rounding of rho and of the node positions to fp32.)

        Built once per scene set, in chunks of `chunk` (env, node) items, from the predicates that exist: the zero-length
        flight of sweep_candidates with sweep_radius = rho (PATH / PATH_GROUND), and the SURFACE / INSIDE bits of
        collide_candidates for the body at the node.  On the GPU only."""
        import dataclasses

        from .flight import pack_bits
        if self.device.type != "cuda":
            raise _lib.GennbvHipError("MeshScene.flight_blocked runs on the GPU only (no CPU fallback): build the MeshScene on a cuda device")
        n, m = self.num_envs, int(lattice.num_nodes)
        ball = dataclasses.replace(body, sweep=True, sweep_radius=lattice.inflated_radius(body))
        here = dataclasses.replace(body, ground=False)
        nodes = torch.zeros(m, 6, dtype=torch.float32, device=self.device)
        nodes[:, :3] = torch.as_tensor(lattice.node_positions(), device=self.device).to(torch.float32)
        blocked = torch.empty(n, m, dtype=torch.bool, device=self.device)
        step = max(1, int(chunk) // n)
        for c0 in range(0, m, step):
            rows = nodes[c0:c0 + step].unsqueeze(0).expand(n, -1, -1).contiguous()
            path = self.sweep_candidates(rows, rows, ball)
            pose = self.collide_candidates(rows, here)
            blocked[:, c0:c0 + step] = ((path & 24) | (pose & 3)) != 0
        return pack_bits(blocked, lattice.words)

    # ------------------------------------------------------------------
    @staticmethod
    def from_boxes(scene: S.Scene, device=None) -> "MeshScene":
        """12 triangles per valid box of a synthetic scene, object id = box index + 1 (synthetic.render_depth's `which`).
        Unused boxes (min > max on some axis) give no triangles."""
        dev = scene.boxes_min.device if device is None else torch.device(device)
        bmin, bmax = scene.boxes_min.to(dev, torch.float32), scene.boxes_max.to(dev, torch.float32)
        tris, ids = [], []
        for e in range(bmin.shape[0]):
            valid = (bmin[e] <= bmax[e]).all(-1)
            k = torch.nonzero(valid).flatten()
            tris.append(box_triangles(bmin[e, k], bmax[e, k]))
            ids.append((k.to(torch.int32) + 1).repeat_interleave(12))
        return MeshScene.from_triangles(tris, ids, device=dev)

    @staticmethod
    def from_triangles(tris: Sequence[torch.Tensor], ids: Sequence[torch.Tensor], device=None,
                       cells_per_triangle: float = CELLS_PER_TRIANGLE, max_cells_per_axis: int = MAX_CELLS_PER_AXIS) -> "MeshScene":
        """tris: one [T_e,3,3] float tensor per env (env-local metres), ids: one [T_e] int tensor per env (object ids > 0).
        An env may have zero triangles."""
        if len(tris) == 0 or len(tris) != len(ids):
            raise ValueError("MeshScene.from_triangles: one triangle tensor and one id tensor per env are required")
        if not 1 <= int(max_cells_per_axis) <= 1024 or not cells_per_triangle > 0:
            raise ValueError("MeshScene.from_triangles: bad cell resolution parameters")
        dev = torch.device(device) if device is not None else torch.as_tensor(tris[0]).device
        n = len(tris)
        tl, il = [], []
        for e, (t, i) in enumerate(zip(tris, ids)):
            t = torch.as_tensor(t)
            i = torch.as_tensor(i)
            if t.dim() != 3 or t.shape[1:] != (3, 3) or not t.is_floating_point():
                raise ValueError(f"env {e}: triangles must be a float [T,3,3] tensor, got {tuple(t.shape)} {t.dtype}")
            if i.shape != (t.shape[0],) or i.is_floating_point() or i.dtype == torch.bool:
                raise ValueError(f"env {e}: object ids must be an int [T] tensor matching the triangles")
            t = t.to(dev, torch.float32)
            if not torch.isfinite(t).all():
                raise ValueError(f"env {e}: triangle vertices must be finite")
            if t.shape[0] and not (int(i.min()) > 0 and int(i.max()) < 2 ** 31):
                raise ValueError(f"env {e}: object ids must be in [1, 2^31)")
            tl.append(t)
            il.append(i.to(dev, torch.int32))
        count = torch.tensor([t.shape[0] for t in tl], dtype=torch.int64)
        all_tris = torch.cat(tl, 0).contiguous() if count.sum() else torch.zeros(0, 3, 3, device=dev)
        all_ids = torch.cat(il, 0).contiguous() if count.sum() else torch.zeros(0, dtype=torch.int32, device=dev)
        tri_env = torch.repeat_interleave(torch.arange(n, device=dev), count.to(dev))
        return MeshScene._bin(all_tris, all_ids, tri_env, count, n, dev, float(cells_per_triangle), int(max_cells_per_axis))

    @staticmethod
    def _bin(tris, ids, tri_env, count, n, dev, cells_per_triangle, max_res) -> "MeshScene":
        t_total = tris.shape[0]
        tmin, tmax = tris.amin(1), tris.amax(1)  # [T,3] triangle AABBs
        big = torch.full((n, 3), float("inf"), device=dev)
        lo = big.scatter_reduce(0, tri_env[:, None].expand(-1, 3), tmin, "amin")
        hi = (-big).scatter_reduce(0, tri_env[:, None].expand(-1, 3), tmax, "amax")
        has = count.to(dev) > 0
        lo = torch.where(has[:, None], lo, torch.zeros_like(lo))
        hi = torch.where(has[:, None], hi, torch.zeros_like(hi))
        eps = (hi - lo).amax(-1) * EPS_REL + EPS_ABS  # [N]
        lo = lo - 2 * eps[:, None]
        hi = hi + 2 * eps[:, None]
        ext = hi - lo
        # cell edge from the triangle count (module docstring), res = ceil(extent / edge) clamped to [1, max_res]
        vol = ext.double().prod(-1)
        edge = (vol / (cells_per_triangle * count.to(dev).double().clamp(min=1))).pow(1.0 / 3.0)
        res = torch.ceil(ext.double() / edge[:, None]).clamp(1, max_res).to(torch.int64)
        res = torch.where(has[:, None], res, torch.zeros_like(res))
        size = torch.where(has[:, None], ext / res.clamp(min=1).to(torch.float32), torch.ones_like(ext))
        ncell = res.prod(-1)
        total_cells = int(ncell.sum())
        if total_cells >= 2 ** 31:
            raise ValueError("MeshScene: too many cells")
        base = torch.cumsum(ncell, 0) - ncell
        # the cell range of each triangle's padded AABB
        if t_total:
            e_lo, e_sz, e_res, e_eps = lo[tri_env], size[tri_env], res[tri_env], eps[tri_env, None]
            i0 = torch.floor((tmin - e_eps - e_lo) / e_sz).to(torch.int64).clamp(min=0)
            i1 = torch.floor((tmax + e_eps - e_lo) / e_sz).to(torch.int64)
            i1 = torch.minimum(i1, e_res - 1)
            i0 = torch.minimum(i0, i1)
            span = i1 - i0 + 1  # [T,3]
            per_tri = span.prod(-1)
            entries = int(per_tri.sum())
            if entries >= 2 ** 31:
                raise ValueError("MeshScene: too many cell entries")
            tri_of = torch.repeat_interleave(torch.arange(t_total, device=dev), per_tri)
            k = torch.arange(entries, device=dev) - (torch.cumsum(per_tri, 0) - per_tri)[tri_of]
            sp = span[tri_of]
            cx = i0[tri_of, 0] + k % sp[:, 0]
            cy = i0[tri_of, 1] + (k // sp[:, 0]) % sp[:, 1]
            cz = i0[tri_of, 2] + k // (sp[:, 0] * sp[:, 1])
            r = res[tri_env[tri_of]]
            cell = base[tri_env[tri_of]] + cx + r[:, 0] * (cy + r[:, 1] * cz)
            order = torch.argsort(cell * max(t_total, 1) + tri_of)  # by cell, triangles ascending inside a cell
            cell_tris = tri_of[order].to(torch.int32).contiguous()
            counts = torch.bincount(cell, minlength=total_cells)
        else:
            cell_tris = torch.zeros(0, dtype=torch.int32, device=dev)
            counts = torch.zeros(total_cells, dtype=torch.int64, device=dev)
        cell_start = torch.zeros(total_cells + 1, dtype=torch.int64, device=dev)
        cell_start[1:] = torch.cumsum(counts, 0)
        return MeshScene(tris.reshape(-1, 3, 3).contiguous(), ids.contiguous(), tri_env, count,
                         lo.to(torch.float32).contiguous(), size.to(torch.float32).contiguous(), res.to(torch.int32).contiguous(),
                         base.to(torch.int32).contiguous(), cell_start.to(torch.int32).contiguous(), cell_tris)

    # ------------------------------------------------------------------
    def grid_spec(self, grid_size: int, range_gt: Optional[torch.Tensor] = None):
        """(range_gt [N,6], voxel_size [N,3]) f32 on the CPU for a G^3 ground-truth grid.  range_gt = (xmax, xmin, ymax,
        ymin, zmax, zmin) of the voxel centres; voxel_size = range / (G - 1) per axis (env_train_gennbv.py:67-80).
        Without range_gt each env's follows the reference's frame: xmax = -xmin = max |x|, the same for y, zmax = max z,
        zmin = 0; an env without triangles or with zero extent on an axis then needs an explicit range_gt."""
        g = int(grid_size)
        if not 2 <= g <= 1024:
            raise ValueError(f"grid_size must be in [2, 1024], got {grid_size}")
        n = self.num_envs
        if range_gt is None:
            rows = []
            for e in range(n):
                t = self.env_triangles(e)[0].detach().to("cpu", torch.float32).reshape(-1, 3)
                if t.shape[0] == 0:
                    raise ValueError(f"env {e} has no triangles: pass range_gt explicitly")
                mx, my, mz = float(t[:, 0].abs().max()), float(t[:, 1].abs().max()), float(t[:, 2].max())
                if not (mx > 0 and my > 0 and mz > 0):
                    raise ValueError(f"env {e} has zero extent on an axis (max|x| {mx}, max|y| {my}, max z {mz}): "
                                     "pass range_gt explicitly")
                rows.append([mx, -mx, my, -my, mz, 0.0])
            rng = torch.tensor(rows, dtype=torch.float32)
        else:
            rng = torch.as_tensor(range_gt).detach().to("cpu", torch.float32)
            if rng.shape != (n, 6):
                raise ValueError(f"range_gt must be [{n}, 6], got {tuple(rng.shape)}")
        vox = torch.stack([rng[:, 0] - rng[:, 1], rng[:, 2] - rng[:, 3], rng[:, 4] - rng[:, 5]], -1) / (g - 1)
        if not (torch.isfinite(rng).all() and torch.isfinite(vox).all() and (vox > 0).all()):
            raise ValueError("range_gt must be finite with max > min on every axis")
        return rng.contiguous(), vox.contiguous()

    def ground_truth(self, grid_size: int, range_gt: Optional[torch.Tensor] = None,
                     env_origins: Optional[torch.Tensor] = None) -> S.Scene:
        """The env's ground truth as a synthetic.Scene: grid_gt [N,G,G,G] f32 = the surface voxels of the triangles
        (gnbv_voxelize_surface), range_gt / voxel_size from grid_spec, num_valid_voxel_gt = the voxel count (at least 1),
        no boxes ([N,0,3], like feed_file.load_scene), env_origins the caller's or make_scenes' layout.  On the GPU only."""
        rng, vox = self.grid_spec(grid_size, range_gt)
        g, n, dev = int(grid_size), self.num_envs, self.device
        if dev.type != "cuda":
            raise _lib.GennbvHipError("MeshScene.ground_truth voxelizes on the GPU only (no CPU fallback): "
                                      "build the MeshScene on a cuda device")
        if env_origins is None:
            env_origins = S.default_env_origins(n)
        env_origins = torch.as_tensor(env_origins).to(dev, torch.float32)
        if env_origins.shape != (n, 3):
            raise ValueError(f"env_origins must be [{n}, 3], got {tuple(env_origins.shape)}")
        rng_d, vox_d = rng.to(dev), vox.to(dev)
        grid = torch.empty(n, g, g, g, dtype=torch.float32, device=dev)
        self.voxelize_into(grid, rng_d, vox_d)
        empty = torch.zeros(n, 0, 3, dtype=torch.float32, device=dev)
        return S.Scene(empty, empty.clone(), grid, rng_d, vox_d, grid.sum(dim=(1, 2, 3)).clamp(min=1.0), env_origins.contiguous())

    def observable_ground_truth(self, grid_size: int, poses: torch.Tensor, cfg, range_gt: Optional[torch.Tensor] = None,
                                base: Optional[S.Scene] = None, inv_intrinsics: Optional[torch.Tensor] = None,
                                env_origins: Optional[torch.Tensor] = None, batch: int = 64) -> S.Scene:
        """The ground truth a camera can see: `base` (a synthetic.Scene to restrict, e.g. make_scenes' own GT; default
        `self.ground_truth(grid_size, range_gt, env_origins)`; with `base` the voxel frame is base's and `range_gt` is refused) with grid_gt = base.grid_gt AND (voxels the voxel update
        marks from at least one of poses [N,K,6] f32, env-local, at stride 1 with cfg's camera: gnbv_view_cover's seen
        set); num_valid_voxel_gt = its count (at least 1); everything else as in `base`.  Surface voxels no camera
        reaches -- faces lying on the ground, faces buried in another object, the insides of closed shells -- leave the
        coverage denominator, so a perfect planner's coverage is 1.  This is a LOWER BOUND of the truly observable set
        that grows with the view set: a voxel only seen from a pose outside `poses` is dropped.  The intended view set is
        eval.baselines.LatticeCandidates(cfg, k, seed, look_at_scene=True) with a few hundred views per env.  K may be
        large: the candidates run in batches of `batch`.  On the GPU only."""
        import dataclasses

        from ..ops.view_cover import ViewCover
        g, n, dev = int(grid_size), self.num_envs, self.device
        if dev.type != "cuda":
            raise _lib.GennbvHipError("MeshScene.observable_ground_truth runs on the GPU only (no CPU fallback): "
                                      "build the MeshScene on a cuda device")
        if base is None:
            base = self.ground_truth(g, range_gt, env_origins)
        elif range_gt is not None:
            raise ValueError("observable_ground_truth: pass either base (its own range_gt / voxel_size are used) or range_gt, not both")
        grid = base.grid_gt.to(dev, torch.float32).contiguous()
        if grid.shape != (n, g, g, g):
            raise ValueError(f"base.grid_gt must be [{n}, {g}, {g}, {g}], got {tuple(grid.shape)}")
        poses = torch.as_tensor(poses).to(dev, torch.float32)
        if poses.dim() != 3 or poses.shape[0] != n or poses.shape[2] != 6 or poses.shape[1] < 1:
            raise ValueError(f"poses must be [{n}, K, 6] with K >= 1, got {tuple(poses.shape)}")
        if int(cfg.grid_size) != g:
            cfg = dataclasses.replace(cfg, grid_size=g)
        rng_d = base.range_gt.to(dev, torch.float32).contiguous()  # the frame is base's, whole
        vox_d = base.voxel_size.to(dev, torch.float32).contiguous()
        lib, st = _lib.load(), _lib.stream_ptr(dev)
        words = int(lib.gnbv_grid_bit_words(g))
        gt_bits = torch.zeros(n, words, dtype=torch.int32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.gnbv_pack_grid_bits(grid.data_ptr(), n, g, gt_bits.data_ptr(), flag.data_ptr(), st), "gnbv_pack_grid_bits")
        if int(flag.item()) != 0:
            raise ValueError("observable_ground_truth needs a binary base.grid_gt (0 / 1)")
        seen = torch.zeros_like(gt_bits)
        k, batch = int(poses.shape[1]), max(1, int(batch))
        ops = {}
        for j0 in range(0, k, batch):
            kb = min(batch, k - j0)
            if kb not in ops:
                ops[kb] = ViewCover(self, cfg, rng_d, vox_d, kb, stride=1, inv_intrinsics=inv_intrinsics, device=dev)
            ops[kb].accumulate(poses[:, j0:j0 + kb].contiguous(), gt_bits, seen)
        out = torch.empty_like(grid)
        _lib.check(lib.gnbv_unpack_grid_bits(seen.data_ptr(), n, g, out.data_ptr(), st), "gnbv_unpack_grid_bits")
        origins = base.env_origins if env_origins is None else torch.as_tensor(env_origins)
        return S.Scene(base.boxes_min.to(dev), base.boxes_max.to(dev), out, rng_d, vox_d, out.sum(dim=(1, 2, 3)).clamp(min=1.0),
                       origins.to(dev, torch.float32).contiguous())

    def voxelize_into(self, grid_out: torch.Tensor, range_gt: torch.Tensor, voxel_size: torch.Tensor) -> torch.Tensor:
        """gnbv_voxelize_surface on the current stream: grid_out [N,G,G,G] f32 (every voxel written), range_gt [N,6] and
        voxel_size [N,3] f32 on the scene's device."""
        _lib.require_cuda(grid_out, range_gt, voxel_size)
        n = self.num_envs
        assert grid_out.dtype == torch.float32 and grid_out.is_contiguous() and grid_out.dim() == 4 and grid_out.shape[0] == n
        assert range_gt.dtype == torch.float32 and range_gt.is_contiguous() and range_gt.shape == (n, 6)
        assert voxel_size.dtype == torch.float32 and voxel_size.is_contiguous() and voxel_size.shape == (n, 3)
        sc = self.c_struct()
        _lib.check(_lib.load().gnbv_voxelize_surface(C.byref(sc), range_gt.data_ptr(), voxel_size.data_ptr(), int(grid_out.shape[1]),
                                                     grid_out.data_ptr(), _lib.stream_ptr(self.device)), "gnbv_voxelize_surface")
        return grid_out

    def surface_points(self, per_env: int, seed: int = 0) -> List[torch.Tensor]:
        """per_env points [per_env,3] f32 per env, uniform over the env's surface: triangles drawn with probability
        proportional to area, then a uniform point on the triangle.  One seeded CPU generator in env order, fp64
        arithmetic: the cloud is the same on every device.  An env without triangles gets [0,3]; an env whose triangles
        all have zero area draws them uniformly.  The GT cloud (pc_gt) of ReplayFeedEvalEnv."""
        if int(per_env) < 0:
            raise ValueError("per_env must be >= 0")
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        out = []
        for e in range(self.num_envs):
            t = self.env_triangles(e)[0].detach().to("cpu", torch.float64)
            if t.shape[0] == 0 or per_env == 0:
                out.append(torch.zeros(0, 3, dtype=torch.float32, device=self.device))
                continue
            area = 0.5 * torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], dim=-1).norm(dim=-1)
            w = area if float(area.sum()) > 0 else torch.ones_like(area)
            k = torch.multinomial(w, int(per_env), replacement=True, generator=gen)
            r = torch.rand(int(per_env), 2, generator=gen, dtype=torch.float64)
            s = r[:, :1].sqrt()
            a, b, c = t[k, 0], t[k, 1], t[k, 2]
            p = (1.0 - s) * a + (s * (1.0 - r[:, 1:])) * b + (s * r[:, 1:]) * c
            out.append(p.to(self.device, torch.float32).contiguous())
        return out

    def cell_box(self, e: int, c: int):
        """(lo, hi) [3] of local cell index c (x fastest) of env e."""
        r = self.cell_res[e].tolist()
        ijk = torch.tensor([c % r[0], (c // r[0]) % r[1], c // (r[0] * r[1])], dtype=torch.float32, device=self.device)
        lo = self.cell_lo[e] + ijk * self.cell_size[e]
        return lo, lo + self.cell_size[e]


def sphere_triangles(centre: Sequence[float], radius: float, n_lat: int = 12, n_lon: int = 24) -> torch.Tensor:
    """A closed UV sphere as [T,3,3] outward-wound triangles, T = 2 * n_lon * (n_lat - 1) (test scenes, dense benchmark)."""
    th = torch.linspace(0, math.pi, n_lat + 1, dtype=torch.float64)
    ph = torch.linspace(0, 2 * math.pi, n_lon + 1, dtype=torch.float64)[:-1]
    pts = torch.stack([torch.sin(th)[:, None] * torch.cos(ph)[None], torch.sin(th)[:, None] * torch.sin(ph)[None],
                       torch.cos(th)[:, None].expand(-1, n_lon)], -1) * radius + torch.tensor(centre, dtype=torch.float64)
    i = torch.arange(n_lat)[:, None].expand(-1, n_lon)
    j = torch.arange(n_lon)[None, :].expand(n_lat, -1)
    j1 = (j + 1) % n_lon
    a, b, c, d = pts[i, j], pts[i, j1], pts[i + 1, j], pts[i + 1, j1]  # [n_lat, n_lon, 3]
    upper = torch.stack([a, c, b], -2)[1:]  # the pole rows have one triangle per quad
    lower = torch.stack([b, c, d], -2)[:-1]
    return torch.cat([upper.reshape(-1, 3, 3), lower.reshape(-1, 3, 3)]).float()


def random_rotation(generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """A uniformly random 3x3 rotation (QR of a Gaussian matrix)."""
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=generator, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))[None]
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q

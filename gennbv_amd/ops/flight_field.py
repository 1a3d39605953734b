"""FlightField: the shortest collision-free route over the flight lattice, per env (csrc/flight.hip).

    field = FlightField(mesh, FlightLattice(cfg, stride=2), body)
    field.update(poses)            # one launch: the distance in mm from each env's pose to every lattice node
    field.cost(targets)            # f32 [N,K] metres (inf: no route), field.cost_mm(targets) the raw u32 of the nodes
    field.path(targets)            # the waypoints of one route per env
    field.pairwise_mm(points)      # int32 [N,P,P] u32 mm between every two of P points (a private field: update() state untouched)

It owns the blocked bits (MeshScene.flight_blocked: built once from the mesh) and the field [N, M] u32.  A route goes
pose -> its nearest node -> free 26-neighbours -> the target's nearest node -> target; `cost` is the integer lattice distance
in metres plus the two stub legs pose <-> node.  Every leg is flyable by the sphere of radius body.path_radius (env/flight.py
has the argument).  `mode`: 0 auto, 1 the field resident in LDS (refused where it does not fit), 2 the field in global memory.
The sweep count of the field kernel has a hard cap; an env that hit it is reported lazily, by `check()` (one read-back) and
by `path()`, the way ScanAccumulator reports its flags.  GPU only.

BeliefFlightField is the same field over the agent's own map: its blocked bits are recomputed every step from the tri-class
grid (csrc/flightmap.hip) and no mesh is consulted.  With `shortcut=True` it also keeps a snapshot of that map and judges straight
legs on it (`sweep`: gnbv_sweep_tri, csrc/sweepmap.hip).  With `unknown="costly"` unknown space is flyable at a price: the nodes
whose ball touches an unknown voxel cost `unknown_penalty_m` more to enter (gnbv_flight_classify_tri, gnbv_flight_field_w,
gnbv_flight_path_w).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib
from ..env.flight import INF_MM


class FlightField:
    def __init__(self, mesh, lattice, body, mode: int = 0, blocked: Optional[torch.Tensor] = None):
        if mesh.device.type != "cuda":
            raise _lib.GennbvHipError("FlightField runs on the GPU only (no CPU fallback): build the MeshScene on a cuda device")
        if int(mode) not in (0, 1, 2):
            raise ValueError(f"FlightField: mode must be 0, 1 or 2, got {mode}")
        self.lib = _lib.load()
        self.mesh, self.lattice, self.body, self.mode = mesh, lattice, body, int(mode)
        self.device = mesh.device
        self.num_envs = n = int(mesh.num_envs)
        m = int(lattice.num_nodes)
        if self.mode == 1 and m > int(self.lib.gnbv_flight_lds_max_nodes()):
            raise _lib.GennbvHipError(f"FlightField: a field of {m} nodes does not fit LDS (mode 1)")
        self.blocked = mesh.flight_blocked(lattice, body) if blocked is None else blocked
        assert self.blocked.dtype == torch.int32 and self.blocked.shape == (n, lattice.words) and self.blocked.is_contiguous()
        _lib.require_cuda(self.blocked)
        self.field = torch.full((n, m), -1, dtype=torch.int32, device=self.device)  # u32 bits; all INF_MM until update()
        self.status = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.source = torch.full((n, 3), float("nan"), dtype=torch.float32, device=self.device)  # the poses of the last update
        self._cost = (C.c_uint32 * 8)(*[int(c) for c in lattice.cost])
        self._lo = (C.c_double * 3)(*[float(v) for v in lattice.lo])
        self._h = (C.c_double * 3)(*[float(v) for v in lattice.h])
        self.launches = 0  # field launches so far
        # a field with a price on some nodes (BeliefFlightField, unknown="costly"): their bits [N, words] and the price; None keeps
        # every launch the plain one
        self.costly, self.penalty_mm = None, 0
        # pairwise_mm: its private field (shares `blocked`), its sticky device flags (1 sweep cap, 2 a sum too wide), its buffers per P
        self._pair, self._pair_status, self._pair_rows, self._pair_out = None, None, {}, {}

    # ------------------------------------------------------------------
    def update(self, poses: torch.Tensor) -> "FlightField":
        """gnbv_flight_field on the current stream from poses [N, >= 3] f32 (unit element stride)."""
        n = self.num_envs
        _lib.require_cuda(poses)
        assert poses.dtype == torch.float32 and poses.dim() == 2 and poses.shape[0] == n and poses.shape[1] >= 3 and poses.stride(1) == 1
        nx, ny, nz = self.lattice.dims
        self.source.copy_(poses[:, :3])
        tail = (self._cost, poses.data_ptr(), max(int(poses.stride(0)), 3), self._lo, self._h, self.field.data_ptr(), self.status.data_ptr(),
                self.mode, _lib.stream_ptr(self.device))
        if self.costly is None:
            _lib.check(self.lib.gnbv_flight_field(self.blocked.data_ptr(), n, nx, ny, nz, *tail), "gnbv_flight_field")
        else:
            _lib.check(self.lib.gnbv_flight_field_w(self.blocked.data_ptr(), self.costly.data_ptr(), self.penalty_mm, n, nx, ny, nz, *tail),
                       "gnbv_flight_field_w")
        self.launches += 1
        return self

    def check(self):
        """Raise if the field kernel's sweep cap ended an env's relaxation (one device -> host copy), here or in a field of
        pairwise_mm, or if a pairwise_mm sum did not fit."""
        bad = torch.nonzero(self.status).flatten().tolist()
        if bad:
            raise _lib.GennbvHipError(f"FlightField: the relaxation of envs {bad[:8]} hit the sweep cap; their fields are not settled")
        if self._pair_status is not None:
            st = self._pair_status.tolist()
            capped, wide = [e for e, s in enumerate(st) if s & 1], [e for e, s in enumerate(st) if s & 2]
            if capped:
                raise _lib.GennbvHipError(f"FlightField.pairwise_mm: the relaxation of envs {capped[:8]} hit the sweep cap")
            if wide:
                raise _lib.GennbvHipError(f"FlightField.pairwise_mm: a route of envs {wide[:8]} with its stubs does not fit 32 bits of "
                                          "millimetres (entries set to 0xFFFFFFFF)")

    def pairwise_mm(self, points: torch.Tensor, count: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [N,P,P] of u32 bits: the length in mm of the shortest route between every two of points [N, P, >= 3] f32.
        Inside count[e] (int32 [N], 1..P; None: P):  out[e,a,a] = 0;  out[e,a,b] = field_mm(node(a) -> node(b)) + stub(a) + stub(b),
        stub(p) = rint(1000 * ||p - its nearest node||) in fp64, summed in 64 bits; 0xFFFFFFFF where no route exists (either node
        blocked, absent or cut off).  A point without a node (a non-finite coordinate) holds 0xFFFFFFFF in its whole row and
        column, the diagonal included.  Rows and columns at or above count[e] hold 0xFFFFFFFF.  Symmetric: the lattice is
        undirected and the distances exact integers.
        P field launches from points[:, s], each followed by one query of all P points, on a private field that shares
        `blocked`: `field`, `source`, `status` and `launches` of this object are not touched.  A sweep cap in one of those
        fields, or a sum that does not stay below 0xFFFFFFFE (the entry is then 0xFFFFFFFF), is kept in a device flag and raised
        by the next check().  The result buffer is reused per P.  No host synchronisation."""
        n = self.num_envs
        _lib.require_cuda(points, count)
        if points.dtype != torch.float32 or points.dim() != 3 or points.shape[0] != n or points.shape[2] < 3 or points.shape[1] < 1:
            raise _lib.GennbvHipError(f"FlightField.pairwise_mm: points must be float32 [{n}, P, >= 3], got {points.dtype} {tuple(points.shape)}")
        p = int(points.shape[1])
        if count is not None and (count.dtype != torch.int32 or count.shape != (n,)):
            raise _lib.GennbvHipError(f"FlightField.pairwise_mm: count must be int32 [{n}], got {count.dtype} {tuple(count.shape)}")
        if self._pair is None:
            self._pair = FlightField(self.mesh, self.lattice, self.body, mode=self.mode, blocked=self.blocked)
            self._pair_status = torch.zeros(n, dtype=torch.int32, device=self.device)
        scratch = self._pair
        if p not in self._pair_rows:
            self._pair_rows[p] = torch.empty(p, n, p, dtype=torch.int32, device=self.device)
        rows = self._pair_rows[p]
        pts = points if points.stride(2) == 1 else points.contiguous()
        for s in range(p):
            scratch.update(pts[:, s])
            scratch.cost_mm(pts, out=rows[s])
            self._pair_status |= scratch.status
        lat = self.lattice
        q = pts[..., :3].to(torch.float64)
        d = q - lat.nearest_positions(q)
        stub = torch.round(1000.0 * torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))  # NaN: no node
        has_node = torch.isfinite(stub)
        stub = torch.where(has_node, stub, torch.zeros_like(stub)).clamp(max=float(2 ** 40)).to(torch.int64)
        mm = rows.permute(1, 0, 2).to(torch.int64) & 0xFFFFFFFF
        routed = mm != INF_MM
        total = mm + stub[:, :, None] + stub[:, None, :]
        fits = total < INF_MM - 1
        self._pair_status |= (routed & ~fits).flatten(1).any(dim=1).to(torch.int32) * 2
        eye = torch.eye(p, dtype=torch.bool, device=self.device)[None]
        total = torch.where(eye & has_node[:, :, None], torch.zeros_like(total), torch.where(routed & fits, total, torch.full_like(total, INF_MM)))
        if count is not None:
            inside = torch.arange(p, device=self.device)[None] < count[:, None]
            total = torch.where(inside[:, :, None] & inside[:, None, :], total, torch.full_like(total, INF_MM))
        out = self._pair_out.get(p)
        if out is None:
            out = self._pair_out[p] = torch.empty(n, p, p, dtype=torch.int32, device=self.device)
        out.copy_(torch.where(total >= 2 ** 31, total - 2 ** 32, total))
        return out

    def _targets(self, targets: torch.Tensor):
        n = self.num_envs
        _lib.require_cuda(targets)
        assert targets.dtype == torch.float32 and targets.dim() == 3 and targets.shape[0] == n and targets.shape[2] >= 3 and targets.stride(2) == 1
        k = int(targets.shape[1])
        if k > 1 and n > 1 and targets.stride(0) != k * targets.stride(1):
            targets = targets.contiguous()
        row = int(targets.stride(1)) if k > 1 else int(targets.stride(0))
        if row < 3:  # a dimension of size 1 may carry any stride
            targets, row = targets.contiguous(), int(targets.shape[2])
        return targets, k, row

    def cost_mm(self, targets: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gnbv_flight_query: int32 [N,K] holding the u32 field value (mm) at the nearest node of targets [N, K, >= 3] f32;
        -1 (0xFFFFFFFF) = blocked, unreachable or no node.  Over a field with a price on unknown space (`costly`) the value holds
        the penalties of the costly nodes entered: it is a cost, not a length."""
        targets, k, row = self._targets(targets)
        n = self.num_envs
        if out is None:
            out = torch.empty(n, k, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.shape == (n, k) and out.is_contiguous()
        nx, ny, nz = self.lattice.dims
        _lib.check(self.lib.gnbv_flight_query(self.field.data_ptr(), n, nx, ny, nz, self._lo, self._h, targets.data_ptr(), k, row,
                                              out.data_ptr(), _lib.stream_ptr(self.device)), "gnbv_flight_query")
        return out

    def cost(self, targets: torch.Tensor) -> torch.Tensor:
        """f32 [N,K]: the length in metres of the route from the poses of the last update() to targets [N, K, >= 3] -- the stub
        from the pose to its node, the lattice distance, the stub from the target's node to the target -- or inf.  Over a field
        with a price on unknown space (`costly`) the lattice term is the penalised value: metres flown plus `unknown_penalty_m` per
        costly node entered."""
        mm = self.cost_mm(targets)
        lat = self.lattice
        t = targets[..., :3].to(torch.float64)
        s = self.source.to(torch.float64)
        stub = (t - lat.nearest_positions(t)).norm(dim=-1) + (s - lat.nearest_positions(s)).norm(dim=-1)[:, None]
        metres = (mm.to(torch.float64) * 1e-3 + stub).to(torch.float32)
        return torch.where(mm == -1, torch.full_like(metres, float("inf")), metres)

    def reachable(self, targets: torch.Tensor) -> torch.Tensor:
        """bool [N,K]: a route over non-blocked nodes exists from the poses of the last update() to each target."""
        return self.cost_mm(targets) != -1

    def path(self, targets: torch.Tensor, max_len: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """gnbv_flight_path for one target per env, targets [N, >= 3] f32 -> (waypoints f32 [N, L, 3], length int32 [N]): the
        route from the pose of the last update() to the target, both end poses included (length = nodes + 2), rows past the
        length NaN; length 0 and all NaN where there is no route.  Synchronises with the host (the length decides the shape);
        not for the hot path.  Raises where an env's field is not settled."""
        n = self.num_envs
        _lib.require_cuda(targets)
        assert targets.dtype == torch.float32 and targets.dim() == 2 and targets.shape[0] == n and targets.shape[1] >= 3 and targets.stride(1) == 1
        self.check()
        nodes, count = self.path_nodes(targets, max_len)
        longest = max(int(count.max()), 0)
        pos = torch.as_tensor(self.lattice.node_positions(), device=self.device).to(torch.float32)
        way = torch.full((n, longest + 2, 3), float("nan"), dtype=torch.float32, device=self.device)
        if longest:
            j = torch.arange(longest, device=self.device)[None]
            valid = j < count[:, None]
            back = (count[:, None].long() - 1 - j).clamp(min=0)  # nodes run target -> source: waypoint 1 + j is node count - 1 - j
            ids = nodes[:, :longest].long().gather(1, back).clamp(min=0)
            way[:, 1:1 + longest] = torch.where(valid[..., None], pos[ids], way[:, 1:1 + longest])
        ok = count > 0
        way[:, 0] = torch.where(ok[:, None], self.source, way[:, 0])
        rows = torch.nonzero(ok).flatten()
        way[rows, 1 + count[rows].long()] = targets[rows, :3]
        return way, torch.where(ok, count + 2, torch.zeros_like(count))

    def path_into(self, targets: torch.Tensor, nodes_out: torch.Tensor, len_out: torch.Tensor):
        """One gnbv_flight_path (with `costly`: gnbv_flight_path_w) launch into the caller's buffers: nodes_out int32 [N, L], len_out int32 [N] (0 no route, -needed where
        L is too short).  No host synchronisation."""
        n = self.num_envs
        nx, ny, nz = self.lattice.dims
        _lib.require_cuda(targets, nodes_out, len_out)
        assert targets.dtype == torch.float32 and targets.dim() == 2 and targets.shape[0] == n and targets.shape[1] >= 3 and targets.stride(1) == 1
        assert nodes_out.dtype == torch.int32 and nodes_out.dim() == 2 and nodes_out.shape[0] == n and nodes_out.is_contiguous()
        assert len_out.dtype == torch.int32 and len_out.shape == (n,) and len_out.is_contiguous()
        tail = (n, nx, ny, nz, self._cost, self._lo, self._h, targets.data_ptr(), max(int(targets.stride(0)), 3), nodes_out.data_ptr(),
                int(nodes_out.shape[1]), len_out.data_ptr(), _lib.stream_ptr(self.device))
        if self.costly is None:
            _lib.check(self.lib.gnbv_flight_path(self.field.data_ptr(), *tail), "gnbv_flight_path")
        else:
            _lib.check(self.lib.gnbv_flight_path_w(self.field.data_ptr(), self.costly.data_ptr(), self.penalty_mm, *tail), "gnbv_flight_path_w")

    def path_nodes(self, targets: torch.Tensor, max_len: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The raw walk: (nodes int32 [N, L] from the target's node back to the source, count int32 [N]; 0 = no route).  Runs the
        kernel again with a longer buffer where the first was too short (a host read-back of the counts)."""
        n = self.num_envs
        nx, ny, nz = self.lattice.dims
        length = int(max_len) if max_len is not None else max(2 * (nx + ny + nz), 8)
        while True:
            nodes = torch.full((n, length), -1, dtype=torch.int32, device=self.device)
            count = torch.zeros(n, dtype=torch.int32, device=self.device)
            self.path_into(targets, nodes, count)
            need = -int(count.min())
            if need <= 0:
                return nodes, count
            length = need


class BeliefFlightField(FlightField):
    """The flight field over the map the agent has scanned so far: the blocked bits come from each env's tri-class grid
    (gnbv_flight_blocked_tri, csrc/flightmap.hip), not from a mesh -- the pilot that knows only what it has seen.

        field = BeliefFlightField(num_envs, lattice, body, range_gt, voxel_size, grid_size)
        field.refresh(tri)     # one launch: the grid (int8 rows, or the fp32 grid slice of observation rows) -> blocked_map
        field.update(poses)    # blocked = blocked_map with each env's own node cleared, then the field launch

    A node is blocked where the ball of radius rho = lattice.inflated_radius(body) + margin touches an occupied voxel
    (`unknown="blocked"`: or an unknown one, the conservative pilot; the default "free" is the optimistic one; "costly" below), with
    `outside="blocked"` where it leaves the grid (range_gt bounds every solid of a scene by grid_spec's construction, hence the
    default "free"), and with body.ground where it reaches z <= 0.  The drone is at its own nearest node, so update() calls
    that node flyable whatever the map says; `blocked_map` stays the pure kernel output.  `map_mode`: 0 auto, 1 the grid's
    bits packed into LDS (refused where they do not fit), 2 the grid read from global memory.  GPU only.

    `shortcut=True` adds the straight leg judged on the map: refresh() also keeps `map_i8` [N, G^3] int8, a snapshot of the map
    (int8 rows copied, fp32 rows as their sign -- the buffer the map was written to may be reused before the env flies, and the
    pilot's knowledge must not alias it), and `sweep` moves the sphere of radius `sweep_radius` = body.path_radius +
    shortcut_margin along straight legs over it (a lattice node needs the inflated rho so that its edges are safe; a straight leg
    needs only the body's own radius).  `sweeps` counts those launches.  With shortcut=False nothing is allocated or launched
    that was not before.

    `unknown="costly", unknown_penalty_m=<metres>` is the cautious pilot: unknown space is flyable but expensive.  refresh() is one
    gnbv_flight_classify_tri launch into `blocked_map` (occupied, outside, ground: what "free" blocks) and `costly_map` (not blocked,
    the ball touches an unknown voxel); update() clears the drone's own node in `blocked` only and launches gnbv_flight_field_w with
    penalty_mm = rint(1000 * unknown_penalty_m) per costly node entered, and the path methods walk with gnbv_flight_path_w.
    `cost_mm` / `cost` then hold penalties; `reachable` and `pairwise_mm` (the plain kernel over `blocked`: geometric lengths) do
    not.  `sweep` and the shortcut judge straight legs with unknown voxels blocking: the cautious pilot cuts corners only
    through space it has seen.  There is no default penalty: nobody has measured one.  With any other `unknown` nothing is
    allocated or launched that was not before."""
    belief = True

    def __init__(self, num_envs: int, lattice, body, range_gt: torch.Tensor, voxel_size: torch.Tensor, grid_size: int,
                 unknown: str = "free", outside: str = "free", margin: float = 0.0, mode: int = 0, map_mode: int = 0, device="cuda:0",
                 shortcut: bool = False, shortcut_margin: float = 0.0, unknown_penalty_m: Optional[float] = None):
        import types
        device = torch.device(device)
        if unknown not in ("free", "blocked", "costly"):
            raise ValueError(f"BeliefFlightField: unknown must be 'free', 'blocked' or 'costly', got {unknown!r}")
        if outside not in ("free", "blocked"):
            raise ValueError(f"BeliefFlightField: outside must be 'free' or 'blocked', got {outside!r}")
        penalty_mm = 0
        if unknown == "costly":
            if unknown_penalty_m is None or not np.isfinite(float(unknown_penalty_m)) or not float(unknown_penalty_m) > 0.0:
                raise ValueError(f"BeliefFlightField: unknown='costly' needs a finite unknown_penalty_m > 0, got {unknown_penalty_m!r}")
            penalty_mm = int(np.rint(1000.0 * float(unknown_penalty_m)))
            # the bound of gnbv_flight_field_w: every route's cost must stay below 0xFFFFFFFE
            if penalty_mm < 1 or int(lattice.num_nodes) * (int(max(lattice.cost)) + penalty_mm) >= INF_MM - 1:
                raise ValueError(f"BeliefFlightField: unknown_penalty_m = {unknown_penalty_m} gives {penalty_mm} mm, outside what "
                                 f"{lattice.num_nodes} nodes admit (M * (max edge cost + penalty) < 0xFFFFFFFE, at least 1 mm)")
        elif unknown_penalty_m is not None:
            raise ValueError("BeliefFlightField: unknown_penalty_m goes with unknown='costly' only")
        if int(map_mode) not in (0, 1, 2):
            raise ValueError(f"BeliefFlightField: map_mode must be 0, 1 or 2, got {map_mode}")
        n, g = int(num_envs), int(grid_size)
        if not 1 <= g <= 128:
            raise ValueError(f"BeliefFlightField: grid_size must be in 1..128, got {grid_size}")
        self.shortcut = bool(shortcut)
        self.sweep_radius = float(body.path_radius) + float(shortcut_margin)
        if not (np.isfinite(self.sweep_radius) and self.sweep_radius > 0.0):
            raise ValueError(f"BeliefFlightField: the path radius plus shortcut_margin must be finite and > 0, got {self.sweep_radius}")
        if device.type != "cuda":
            raise _lib.GennbvHipError("BeliefFlightField runs on the GPU only (no CPU fallback)")
        lib = _lib.load()
        cautious = unknown == "costly"
        if int(map_mode) == 1 and g > int(lib.gnbv_flightmap_classify_lds_max_grid() if cautious else lib.gnbv_flightmap_lds_max_grid()):
            raise _lib.GennbvHipError(f"BeliefFlightField: the bits of a {g}^3 grid do not fit LDS (map_mode 1)")
        self.rho = float(lattice.inflated_radius(body)) + float(margin)
        if not (np.isfinite(self.rho) and self.rho > 0.0):
            raise ValueError(f"BeliefFlightField: the inflated radius plus margin must be finite and > 0, got {self.rho}")
        self.grid_size, self.map_mode = g, int(map_mode)
        # (cautious: what sweep() hands to gnbv_sweep_tri -- straight legs only through seen space; the nodes' unknown goes to costly_map)
        self.unknown, self.unknown_blocks, self.outside_blocks = unknown, unknown in ("blocked", "costly"), outside == "blocked"
        self.range_gt = range_gt.to(device, torch.float32).contiguous()
        self.voxel_size = voxel_size.to(device, torch.float32).contiguous()
        assert self.range_gt.shape == (n, 6) and self.voxel_size.shape == (n, 3)
        blocked = torch.full((n, lattice.words), -1, dtype=torch.int32, device=device)  # all blocked until the first refresh
        super().__init__(types.SimpleNamespace(device=device, num_envs=n), lattice, body, mode=mode, blocked=blocked)
        self.blocked_map = torch.full_like(self.blocked, -1)
        self.costly_map = None
        if cautious:
            self.costly_map = torch.zeros_like(self.blocked)
            self.costly, self.penalty_mm = self.costly_map, penalty_mm
        self.refreshes = 0  # map launches so far
        self.sweeps = 0  # gnbv_sweep_tri launches so far
        self.map_i8 = torch.zeros(n, g ** 3, dtype=torch.int8, device=device) if self.shortcut else None  # all unknown until refresh()
        self.has_map = False  # a refresh() has filled the snapshot

    def refresh(self, tri: torch.Tensor) -> "BeliefFlightField":
        """gnbv_flight_blocked_tri on the current stream into `blocked_map` (unknown="costly": gnbv_flight_classify_tri into `blocked_map`
        and `costly_map`): tri [N, >= G^3] int8 or float32, unit element stride, any row stride (e.g.
        obs[:, state_dim:state_dim + grid_dim])."""
        n, g3 = self.num_envs, self.grid_size ** 3
        nx, ny, nz = self.lattice.dims
        head = (*_lib.tri_args(tri, n, g3, "BeliefFlightField.refresh"), self.grid_size, self.range_gt.data_ptr(),
                self.voxel_size.data_ptr(), n, nx, ny, nz, self._lo, self._h, self.rho)
        flags = (int(self.outside_blocks), int(bool(self.body.ground)))
        tail = (self.map_mode, _lib.stream_ptr(self.device))
        if self.costly_map is None:
            _lib.check(self.lib.gnbv_flight_blocked_tri(*head, int(self.unknown_blocks), *flags, self.blocked_map.data_ptr(), *tail),
                       "gnbv_flight_blocked_tri")
        else:
            _lib.check(self.lib.gnbv_flight_classify_tri(*head, *flags, self.blocked_map.data_ptr(), self.costly_map.data_ptr(), *tail),
                       "gnbv_flight_classify_tri")
        self.refreshes += 1
        if self.shortcut:
            self.map_i8.copy_(tri[:, :g3] if tri.dtype == torch.int8 else torch.sign(tri[:, :g3]))
            self.has_map = True
        return self

    def costly_at(self, nodes: torch.Tensor) -> torch.Tensor:
        """bool, the shape of nodes [N, ...] (integer node ids, row e of env e): the `costly_map` bit of each node; False for an id
        below 0.  Torch gathers, no host synchronisation."""
        if self.costly_map is None:
            raise _lib.GennbvHipError("BeliefFlightField.costly_at: the field has no costly_map (unknown='costly')")
        ids = nodes.long().reshape(self.num_envs, -1)
        safe = ids.clamp(min=0)
        bit = (self.costly_map.gather(1, safe >> 5).long() >> (safe & 31)) & 1
        return ((bit != 0) & (ids >= 0)).reshape(nodes.shape)

    def costly_count(self, nodes: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
        """int64 [N]: the number of costly nodes ENTERED on a walked route -- nodes int32 [N, L] from the target's node back to the
        source and count int32 [N] as path_nodes / path_into give them; the source (the last node) is not entered, and a count
        <= 0 gives 0.  penalty_mm times this is the penalty part of the field at the target."""
        inside = torch.arange(nodes.shape[1], device=self.device)[None] < (count[:, None].long() - 1)
        return (self.costly_at(nodes) & inside).sum(dim=1)

    def sweep(self, from_poses: torch.Tensor, to_poses: torch.Tensor, tri: Optional[torch.Tensor] = None, radius: Optional[float] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One gnbv_sweep_tri launch on the current stream: uint8 [N,K], the code (1 MAP | 2 OUTSIDE | 4 GROUND) of the sphere of
        `radius` (default `sweep_radius`) moved along the straight legs from from_poses [N, >= 3] (one start per env) or
        [N, K, >= 3] to to_poses [N, K, >= 3] f32, judged on `tri` (refresh()'s forms) or, where tri is None, on the snapshot
        `map_i8` of the last refresh -- with the field's unknown / outside flags, body.ground and map_mode.  0 = the map shows the
        leg in the clear.  No host synchronisation."""
        n = self.num_envs
        if tri is None:
            if not (self.shortcut and self.has_map):
                raise _lib.GennbvHipError("BeliefFlightField.sweep: no map snapshot (shortcut=True and a refresh()) and no tri given")
            tri = self.map_i8
        grid = _lib.tri_args(tri, n, self.grid_size ** 3, "BeliefFlightField.sweep")
        r = self.sweep_radius if radius is None else float(radius)
        if not (np.isfinite(r) and r > 0.0):
            raise ValueError(f"BeliefFlightField.sweep: radius must be finite and > 0, got {radius}")
        to_poses, k, to_row = self._targets(to_poses)
        _lib.require_cuda(from_poses)
        if from_poses.dtype != torch.float32 or from_poses.dim() not in (2, 3) or from_poses.shape[0] != n or from_poses.shape[-1] < 3 \
                or (from_poses.dim() == 3 and from_poses.shape[1] != k):
            raise _lib.GennbvHipError(f"BeliefFlightField.sweep: from_poses must be float32 [{n}, >= 3] or [{n}, {k}, >= 3], got "
                                      f"{from_poses.dtype} {tuple(from_poses.shape)}")
        if from_poses.stride(-1) != 1 or (n > 1 and from_poses.stride(0) < 3) or \
                (from_poses.dim() == 3 and k > 1 and from_poses.stride(1) != 0 and from_poses.stride(1) < 3):
            from_poses = from_poses.contiguous()
        f_env = max(int(from_poses.stride(0)), 3)
        f_item = 0 if from_poses.dim() == 2 or k == 1 else int(from_poses.stride(1))
        if out is None:
            out = torch.empty(n, k, dtype=torch.uint8, device=self.device)
        _lib.require_cuda(out)
        assert out.dtype == torch.uint8 and out.shape == (n, k) and out.is_contiguous()
        _lib.check(self.lib.gnbv_sweep_tri(*grid, self.grid_size, self.range_gt.data_ptr(), self.voxel_size.data_ptr(), n, from_poses.data_ptr(),
                                           f_env, f_item, to_poses.data_ptr(), k, to_row, r, int(self.unknown_blocks),
                                           int(self.outside_blocks), int(bool(self.body.ground)), out.data_ptr(), self.map_mode,
                                           _lib.stream_ptr(self.device)), "gnbv_sweep_tri")
        self.sweeps += 1
        return out

    def update(self, poses: torch.Tensor) -> "BeliefFlightField":
        """blocked = blocked_map with the bit of each env's own nearest node cleared (the drone is there; an env with a
        non-finite pose is left alone), then FlightField.update."""
        _lib.require_cuda(poses)
        lat = self.lattice
        near = lat.nearest_positions(poses[:, :3])  # NaN rows where there is no node
        has = torch.isfinite(near).all(-1)
        lo = torch.as_tensor(lat.lo, device=self.device)
        h = torch.as_tensor(lat.h, device=self.device)
        idx = torch.round((torch.where(has[:, None], near, lo.expand_as(near)) - lo) / torch.where(h > 0, h, torch.ones_like(h))).to(torch.int64)
        nx, ny, _ = lat.dims
        node = (idx[:, 2] * ny + idx[:, 1]) * nx + idx[:, 0]
        bit = torch.ones_like(node) << (node & 31)
        bit = torch.where(bit >= 2 ** 31, bit - 2 ** 32, bit).to(torch.int32)  # bit 31 as an int32
        clear = torch.where(has, ~bit, torch.full_like(bit, -1))
        self.blocked.copy_(self.blocked_map)
        rows = torch.arange(self.num_envs, device=self.device)
        self.blocked[rows, node >> 5] &= clear
        return super().update(poses)


def field_u32(t: torch.Tensor) -> np.ndarray:
    """An int32 tensor of u32 bits (field, cost_mm) as a numpy uint32 array on the host."""
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


__all__ = ["FlightField", "BeliefFlightField", "INF_MM", "field_u32"]

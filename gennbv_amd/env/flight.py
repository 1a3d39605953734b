"""FlightLattice: the node lattice of the collision-free flight search (csrc/flight.hip, ops/flight_field.py).

The task's position lattice (TaskConfig.clip_pose_low, action_unit, clip_pose_idx_low / _up) sub-sampled by `stride`:
node (i, j, k) sits at clip_pose_low[a] + stride * action_unit[a] * idx on axis a, idx = 0 ... (idx_up[a] - idx_low[a]) /
stride; h = stride * |action_unit| is the node spacing.  Poses are env-local, so one lattice serves every env.  The flat node
id is (k ny + j) nx + i; M = nx ny nz; an axis with action_unit == 0 has one node.

`stride` must divide idx_up - idx_low on every position axis: then the nodes span the whole pose lattice and every lattice pose
is within |h| / 2 of its nearest node (at most h[a] / 2 on each axis).

Soundness of a route over the lattice.  MeshScene.flight_blocked calls a node free when the sphere of radius
rho = (path_radius + |h| / 2) (1 + 2^-20) around it is free.  Every point of an edge between two 26-adjacent nodes is within
|h| / 2 of one of them (an edge is at most |h| long), and every lattice pose is within |h| / 2 of its nearest node; so
the body's sphere of radius path_radius, anywhere on pose -> nearest node -> free 26-neighbours -> nearest node -> pose, stays
inside the inflated sphere of a free node: the route is flyable.  It is conservative: gaps narrower than 2 rho are closed, and no
route is passed that the swept sphere could not fly.

Edge costs are integers: cost[|dx| | |dy| << 1 | |dz| << 2] = rint(1000 * ||d * h||) millimetres, computed once in fp64 here.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from .config import TaskConfig

INF_MM = 0xFFFFFFFF  # blocked / unreachable / no node, in every u32 table of the flight kernels
MAX_NODES_PER_AXIS = 1024


class FlightLattice:
    def __init__(self, cfg: TaskConfig, stride: int = 2):
        stride = int(stride)
        if stride < 1:
            raise ValueError(f"FlightLattice: stride must be >= 1, got {stride}")
        self.cfg, self.stride = cfg, stride
        dims, lo, h = [], [], []
        for a in range(3):
            span = int(cfg.clip_pose_idx_up[a]) - int(cfg.clip_pose_idx_low[a])
            unit = float(cfg.action_unit[a])
            if span < 0:
                raise ValueError(f"FlightLattice: axis {a} has clip_pose_idx_up < clip_pose_idx_low")
            if span % stride != 0:
                raise ValueError(f"FlightLattice: stride {stride} does not divide the {span} lattice steps of axis {a}")
            n = 1 if unit == 0.0 else span // stride + 1
            if n > MAX_NODES_PER_AXIS:
                raise ValueError(f"FlightLattice: axis {a} would have {n} nodes (at most {MAX_NODES_PER_AXIS})")
            dims.append(n)
            # (poses are action * unit + clip_pose_low with the action counted from 0: env/synthetic.poses_from_actions)
            lo.append(float(cfg.clip_pose_low[a]) + unit * int(cfg.clip_pose_idx_low[a]))
            h.append(abs(unit) * stride if n > 1 else 0.0)
            if unit < 0.0:
                lo[-1] -= h[-1] * (n - 1)
        self.dims: Tuple[int, int, int] = tuple(dims)
        self.lo = np.array(lo, np.float64)
        self.h = np.array(h, np.float64)
        self.num_nodes = dims[0] * dims[1] * dims[2]
        self.words = (self.num_nodes + 31) // 32
        self.h_norm = float(np.sqrt((self.h ** 2).sum()))
        self.cost = edge_costs(self.h)
        if self.num_nodes * int(self.cost.max()) >= INF_MM - 1:
            raise ValueError("FlightLattice: route lengths would not fit 32 bits of millimetres")

    # ------------------------------------------------------------------
    def inflated_radius(self, body) -> float:
        """rho of the module docstring for a CollisionBody."""
        return (float(body.path_radius) + 0.5 * self.h_norm) * (1.0 + 2.0 ** -20)

    def node_index(self) -> np.ndarray:
        """(i, j, k) [M, 3] int64 of every node, in id order."""
        nx, ny, nz = self.dims
        c = np.arange(self.num_nodes, dtype=np.int64)
        return np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], -1)

    def node_positions(self) -> np.ndarray:
        """[M, 3] fp64 node positions, in id order."""
        return self.lo[None] + self.h[None] * self.node_index()

    def nearest_np(self, p) -> np.ndarray:
        """Node id [...] int64 of positions p [..., >= 3] (any float type; taken to fp64), -1 for a non-finite x, y or z:
        per axis clamp(floor((p - lo) / h + 0.5), 0, n - 1), 0 on an axis with one node."""
        p = np.asarray(p)[..., :3].astype(np.float64)
        fin = np.isfinite(p).all(-1)
        idx = []
        for a in range(3):
            n = self.dims[a]
            if n == 1:
                idx.append(np.zeros(p.shape[:-1], np.int64))
                continue
            with np.errstate(invalid="ignore"):
                f = np.floor((p[..., a] - self.lo[a]) / self.h[a] + 0.5)
            idx.append(np.clip(np.where(fin, f, 0.0), 0, n - 1).astype(np.int64))
        nx, ny, _ = self.dims
        return np.where(fin, (idx[2] * ny + idx[1]) * nx + idx[0], -1)

    def nearest_positions(self, p: torch.Tensor) -> torch.Tensor:
        """torch twin of the nearest-node rule: the fp64 position [..., 3] of the nearest node of p [..., >= 3] (NaN where
        there is none), on p's device."""
        q = p[..., :3].to(torch.float64)
        lo = torch.as_tensor(self.lo, device=p.device)
        h = torch.as_tensor(self.h, device=p.device)
        top = torch.tensor([n - 1 for n in self.dims], dtype=torch.float64, device=p.device)
        safe = torch.where(h > 0, h, torch.ones_like(h))
        idx = torch.minimum(torch.clamp(torch.floor((q - lo) / safe + 0.5), min=0.0), top)
        pos = lo + h * idx
        fin = torch.isfinite(q).all(-1, keepdim=True)
        return torch.where(fin, pos, torch.full_like(pos, float("nan")))


def edge_costs(h) -> np.ndarray:
    """cost[8] u32, index |dx| | |dy| << 1 | |dz| << 2: rint(1000 * ||d * h||) in fp64 (millimetres); cost[0] = 0."""
    h = np.asarray(h, np.float64)
    out = np.zeros(8, np.uint32)
    for b in range(8):
        d = np.array([(b >> a) & 1 for a in range(3)], np.float64)
        out[b] = np.uint32(np.rint(1000.0 * math.sqrt(float(((d * h) ** 2).sum()))))
    return out


def pack_bits(blocked: torch.Tensor, words: Optional[int] = None) -> torch.Tensor:
    """bool [N, M] -> int32 [N, ceil(M / 32)] (bit c & 31 of word c >> 5), padding bits SET."""
    n, m = blocked.shape
    words = (m + 31) // 32 if words is None else int(words)
    full = torch.ones(n, words * 32, dtype=torch.bool, device=blocked.device)
    full[:, :m] = blocked
    shift = torch.arange(32, dtype=torch.int64, device=blocked.device)
    v = (full.view(n, words, 32).to(torch.int64) << shift).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).contiguous()

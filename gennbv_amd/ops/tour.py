"""route_tour: order a set of points into a short open flight tour (csrc/tour.hip gnbv_tour_route), and euclid_mm, the
straight-line leg lengths for envs without a flight field.

    D = field.pairwise_mm(points, count)      # or euclid_mm(points, count): int32 [N,P,P] holding u32 millimetres
    res = route_tour(D, count)                # TourResult(order [N,P], routed [N], length_mm [N] int64, status [N])

Point 0 of every env is the fixed start and the path is open.  The tour is nearest neighbour from 0 improved by best-improvement
2-opt, on integers with fixed tie rules: one right answer (include/gennbv_hip.h has the exact rule and the status bits).  Outputs
are preallocated per shape and reused: a result is valid until the next call with the same shape.  No host synchronisation.
route_tour is GPU only, no CPU fallback; euclid_mm is plain tensor arithmetic on the device of its input.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from .. import _lib
from ..env.flight import INF_MM

MAX_POINTS = 128
MAX_ENVS = 65535
STATUS_MISSING_LEG, STATUS_CAPPED, STATUS_BAD_COUNT = 1, 2, 4


class TourResult(NamedTuple):
    order: torch.Tensor      # int32 [N,P]: the route (order[:, :routed], order[:, 0] == 0), then every other index, ascending
    routed: torch.Tensor     # int32 [N]: points on the route, the start included
    length_mm: torch.Tensor  # int64 [N]: the sum of the legs along the route
    status: torch.Tensor     # int32 [N]: bit 1 a missing leg was read, bit 2 the move cap was hit, bit 4 count outside 1..P


_outputs = {}  # (device, n, p) -> TourResult


def route_tour(dist_mm: torch.Tensor, count: Optional[torch.Tensor] = None, max_moves: Optional[int] = None) -> TourResult:
    """gnbv_tour_route on the current stream.  dist_mm int32 [N,P,P] of u32 bits (-1 = 0xFFFFFFFF = no route), contiguous,
    P <= 128; count int32 [N] (None: P); max_moves (None: P * P) caps the 2-opt moves."""
    _lib.require_cuda(dist_mm, count)
    if dist_mm.dtype != torch.int32 or dist_mm.dim() != 3 or dist_mm.shape[1] != dist_mm.shape[2] or not dist_mm.is_contiguous():
        raise _lib.GennbvHipError(f"route_tour: dist_mm must be contiguous int32 [N, P, P], got {dist_mm.dtype} {tuple(dist_mm.shape)}")
    n, p = int(dist_mm.shape[0]), int(dist_mm.shape[1])
    if not (1 <= n <= MAX_ENVS and 1 <= p <= MAX_POINTS):
        raise _lib.GennbvHipError(f"route_tour: N in 1..{MAX_ENVS} and P in 1..{MAX_POINTS}, got N = {n}, P = {p}")
    if count is not None and (count.dtype != torch.int32 or count.shape != (n,) or not count.is_contiguous() or count.device != dist_mm.device):
        raise _lib.GennbvHipError(f"route_tour: count must be contiguous int32 [{n}] on {dist_mm.device}, got {count.dtype} {tuple(count.shape)}")
    moves = p * p if max_moves is None else int(max_moves)
    if moves < 0:
        raise _lib.GennbvHipError(f"route_tour: max_moves >= 0, got {moves}")
    dev = dist_mm.device
    key = (dev, n, p)
    if key not in _outputs:
        _outputs[key] = TourResult(torch.empty(n, p, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                                   torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    res = _outputs[key]
    a = _lib.GnbvTourRoute()
    a.n, a.p, a.dist_mm, a.count, a.max_moves = n, p, dist_mm.data_ptr(), _lib.ptr(count), moves
    a.order, a.routed, a.length_mm, a.status = res.order.data_ptr(), res.routed.data_ptr(), res.length_mm.data_ptr(), res.status.data_ptr()
    _lib.check(_lib.load().gnbv_tour_route(C.byref(a), _lib.stream_ptr(dev)), "gnbv_tour_route")
    return res


def u32_bits(mm: torch.Tensor) -> torch.Tensor:
    """int64 values in 0 .. 2^32 - 1 -> the int32 tensor holding the same u32 bits (the cost_mm convention)."""
    return torch.where(mm >= 2 ** 31, mm - 2 ** 32, mm).to(torch.int32)


def euclid_mm(points: torch.Tensor, count: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [N,P,P] of u32 bits: rint(1000 * ||points[e, a] - points[e, b]||) in fp64 (dx dx + dy dy + dz dz summed in this
    order, square root, times 1000, round half to even), the straight flight in millimetres; 0xFFFFFFFF where the distance is
    not finite or not below 0xFFFFFFFE, and in every row and column at or above count[e] (int32 [N], None: P).
    points [N, P, >= 3], any float type."""
    if points.dim() != 3 or points.shape[2] < 3 or not points.is_floating_point():
        raise _lib.GennbvHipError(f"euclid_mm: points must be floating point [N, P, >= 3], got {points.dtype} {tuple(points.shape)}")
    n, p = int(points.shape[0]), int(points.shape[1])
    q = points[..., :3].to(torch.float64)
    d = q[:, :, None, :] - q[:, None, :, :]
    mm = torch.round(1000.0 * torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))
    ok = torch.isfinite(mm) & (mm < float(INF_MM - 1))
    if count is not None:
        if count.shape != (n,):
            raise _lib.GennbvHipError(f"euclid_mm: count must be [{n}], got {tuple(count.shape)}")
        inside = torch.arange(p, device=points.device)[None] < count.to(points.device)[:, None]
        ok &= inside[:, :, None] & inside[:, None, :]
    out = torch.where(ok, mm, torch.zeros_like(mm)).to(torch.int64)
    return u32_bits(torch.where(ok, out, torch.full_like(out, INF_MM))).contiguous()


__all__ = ["TourResult", "route_tour", "euclid_mm", "u32_bits", "MAX_POINTS", "STATUS_MISSING_LEG", "STATUS_CAPPED", "STATUS_BAD_COUNT"]

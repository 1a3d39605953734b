"""ScanAccumulator: the reconstruction-accuracy metric of the evaluation env on the device (csrc/scan.hip).

The reference keeps a growing list of back-projected points per env (env_eval_gennbv.py:156-164), rounds it to 1 cm,
de-duplicates it and scores it by Chamfer distance x 100 when the env finishes (:253-263).  Here each env holds the SET of
its 1 cm keys in a device hash table: `add_frame` adds one step's frames of every env in one launch, `score(done_mask)`
scores every flagged env that has not been scored yet in one fixed sequence of launches, `clear(mask)` empties the sets of
the envs that reset.  None of the three synchronises with the host; results are read back when the caller asks
(`results()`, `points(e)`), and a set that overflowed or saw a non-finite / out-of-range point raises there instead of
returning a wrong value.

The GT clouds are static: they are sorted spatially (Morton order) and given a bounding-box tree once, here, with torch.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from .. import _lib

DEFAULT_EPISODE_STEPS = 30  # the reference's evaluation episode (config_gennbv_eval.py:7): reset frame + 30 steps
LEAF = 32                   # points per leaf of the trees (csrc/scan.hip kLeaf)
FLAG_OVERFLOW, FLAG_RANGE = 1, 2


def _spread3(v: torch.Tensor) -> torch.Tensor:
    v = v & 0x1FFFFF
    v = (v | (v << 32)) & 0x1F00000000FFFF
    v = (v | (v << 16)) & 0x1F0000FF0000FF
    v = (v | (v << 8)) & 0x100F00F00F00F00F
    v = (v | (v << 4)) & 0x10C30C30C30C30C3
    v = (v | (v << 2)) & 0x1249249249249249
    return v


def _gt_tree(y: torch.Tensor):
    """Morton-sorted points, their original indices and the heap of leaf / node boxes of one GT cloud (any order of the
    points gives the same minima; the spatial order makes the boxes tight and the queries coherent)."""
    m = y.shape[0]
    lo, hi = y.min(0).values, y.max(0).values
    q = ((y - lo) / torch.clamp(hi - lo, min=1e-30) * 2097151.0).floor().clamp(0, 2097151).to(torch.int64)
    code = (_spread3(q[:, 0]) << 2) | (_spread3(q[:, 1]) << 1) | _spread3(q[:, 2])
    perm = torch.argsort(code, stable=True)
    ys = y[perm].contiguous()
    leaves = -(-m // LEAF)
    p = 1
    while p < leaves:
        p <<= 1
    padded = torch.cat([ys, ys[-1:].expand(leaves * LEAF - m, 3)]).view(leaves, LEAF, 3)
    blo = torch.full((2 * p, 3), float("inf"), dtype=torch.float32, device=y.device)
    bhi = torch.full((2 * p, 3), float("-inf"), dtype=torch.float32, device=y.device)
    blo[p:p + leaves], bhi[p:p + leaves] = padded.min(1).values, padded.max(1).values
    s = p // 2
    while s >= 1:
        blo[s:2 * s] = torch.minimum(blo[2 * s:4 * s:2], blo[2 * s + 1:4 * s:2])
        bhi[s:2 * s] = torch.maximum(bhi[2 * s:4 * s:2], bhi[2 * s + 1:4 * s:2])
        s //= 2
    z = torch.zeros(2 * p, 1, dtype=torch.float32, device=y.device)
    nodes = torch.stack([torch.cat([blo, z], 1), torch.cat([bhi, z], 1)], 1)  # [2P, 2, 4]
    return torch.cat([ys, torch.zeros(m, 1, dtype=torch.float32, device=y.device)], 1), perm.to(torch.int32), p, nodes


class ScanAccumulator:
    """Per-env sets of 1 cm scan keys and their Chamfer accuracy against `pc_gt` (one [m_e, 3] cloud per env).

    capacity_per_env: the most unique keys an env can hold (rounded up to a multiple of 64); default
    h * w * (DEFAULT_EPISODE_STEPS + 1), every pixel of every frame of one evaluation episode.  Device memory:
    16 B per key of capacity for the set, about 40 B per key of capacity for the scoring workspace."""

    def __init__(self, num_envs: int, pc_gt: Sequence[torch.Tensor], h: int, w: int, inv_intri, depth_sense_dist: float,
                 capacity_per_env: Optional[int] = None, device="cuda:0"):
        self._lib = lib = _lib.load()
        self.device = torch.device(device)
        n = self.num_envs = int(num_envs)
        self.h, self.w = int(h), int(w)
        cap = self.h * self.w * (DEFAULT_EPISODE_STEPS + 1) if capacity_per_env is None else int(capacity_per_env)
        cap = -(-cap // 64) * 64
        if n <= 0 or cap <= 0 or cap >= 1 << 31:
            raise _lib.GennbvHipError(f"ScanAccumulator: bad num_envs {n} / capacity {cap}")
        self.capacity = cap
        self.inv_intri = torch.as_tensor(inv_intri, dtype=torch.float32).detach().reshape(3, 3).cpu().contiguous()  # [host]
        self.depth_sense_dist = float(depth_sense_dist)
        dev = self.device
        self.table = torch.full((n, cap), -1, dtype=torch.int64, device=dev)  # all-ones bytes = empty slot
        self.keys = torch.empty((n, cap), dtype=torch.int64, device=dev)
        self.counts = torch.zeros(n, dtype=torch.int32, device=dev)
        self._state = torch.zeros(3, n, dtype=torch.int32, device=dev)  # accuracy (fp32 bits), scored, flags: one read-back
        self.accuracy_cm = self._state[0].view(torch.float32)
        self.scored = self._state[1]
        self.flags = self._state[2]
        self._all = torch.ones(n, dtype=torch.uint8, device=dev)
        self._set = _lib.GnbvScanSet(n, cap, self.table.data_ptr(), self.keys.data_ptr(), self.counts.data_ptr(), self.flags.data_ptr())

        if len(pc_gt) != n:
            raise _lib.GennbvHipError(f"ScanAccumulator: {len(pc_gt)} GT clouds for {n} envs")
        pts, orig, pow2, nodes, starts, node_starts = [], [], [], [], [0], []
        n_nodes = 0
        for y in pc_gt:
            y = torch.as_tensor(y).to(dev, torch.float32).reshape(-1, 3).contiguous()
            if y.shape[0] == 0 or not bool(torch.isfinite(y).all()):
                raise _lib.GennbvHipError("ScanAccumulator: every GT cloud needs at least one point, all finite")
            p4, o, p, nd = _gt_tree(y)
            pts.append(p4)
            orig.append(o)
            pow2.append(p)
            nodes.append(nd)
            starts.append(starts[-1] + y.shape[0])
            node_starts.append(n_nodes)
            n_nodes += nd.shape[0]
        self.gt_points = torch.cat(pts).contiguous()
        self.gt_orig = torch.cat(orig).contiguous()
        self.gt_nodes = torch.cat(nodes).contiguous()
        self.gt_start = torch.tensor(starts, dtype=torch.int64, device=dev)
        self.gt_node_start = torch.tensor(node_starts, dtype=torch.int64, device=dev)
        self.gt_pow2 = torch.tensor(pow2, dtype=torch.int32, device=dev)
        self._gt = _lib.GnbvScanGt(n, starts[-1], self.gt_start.data_ptr(), self.gt_points.data_ptr(), self.gt_orig.data_ptr(),
                                   self.gt_node_start.data_ptr(), self.gt_pow2.data_ptr(), self.gt_nodes.data_ptr())
        need = int(lib.gnbv_scan_workspace_bytes(n, cap, starts[-1]))
        self._ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        self._ws_ptr = (self._ws.data_ptr() + 255) & ~255
        self._ws_bytes = need

    # -- hot path: no host synchronisation ------------------------------------------------------------------------
    def _mask(self, mask: torch.Tensor) -> torch.Tensor:
        _lib.require_cuda(mask)
        if mask.shape != (self.num_envs,):
            raise _lib.GennbvHipError(f"mask of shape {tuple(mask.shape)} for {self.num_envs} envs")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        elif mask.dtype != torch.uint8:
            mask = (mask != 0).view(torch.uint8)
        return mask.contiguous()

    def add_frame(self, depth_raw: torch.Tensor, seg_raw: torch.Tensor, c2w: torch.Tensor) -> None:
        """Add every env's foreground keys of one frame: depth_raw / seg_raw [N, H, W] as rendered, c2w [N, 4, 4]."""
        _lib.require_cuda(depth_raw, seg_raw, c2w)
        d, s, m = depth_raw.contiguous().float(), seg_raw.contiguous().float(), c2w.contiguous().float()
        shp = (self.num_envs, self.h, self.w)
        if d.shape != shp or s.shape != shp or m.shape != (self.num_envs, 4, 4):
            raise _lib.GennbvHipError(f"add_frame: depth {tuple(d.shape)}, seg {tuple(s.shape)}, c2w {tuple(m.shape)} for {shp}")
        _lib.check(self._lib.gnbv_scan_add_frame(C.byref(self._set), d.data_ptr(), s.data_ptr(), m.data_ptr(), self.inv_intri.data_ptr(),
                                                 self.h, self.w, self.depth_sense_dist, _lib.stream_ptr(self.device)), "gnbv_scan_add_frame")

    def score(self, done_mask: torch.Tensor) -> None:
        """Score every env with done_mask[e] set whose set is non-empty and that has no score yet (the first finished
        episode of an env is kept: env_eval_gennbv.py:262-263)."""
        m = self._mask(done_mask)
        _lib.check(self._lib.gnbv_scan_score(C.byref(self._set), C.byref(self._gt), m.data_ptr(), self.accuracy_cm.data_ptr(),
                                             self.scored.data_ptr(), self._ws_ptr, self._ws_bytes, _lib.stream_ptr(self.device)),
                   "gnbv_scan_score")

    def clear(self, mask: torch.Tensor) -> None:
        """Empty the sets of the envs with mask[e] set (reset_idx, env_eval_gennbv.py:321-322)."""
        m = self._mask(mask)
        _lib.check(self._lib.gnbv_scan_clear(C.byref(self._set), m.data_ptr(), _lib.stream_ptr(self.device)), "gnbv_scan_clear")

    def reset(self) -> None:
        """A new evaluation: every set empty, no scores, no flags."""
        self.clear(self._all)
        self._state.zero_()

    # -- read-back ------------------------------------------------------------------------------------------------------
    def _raise_on(self, flags, envs):
        bad = [e for e in envs if int(flags[e])]
        if bad:
            what = {e: ("overflow " if int(flags[e]) & FLAG_OVERFLOW else "") + ("non-finite/out-of-range point" if int(flags[e]) & FLAG_RANGE else "")
                    for e in bad}
            raise _lib.GennbvHipError(f"ScanAccumulator: env sets are invalid (capacity {self.capacity}): {what}")

    def results(self) -> Dict[int, float]:
        """{env: accuracy in cm} of the scored envs, one device -> host copy; raises if any env's set is flagged."""
        st = self._state.cpu()
        self._raise_on(st[2], range(self.num_envs))
        acc = st[0].view(torch.float32)
        return {e: float(acc[e]) for e in range(self.num_envs) if int(st[1, e])}

    def points(self, e: int) -> torch.Tensor:
        """Env e's unique cloud [k, 3] fp32 in lexicographic order: unique_rounded_points of the points added since its last
        clear, bit for bit."""
        e = int(e)
        if not 0 <= e < self.num_envs:
            raise IndexError(e)
        self._raise_on(self.flags.cpu(), [e])
        k = int(self.counts[e])
        out = torch.empty((k, 3), dtype=torch.float32, device=self.device)
        if k:
            _lib.check(self._lib.gnbv_scan_export(C.byref(self._set), e, out.data_ptr(), self._ws_ptr, self._ws_bytes,
                                                  _lib.stream_ptr(self.device)), "gnbv_scan_export")
        return out


"""ViewPool: a fixed pool of candidate views per env whose visible ground truth is traced ONCE into bit masks
(csrc/viewcover.hip gnbv_view_cover_masks), and greedy set cover on those masks (csrc/covergreedy.hip gnbv_cover_greedy).

With the scene and the candidate set fixed, S(e, j) & gt does not change during an episode; only the scanned set does.  So a
decision over the pool is popcount(mask & ~scanned) per candidate and an argmax -- memory speed instead of trace speed -- and
`plan(T)` is the classic greedy set-cover next-best-view plan: T views, each the one that adds the most still-uncovered
ground-truth voxels.  `union_bits()` is the pool's observable ground truth.  All results are integers with one right answer
(include/gennbv_hip.h has the exact definitions).  Outputs are preallocated and reused: a result is valid until the next call
of the same method.  GPU only, no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ..env import synthetic as S
from ..env.config import TaskConfig
from .cover_greedy import CoverGreedy, check_contact, check_covered, check_rounds

MAX_GRID = 128
MAX_POOL = 4096
UNKNOWN = 2 ** 31 - 1  # an upper bound that says nothing (GnbvCoverGreedy.ub)


class ViewPool:
    def __init__(self, mesh, cfg: TaskConfig, range_gt: torch.Tensor, voxel_size: torch.Tensor, gt_bits: torch.Tensor,
                 poses: torch.Tensor, stride: int = 1, inv_intrinsics: Optional[torch.Tensor] = None, batch: int = 64,
                 max_bytes: int = 8 << 30, body=None, collision_mesh=None, chunk: int = 0, window: int = 0):
        """poses [N,P,6] f32 (x, y, z, roll, pitch, yaw), env-local; gt_bits int32 [N, words] in the updater's layout.  `body`
        (a CollisionBody): candidates whose pose collides with `collision_mesh` (default: mesh) are never chosen unless all
        of an env's are.  `chunk` / `window` go to the kernel (any value gives the same masks)."""
        if mesh.device.type != "cuda":
            raise _lib.GennbvHipError("ViewPool runs on the GPU only (no CPU fallback): build the MeshScene on a cuda device")
        g = int(cfg.grid_size)
        if not 2 <= g <= MAX_GRID:
            raise _lib.GennbvHipError(f"ViewPool: grid_size in 2..{MAX_GRID}, got {g}")
        self.lib = _lib.load()
        self.device = dev = torch.device(mesh.device)
        n = self.num_envs = int(mesh.num_envs)
        if poses.dim() != 3 or poses.shape[0] != n or poses.shape[2] != 6 or not 1 <= poses.shape[1] <= MAX_POOL:
            raise _lib.GennbvHipError(f"ViewPool: poses must be [{n}, P, 6] with P in 1..{MAX_POOL}, got {tuple(poses.shape)}")
        if int(stride) < 1 or int(batch) < 1:
            raise _lib.GennbvHipError(f"ViewPool: stride >= 1 and batch >= 1, got stride {stride}, batch {batch}")
        p = self.pool_size = int(poses.shape[1])
        self.g, self.words = g, int(self.lib.gnbv_grid_bit_words(g))
        nbytes = n * p * self.words * 4
        if nbytes > int(max_bytes):
            raise _lib.GennbvHipError(f"ViewPool: the masks of {n} envs x {p} views x {self.words} words take {nbytes} bytes, "
                                      f"above max_bytes = {int(max_bytes)}")
        _lib.require_cuda(gt_bits)
        if gt_bits.dtype != torch.int32 or gt_bits.shape != (n, self.words) or not gt_bits.is_contiguous():
            raise _lib.GennbvHipError(f"ViewPool: gt_bits must be contiguous int32 [{n}, {self.words}] (gnbv_grid_bit_words), "
                                      f"got {gt_bits.dtype} {tuple(gt_bits.shape)}")
        self.poses = poses.to(dev, torch.float32).contiguous()
        self.gt_bits = gt_bits
        h, w = int(cfg.camera_height), int(cfg.camera_width)
        kinv = S.inverse_intrinsics(h, w, cfg.horizontal_fov) if inv_intrinsics is None else inv_intrinsics
        kinv_host = kinv.detach().to("cpu", torch.float32).contiguous()
        assert kinv_host.shape == (3, 3)
        rng = range_gt.to(dev, torch.float32).contiguous()
        vox = voxel_size.to(dev, torch.float32).contiguous()
        assert rng.shape == (n, 6) and vox.shape == (n, 3)

        # ---- the masks, once: batches of `batch` candidates; the union of all masks comes from the same launches (seen_bits)
        self.masks = torch.empty(n, p, self.words, dtype=torch.int32, device=dev)
        self._union = torch.zeros(n, self.words, dtype=torch.int32, device=dev)
        scene = mesh.c_struct()
        a = _lib.GnbvViewCover()
        a.n, a.g = n, g
        a.range_gt, a.voxel_size, a.inv_intri = rng.data_ptr(), vox.data_ptr(), kinv_host.data_ptr()
        a.h, a.w, a.stride, a.depth_sense_dist = h, w, int(stride), float(cfg.depth_sense_dist)
        a.gt_bits, a.scanned_bits, a.cover, a.seen_bits = gt_bits.data_ptr(), None, None, self._union.data_ptr()
        a.chunk, a.window = int(chunk), int(window)
        st = _lib.stream_ptr(dev)
        kb = min(int(batch), p)
        stage = None if kb == p else torch.empty(n, kb, self.words, dtype=torch.int32, device=dev)
        for j0 in range(0, p, kb):
            j1 = min(p, j0 + kb)
            part = self.poses if stage is None else self.poses[:, j0:j1].contiguous()
            out = self.masks if stage is None else stage.view(-1)[:n * (j1 - j0) * self.words].view(n, j1 - j0, self.words)
            a.k, a.poses = j1 - j0, part.data_ptr()
            _lib.check(self.lib.gnbv_view_cover_masks(C.byref(scene), C.byref(a), out.data_ptr(), st), "gnbv_view_cover_masks")
            if stage is not None:
                self.masks[:, j0:j1].copy_(out)
        del stage
        self.contact = None
        if body is not None:
            cm = mesh if collision_mesh is None else collision_mesh
            self.contact = cm.collide_candidates(self.poses, body, out=torch.zeros(n, p, dtype=torch.uint8, device=dev))

        # ---- greedy set cover: preallocated outputs
        self._gains = torch.empty(n, p, dtype=torch.int32, device=dev)
        self._choice1 = torch.empty(n, 1, dtype=torch.int32, device=dev)
        self._gain1 = torch.empty(n, 1, dtype=torch.int32, device=dev)
        self._cg = CoverGreedy(self.lib, dev, n, p, self.words)

    def _covered(self, who, covered_bits):
        return check_covered(who, covered_bits, self.num_envs, self.words)

    def _round(self, covered_in, gains0, ub, lazy, contact=None):
        """one round into _choice1 / _gain1, no covered_out"""
        self._cg.launch(1, self.masks, covered_in, self.contact if contact is None else contact, self._choice1, self._gain1, None,
                        gains0, ub, lazy)

    def select(self, covered_bits: Optional[torch.Tensor], ub: Optional[torch.Tensor] = None, contact: Optional[torch.Tensor] = None):
        """One round against covered_bits [N, words] (None = nothing covered) -> (choice [N], gain [N]) int32.  `ub` [N,P]
        int32: upper bounds carried from call to call (GnbvCoverGreedy.ub: read, used for lazy evaluation, rewritten; UNKNOWN
        says nothing; valid while each env's covered set only grows -- reset an env's row to UNKNOWN when it shrinks).  Without
        `ub` every candidate is evaluated.  `contact` [N,P] u8 replaces the pool's static contact for this call only (e.g.
        the static contact | the flight from the current pose); a bound does not depend on contact -- the kernel keeps a
        contact candidate's bound as it is, still >= its gain -- so `ub` stays valid while the contact set changes."""
        cov = self._covered("ViewPool.select", covered_bits)
        check_contact("ViewPool.select", contact, self.num_envs, self.pool_size)
        if ub is not None:
            _lib.require_cuda(ub)
            if ub.dtype != torch.int32 or ub.shape != (self.num_envs, self.pool_size) or not ub.is_contiguous():
                raise _lib.GennbvHipError(f"ViewPool.select: ub must be contiguous int32 [{self.num_envs}, {self.pool_size}]")
            self._round(cov, None, ub, True, contact)
        else:
            self._round(cov, self._gains, None, False, contact)
        return self._choice1[:, 0], self._gain1[:, 0]

    def plan(self, rounds: int, covered_bits: Optional[torch.Tensor] = None, lazy: bool = True):
        """Greedy set cover: `rounds` views from the pool, starting from covered_bits (None = nothing covered; not modified)
        -> (choice [N,T], gain [N,T], covered [N, words] = covered_bits | the chosen masks).  `lazy` changes the work, not the
        result.  The plan keeps the pool's static contact (poses that collide): an offline plan has no "current pose" per
        round, so no flight is tested."""
        rounds = check_rounds("ViewPool.plan", rounds)
        cov = self._covered("ViewPool.plan", covered_bits)
        choice, gain, covered, _ = self._cg.outputs(rounds)
        self._cg.launch(rounds, self.masks, cov, self.contact, choice, gain, covered, self._gains, None, lazy)
        return choice, gain, covered

    def gains(self, covered_bits: Optional[torch.Tensor]) -> torch.Tensor:
        """[N,P] int32: popcount(mask & ~covered_bits) of every candidate."""
        self._round(self._covered("ViewPool.gains", covered_bits), self._gains, None, False)
        return self._gains

    def union_bits(self) -> torch.Tensor:
        """[N, words] int32: the OR of all masks, the pool's observable ground truth (computed once, with the masks)."""
        return self._union
